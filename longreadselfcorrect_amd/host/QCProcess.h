// QCProcess.h -- the per-read quality checks of `stride filter`, batch at a time: same parameters, order of the checks and
// counters as the reference's Algorithm/QCProcess.h:18-141 and QCProcess.cpp:54-88,268-441.  The duplicate check is
// lrsc_dupcheck_reads (one device call per batch), the homopolymer check's k-mer counts are lrsc_find_kmers calls, one per
// composite length; the rest is host code.
#pragma once
#include <cstddef>
#include <iosfwd>
#include <string>
#include <vector>

#include "../../include/lrsc.h"
#include "SequenceWorkItem.h"

namespace stride {

struct QCParameters {                    // QCParameters::setDefaults
    lrsc_ctx* ctx = nullptr;             // the index to check against, on its device
    lrsc_dupcheck* dupcheck = nullptr;   // the run's shared bit vector
    bool checkDuplicates = true;
    bool substringOnly = false;
    bool checkKmer = true;               // `stride filter` cannot switch it on (StriDe/filter.cpp:87,252); not implemented here
    bool checkHPRuns = true;
    bool checkDegenerate = true;
    int verbose = 0;
    int kmerLength = 27;
    int kmerThreshold = 2;
    size_t hpKmerLength = 51;
    size_t hpHardAcceptCount = 10;
    double hpMinProportion = 0.1f;
    size_t hpMinLength = 6;
    size_t hpMinContext = 5;
    double degenProportion = 0.90;
};

struct QCResult {
    bool kmerPassed = true, dupPassed = true, hpPassed = true, degenPassed = true;
    bool passed() const { return kmerPassed && dupPassed && hpPassed && degenPassed; }
};

class QCProcess {
public:
    explicit QCProcess(const QCParameters& params) : m_params(params) {}
    // QCProcess::process for every read of the batch, in order.  dup (may be null) receives the duplicate check's records, which
    // are computed whether or not checkDuplicates is set: the caller's guard needs the '$' intervals.
    std::vector<QCResult> process_batch(const std::vector<SequenceWorkItem>& items, std::vector<lrsc_dup_result>* dup);

private:
    void homopolymerCheck(const std::vector<SequenceWorkItem>& items, std::vector<QCResult>& results);
    bool degenerateCheck(const SequenceWorkItem& item) const;
    QCParameters m_params;
};

class QCPostProcess {                    // pass / discard writers and the six counters
public:
    QCPostProcess(std::ostream* pCorrectedWriter, std::ostream* pDiscardWriter);
    ~QCPostProcess();                    // prints the counters
    void process(const SequenceWorkItem& item, const QCResult& result);

private:
    std::ostream* m_pCorrectedWriter;
    std::ostream* m_pDiscardWriter;
    size_t m_readsKept = 0, m_readsDiscarded = 0, m_readsFailedKmer = 0, m_readsFailedDup = 0, m_readsFailedHP = 0, m_readsFailedDegen = 0;
};

} // namespace stride
