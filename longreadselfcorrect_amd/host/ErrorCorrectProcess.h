// ErrorCorrectProcess.h -- the per-read work and the post-processing of `stride correct -a kmer`, batch at a time: same results,
// counters and metrics as the reference's Algorithm/ErrorCorrectProcess.h:24-160 and ErrorCorrectProcess.cpp:287-438,550-676.
// The k-mer correction is lrsc_kmer_correct, one device call per batch; the overlap and hybrid algorithms are not built.
#pragma once
#include <cstddef>
#include <cstdint>
#include <iosfwd>
#include <map>
#include <string>
#include <vector>

#include "../../include/lrsc.h"
#include "SequenceWorkItem.h"

namespace stride {

struct ErrorCorrectParameters {
    lrsc_ctx* ctx = nullptr;             // the index to count in, on its device
    int kmerLength = 31;
    int kmerThreshold = 3;               // CorrectionThresholds::setBaseMinSupport
    int numKmerRounds = 10;
    int highQualityCutoff = 20;          // CorrectionThresholds' m_highQualityCutoff
    std::string readsFile;               // for messages
};

struct ErrorCorrectResult {
    std::string correctSequence;
    bool kmerQC = false, overlapQC = false;
};

class ErrorCorrectProcess {
public:
    explicit ErrorCorrectProcess(const ErrorCorrectParameters& params) : m_params(params) {}
    // ErrorCorrectProcess::kmerCorrection for every read of the batch, in order.  A quality string that is not one character of
    // '!' or above per base ends the run with a message that names the read.  A read with a base other than A, C, G, T is
    // returned as it is with kmerQC = false (one warning per run); so is an empty one.
    std::vector<ErrorCorrectResult> process_batch(const std::vector<SequenceWorkItem>& items);

private:
    ErrorCorrectParameters m_params;
    bool m_warnedOtherBases = false;
};

// Util/Metrics.h:15-58
template <class Key>
class ErrorCountMap {
public:
    void incrementSample(const Key& key) { ++m_data[key].num_samples; }
    void incrementError(const Key& key) { ++m_data[key].num_errors; }
    void write(std::ostream* pWriter, const std::string& leader, const std::string& header) const;

private:
    struct ErrorCount { int64_t num_samples = 0, num_errors = 0; };
    std::map<Key, ErrorCount> m_data;
};

class ErrorCorrectPostProcess {          // corrected / discard writers, the three counters, the metrics
public:
    ErrorCorrectPostProcess(std::ostream* pCorrectedWriter, std::ostream* pDiscardWriter, bool bCollectMetrics);
    ~ErrorCorrectPostProcess();          // prints the counters
    void process(const SequenceWorkItem& item, const ErrorCorrectResult& result);
    void writeMetrics(std::ostream* pWriter);

private:
    void collectMetrics(const std::string& originalSeq, const std::string& correctedSeq, const std::string& qualityStr);
    std::ostream* m_pCorrectedWriter;
    std::ostream* m_pDiscardWriter;
    bool m_bCollectMetrics;
    ErrorCountMap<char> m_qualityMetrics;
    ErrorCountMap<int64_t> m_positionMetrics;
    ErrorCountMap<char> m_originalBaseMetrics;
    ErrorCountMap<std::string> m_precedingSeqMetrics;
    size_t m_totalBases = 0, m_totalErrors = 0, m_readsKept = 0, m_readsDiscarded = 0, m_kmerQCPassed = 0, m_overlapQCPassed = 0, m_qcFail = 0;
};

} // namespace stride
