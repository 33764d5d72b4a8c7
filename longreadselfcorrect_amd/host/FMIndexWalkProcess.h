// FMIndexWalkProcess.h -- the per-pair work and the post-processing of `stride fmwalk -a merge`, batch at a time: same results,
// output and counters as the reference's FMIndexWalk/FMIndexWalkProcess.cpp:153-226 (MergePairedReads) and 898-920, 972-1020
// (FMIndexWalkPostProcess on pairs).  The trim and the walks are lrsc_fmwalk_merge, one device call per batch; the kmerize,
// validate and hybrid algorithms are not built.
#pragma once
#include <cstddef>
#include <iosfwd>
#include <string>
#include <vector>

#include "../../include/lrsc.h"
#include "SequenceWorkItem.h"

namespace stride {

struct FMIndexWalkParameters {
    lrsc_ctx* ctx = nullptr;             // the index to walk, on its device
    int kmerLength = 31;
    int kmerThreshold = 3;               // CorrectionThresholds::setBaseMinSupport
    int maxLeaves = 32;
    int maxInsertSize = 400;
    int minOverlap = 81;
    int maxOverlap = -1;                 // -1: 0.9 * the mean length of the pair's reads
};

struct FMIndexWalkResult {
    std::string correctSequence;
    bool merge = false;
};

class FMIndexWalkProcess {
public:
    explicit FMIndexWalkProcess(const FMIndexWalkParameters& params) : m_params(params) {}
    // MergePairedReads for every pair of the batch, in order.  A pair with an empty read or with a base other than A, C, G, T is
    // not merged (one warning per run for the latter); nor is one with a read shorter than the k-mer, on which the reference throws.
    std::vector<FMIndexWalkResult> process_batch(const std::vector<SequenceWorkItemPair>& pairs);

private:
    FMIndexWalkParameters m_params;
    bool m_warnedOtherBases = false;
};

class FMIndexWalkPostProcess {           // the merged reads' writer and the three counters
public:
    explicit FMIndexWalkPostProcess(std::ostream* pCorrectedWriter) : m_pCorrectedWriter(pCorrectedWriter) {}
    ~FMIndexWalkPostProcess();           // prints the counters
    void process(const SequenceWorkItemPair& itemPair, const FMIndexWalkResult& result);

private:
    std::ostream* m_pCorrectedWriter;
    size_t m_kmerizePassed = 0, m_mergePassed = 0, m_qcFail = 0;
};

} // namespace stride
