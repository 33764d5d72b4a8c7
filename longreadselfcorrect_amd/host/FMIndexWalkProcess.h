// FMIndexWalkProcess.h -- the per-read and per-pair work and the post-processing of `stride fmwalk`, batch at a time: same results,
// output and counters as the reference's FMIndexWalk/FMIndexWalkProcess.cpp:29-150 (MergeAndKmerize), 153-226 (MergePairedReads),
// 229-267 (KmerizeReads), 269-391 (ValidateReads) and 898-1020 (FMIndexWalkPostProcess on reads and on pairs).  The trim, the
// walks and the splits are lrsc_fmwalk_merge, lrsc_fmwalk_hybrid, lrsc_fmwalk_kmerize and lrsc_fmwalk_validate, one device call
// per batch.
#pragma once
#include <cstddef>
#include <iosfwd>
#include <string>
#include <vector>

#include "../../include/lrsc.h"
#include "SequenceWorkItem.h"

namespace stride {

enum FMIndexWalkAlgorithm { FMW_HYBRID, FMW_MERGE, FMW_KMERIZE, FMW_VALIDATE };

struct FMIndexWalkParameters {
    lrsc_ctx* ctx = nullptr;             // the index to walk, on its device
    FMIndexWalkAlgorithm algorithm = FMW_MERGE;
    int kmerLength = 31;
    int kmerThreshold = 3;               // CorrectionThresholds::setBaseMinSupport
    int maxLeaves = 32;
    int maxInsertSize = 400;
    int minOverlap = 81;
    int maxOverlap = -1;                 // -1: 0.9 (hybrid: 0.95) * the mean length of the pair's reads
    size_t repeatKmerFreq = 0;           // hybrid: kd.getQuartile(2) * 1.3, as isSuitableForFMWalk computes it
};

struct FMIndexWalkResult {
    std::string correctSequence, correctSequence2;
    std::vector<std::string> kmerizedReads, kmerizedReads2;
    bool merge = false, kmerize = false, kmerize2 = false;
};

class FMIndexWalkProcess {
public:
    explicit FMIndexWalkProcess(const FMIndexWalkParameters& params) : m_params(params) {}
    // MergePairedReads or, in hybrid mode, MergeAndKmerize for every pair of the batch, in order.  A pair with an empty read or
    // with a base other than A, C, G, T is neither merged nor kmerized (one warning per run for the latter); a read shorter than
    // the k-mer, on which the reference throws, counts as trimmed to nothing.
    std::vector<FMIndexWalkResult> process_batch(const std::vector<SequenceWorkItemPair>& pairs);
    // KmerizeReads or, in validate mode, ValidateReads for every read of the batch, in order; an empty read or one with another
    // base is neither kmerized nor merged.  In validate mode a read that lrsc_fmwalk_validate would refuse for its length ends the
    // run with one line that names it.
    std::vector<FMIndexWalkResult> process_batch(const std::vector<SequenceWorkItem>& reads);

private:
    FMIndexWalkParameters m_params;
    bool m_warnedOtherBases = false;
};

class FMIndexWalkPostProcess {           // the writers and the three counters
public:
    // pLowComplexWriter: the validate algorithm's LowComplexityReads.fa, the reads that are neither kmerized nor merged
    explicit FMIndexWalkPostProcess(std::ostream* pCorrectedWriter, std::ostream* pDiscardWriter = nullptr, FMIndexWalkAlgorithm algorithm = FMW_MERGE,
                                    std::ostream* pLowComplexWriter = nullptr)
        : m_pCorrectedWriter(pCorrectedWriter), m_pDiscardWriter(pDiscardWriter), m_pLowComplexWriter(pLowComplexWriter), m_algorithm(algorithm) {}
    ~FMIndexWalkPostProcess();           // prints the counters
    void process(const SequenceWorkItem& item, const FMIndexWalkResult& result);
    void process(const SequenceWorkItemPair& itemPair, const FMIndexWalkResult& result);

private:
    std::ostream* m_pCorrectedWriter;
    std::ostream* m_pDiscardWriter;
    std::ostream* m_pLowComplexWriter;
    FMIndexWalkAlgorithm m_algorithm;
    size_t m_kmerizePassed = 0, m_mergePassed = 0, m_qcFail = 0;
};

} // namespace stride
