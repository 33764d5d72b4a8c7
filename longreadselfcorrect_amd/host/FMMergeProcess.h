// FMMergeProcess.h -- the work and the post-processing of `stride fm-merge`: the reference's Algorithm/FMMergeProcess.cpp:30-230
// (FMMergeProcess::process over every read of the file) and 313-329 (FMMergePostProcess), with all reads in one lrsc_fmmerge call:
// the step is global, a chain of reads may run through the whole file.
//
// The reference takes the strand of a merged sequence and the place where it cuts a cycle from the iteration order of a hash map.
// Here a sequence reads on the forward strand of its lowest-numbered read, a cycle starts with that read, and the sequences come in
// the order of their lowest-numbered used read (include/lrsc.h).
#pragma once
#include <cstddef>
#include <cstdint>
#include <iosfwd>
#include <string>
#include <vector>

#include "../../include/lrsc.h"

namespace stride {

struct FMMergeResult {
    std::vector<lrsc_fmmerge_read> reads;            // every read's place
    std::vector<lrsc_fmmerge_seq> seqs;              // merged-0, merged-1, ...
    std::string bases;                               // the sequences back to back
};

class FMMergeProcess {
public:
    FMMergeProcess(lrsc_ctx* ctx, int minOverlap) : m_ctx(ctx), m_minOverlap(minOverlap) {}
    // Every read of the file (bases back to back, n + 1 offsets) merged.  False, with the library's message on stderr, when the
    // call is refused: the index is not that of these reads, or `stride filter` has not been run on them.
    bool process(const std::string& bases, const std::vector<uint64_t>& off, FMMergeResult& result);

private:
    lrsc_ctx* m_ctx;
    int m_minOverlap;
};

class FMMergePostProcess {
public:
    explicit FMMergePostProcess(std::ostream* writer) : m_writer(writer) {}
    ~FMMergePostProcess();                           // the three summary lines
    // the records of all sequences, named merged-i; numTotal = the reads they were made of
    bool process(const FMMergeResult& result);

private:
    std::ostream* m_writer;
    size_t m_numMerged = 0, m_numTotal = 0, m_totalLength = 0;
};

} // namespace stride
