// OverlapProcess.h -- the per-read work and the post-processing of `stride overlap`, batch at a time: the edges and vertex records
// of the reference's Concurrency/OverlapProcess.cpp:32-109 with Algorithm/OverlapBlock.cpp:128-160 (toOverlap) and SQG/ASQG.cpp
// (VertexRecord::write, EdgeRecord::write).  The overlap blocks of a batch are one lrsc_overlap_exact call; the -e, -a, -l and -f
// modes are not built.
//
// The reference's process() returns on a substring read before it clears its block list, so that read's blocks are written with
// the next read as their query.  Here a substring read writes no edges and leaves none behind.
#pragma once
#include <zlib.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/lrsc.h"
#include "SequenceWorkItem.h"

namespace stride {

struct OverlapParameters {
    lrsc_ctx* ctx = nullptr;                         // the index of the reads, on its device
    int minOverlap = 45;
    const std::vector<uint32_t>* order[2] = {nullptr, nullptr};   // .sai, .rsai: row of a '$' interval -> read
    const std::vector<std::string>* ids = nullptr;   // ReadInfoTable of the reads file: id and length of read i
    const std::vector<uint32_t>* lengths = nullptr;
};

struct OverlapResult {
    bool isSubstring = false;
};

class OverlapProcess {
public:
    OverlapProcess(const OverlapParameters& params, gzFile edges) : m_params(params), m_edges(edges) {}
    // overlapRead and the edges of every read of the batch, in order.  A read with a base other than A, C, G, T gets no edges (one
    // warning per run).  False, with a message, when a read's blocks outgrow the device workspace or the edges cannot be written.
    bool process_batch(const std::vector<SequenceWorkItem>& items, std::vector<OverlapResult>& results);

private:
    OverlapParameters m_params;
    gzFile m_edges;
    bool m_warnedOtherBases = false;
};

class OverlapPostProcess {               // OverlapAlgorithm::writeResultASQG: the VT record of a read
public:
    explicit OverlapPostProcess(gzFile asqg) : m_asqg(asqg) {}
    bool process(const SequenceWorkItem& item, const OverlapResult& result);

private:
    gzFile m_asqg;
};

// gzwrite of the whole string
bool gzPut(gzFile f, const std::string& s);

} // namespace stride
