// OverlapProcess.cpp -- see OverlapProcess.h (reference behaviour: Concurrency/OverlapProcess.cpp:32-109,
// Algorithm/OverlapBlock.cpp:128-160, Util/SeqCoord.h:40-48,99-107, SQG/ASQG.cpp:185-255).
#include "OverlapProcess.h"

#include <cstdlib>
#include <iostream>
#include <sstream>

namespace stride {

static bool onlyACGT(const std::string& s)
{
    for(size_t i = 0; i < s.size(); ++i)
        if(s[i] != 'A' && s[i] != 'C' && s[i] != 'G' && s[i] != 'T') return false;
    return true;
}

bool gzPut(gzFile f, const std::string& s)
{
    for(size_t at = 0; at < s.size();) {
        const size_t n = s.size() - at < (1u << 30) ? s.size() - at : (1u << 30);
        if(gzwrite(f, s.data() + at, (unsigned)n) != (int)n) return false;
        at += n;
    }
    return true;
}

bool OverlapProcess::process_batch(const std::vector<SequenceWorkItem>& items, std::vector<OverlapResult>& results)
{
    results.assign(items.size(), OverlapResult());
    std::string bases;
    std::vector<uint64_t> off(1, 0);
    std::vector<size_t> sent;                                     // the reads that go to the device
    for(size_t n = 0; n < items.size(); ++n) {
        const std::string& s = items[n].read.seq;
        if(s.empty()) continue;
        if(!onlyACGT(s)) {
            if(!m_warnedOtherBases) std::cerr << "Warning: read " << items[n].read.id << " holds a base other than A, C, G, T: such reads get no edges\n";
            m_warnedOtherBases = true;
            continue;
        }
        sent.push_back(n);
        bases += s;
        off.push_back(bases.size());
    }
    if(sent.empty()) return true;
    std::vector<lrsc_overlap_read> per_read(sent.size());
    std::vector<lrsc_overlap_block> blocks(4 * sent.size());
    uint64_t used = 0;
    int st = lrsc_overlap_exact(m_params.ctx, bases.data(), off.data(), (uint32_t)sent.size(), m_params.minOverlap, per_read.data(), blocks.data(), blocks.size(), &used);
    if(st == LRSC_ERR_CAPACITY) {                                 // the size that the call asked for
        blocks.resize(used);
        st = lrsc_overlap_exact(m_params.ctx, bases.data(), off.data(), (uint32_t)sent.size(), m_params.minOverlap, per_read.data(), blocks.data(), blocks.size(), &used);
    }
    if(st != LRSC_OK) {
        std::cerr << "lrsc_overlap_exact: " << lrsc_strerror(st) << " (" << lrsc_last_error() << ")\n";
        return false;
    }
    const std::vector<std::string>& ids = *m_params.ids;
    const std::vector<uint32_t>& lengths = *m_params.lengths;
    std::ostringstream edges;
    for(size_t q = 0; q < sent.size(); ++q) {
        const SequenceWorkItem& item = items[sent[q]];
        const lrsc_overlap_read& r = per_read[q];
        if(r.status != 0) {
            std::cerr << "overlap: the overlap blocks of read " << item.read.id << " outgrow the device's workspace\n";
            return false;
        }
        results[sent[q]].isSubstring = r.is_substring != 0;
        if(r.is_substring) continue;                              // "Give up substring overlap"
        const std::string& queryID = ids[item.idx];
        const int queryLen = (int)lengths[item.idx];
        for(uint64_t b = r.first_block; b < r.first_block + r.n_blocks; ++b) {
            const lrsc_overlap_block& blk = blocks[b];
            const std::vector<uint32_t>& sai = *m_params.order[blk.target_rev ? 1 : 0];
            for(int64_t j = blk.lower; j <= blk.upper; ++j) {
                if(j < 0 || (uint64_t)j >= sai.size() || sai[(size_t)j] >= ids.size()) {
                    std::cerr << "overlap: a block of read " << item.read.id << " lies outside the lexicographic index\n";
                    return false;
                }
                const uint32_t target = sai[(size_t)j];
                const std::string& targetID = ids[target];
                if(queryID == targetID) continue;
                // OverlapBlock::toOverlap: the coordinates are those of the reads as given, flipped where the search was reversed
                const int targetLen = (int)lengths[target], ol = (int)blk.overlap_len;
                int s1 = queryLen - ol, e1 = queryLen - 1, s2 = 0, e2 = ol - 1;
                if(blk.query_rev) { const int t = queryLen - s1 - 1; s1 = queryLen - e1 - 1; e1 = t; }
                if(blk.target_rev) { const int t = targetLen - s2 - 1; s2 = targetLen - e2 - 1; e2 = t; }
                const bool containment = (s1 == 0 && e1 + 1 == queryLen) || (s2 == 0 && e2 + 1 == targetLen);
                if(containment && blk.query_rev) continue;
                if(queryID < targetID) continue;                  // the canonical edge is written from the read with the greater name
                edges << "ED\t" << queryID << " " << targetID << " " << s1 << " " << e1 << " " << queryLen << " " << s2 << " " << e2 << " " << targetLen << " "
                      << (blk.target_rev != blk.query_rev ? 1 : 0) << " 0\n";
            }
        }
    }
    if(!gzPut(m_edges, edges.str())) {
        std::cerr << "overlap: could not write the edges\n";
        return false;
    }
    return true;
}

bool OverlapPostProcess::process(const SequenceWorkItem& item, const OverlapResult& result)
{
    return gzPut(m_asqg, "VT\t" + item.read.id + "\t" + item.read.seq + "\tSS:i:" + (result.isSubstring ? "1" : "0") + "\n");
}

} // namespace stride
