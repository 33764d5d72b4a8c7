// fm_locate.h -- which read and offset a BWT row belongs to: the per-lane arithmetic of the device locate (fm_locate.hip), the
// reference's SampledSuffixArray (SuffixTools/SampledSuffixArray.cpp:44-190) on the rank-block layout.
//
// A strand of an index is the BWT of a string set whose sentinels sort in input order: row i < n is the suffix that is read
// i's sentinel alone.  One LF step, i <- C[c] + Occ(c, i) with c = BWT[i], leads from the suffix of a read at position p to
// the one at p - 1, and the row whose symbol is '$' is the whole read.  Both c and Occ(c, i) come from the one rank block of
// row i (fm_strand.h's lf_step).
//
//   prepare  One lane per read i walks it backwards from row i, counting its steps t.  Every visited row r that is a multiple
//            of the sample rate gets samples[r / rate] = (i, t).  At the '$' row, whose rank among the '$' rows is k (the
//            directory entry of the row's group plus the scan of the list up to the row), order[k] = i and read_len[i] = t.
//            The walks of all reads visit every row of the strand once: no atomics.
//   fix-up   samples[s] = (read, read_len[read] - t): SA[r] as SampledSuffixArray::build stores it, position len at the
//            sentinel row, counting down to 0 at the '$' row.
//   locate   calcSA: while the row is no multiple of the rate (always, at rate 0) one LF step and offset + 1; on a sampled row
//            the answer is (sample.read, sample.pos + offset), on a '$' row (order[k], offset).  The sample is looked at before
//            the symbol, as in the reference.
//
// Every walk ends on any input: after num_symbols steps, or when a position leaves the index, the lane reports kWalkBroken
// and the call fails.  All functions here are LRSC_HD and free of HIP types: the kernels call them, and
// tests/host_tools/locate_driver.cpp compiles the same source for the CPU and holds it against a suffix sort.
#pragma once
#include <stdint.h>

#include <string>

#include "fm_strand.h"

namespace lrsc {

constexpr uint32_t kLocateThreads = 128;                          // lanes, one read (prepare) or one row (locate) each, per workgroup
// Wavefronts per SIMD that both launches are sized for: a walk is a chain of dependent 64-byte loads and latency-bound, so the
// kernels have to stay within 512 / kLocateWavesPerSimd VGPRs.
constexpr uint32_t kLocateWavesPerSimd = 8;
constexpr uint32_t kLocateUnset = 0xFFFFFFFFu;                    // an entry no walk has written (the tables start as 0xFF bytes)

struct SaElem { uint32_t read, pos; };                            // lrsc_sa_elem: SA[row] = the suffix of `read` that starts at `pos`

// the locate tables of one strand, on the device
struct LocateTables {
    SaElem* samples = nullptr;                                    // n_samples entries: SA of the rows that are multiples of rate
    uint32_t* order = nullptr;                                    // n_reads: k-th '$' row -> read (the .sai / .rsai content)
    uint32_t* read_len = nullptr;                                 // n_reads
    uint64_t n_samples = 0;                                       // rate > 0: num_symbols / rate + 1, else 0
    uint32_t rate = 0;
};
LRSC_HD uint64_t locate_sample_count(uint64_t n_symbols, uint32_t rate) { return rate ? n_symbols / rate + 1 : 0; }

// ---- prepare: the walk of one read ----
// Returns kWalkOk after writing the read's samples, order[] entry and length.  n_reads = S.n_dollars.
template <class Block>
LRSC_HD uint32_t locate_prepare_read(const StrandView<Block>& S, const uint32_t* mtab, uint32_t read, uint32_t rate, SaElem* samples,
                                     uint32_t* order, uint32_t* read_len)
{
    uint64_t k = 0, t = 0;
    const uint32_t st = walk_read_back(S, mtab, read, [&](typename BlockLay<Block>::pos_t i, uint64_t steps) {
        if(rate != 0 && i % rate == 0) samples[i / rate] = SaElem{read, (uint32_t)steps};
    }, k, t);
    if(st != kWalkOk) return st;
    order[k] = read;
    read_len[read] = (uint32_t)t;
    return kWalkOk;
}

// ---- fix-up: steps from the sentinel row -> position in the read ----
// slot = the sample's index: the last slot is for row num_symbols when that is a multiple of the rate, a row that does not
// exist, and stays unset (the reference's empty SAElem)
LRSC_HD uint32_t locate_fix_sample(SaElem& s, uint64_t slot, uint32_t rate, uint64_t n_symbols, const uint32_t* read_len, uint64_t n_reads)
{
    if(slot * rate >= n_symbols) return kWalkOk;
    if(s.read == kLocateUnset || s.read >= n_reads) return kWalkBroken;     // a row that no walk came through
    const uint32_t len = read_len[s.read];
    if(s.pos > len) return kWalkBroken;
    s.pos = len - s.pos;
    return kWalkOk;
}

// ---- locate: calcSA of one row ----
// steps += the LF steps taken
template <class Block>
LRSC_HD uint32_t locate_row(const StrandView<Block>& S, const uint32_t* mtab, uint64_t row, uint32_t rate, const SaElem* samples,
                            const uint32_t* order, SaElem& out, uint32_t& steps)
{
    using P = typename BlockLay<Block>::pos_t;
    out = SaElem{kLocateUnset, kLocateUnset};
    if(row >= S.N) return kWalkBroken;
    P i = (P)row;
    for(uint64_t offset = 0; offset < S.N; ++offset) {
        if(i >= S.N) return kWalkBroken;
        if(rate != 0 && i % rate == 0) {
            const SaElem s = samples[i / rate];
            out = SaElem{s.read, s.pos + (uint32_t)offset};
            return kWalkOk;
        }
        const Block b = S.blocks[block_of<Block>(i)];
        uint64_t k = 0;
        if(!lf_step(S, b, mtab, i, k)) {
            out = SaElem{order[k], (uint32_t)offset};
            return kWalkOk;
        }
        ++steps;
    }
    return kWalkBroken;
}

// ---- the device side (fm_locate.hip) ----
// Builds the tables of one strand, a copy on the current device, at `rate` (0: order and lengths only).  On an error nothing
// stays allocated.  LRSC_ERR_FORMAT when a walk does not end or the walks do not cover the strand.
int locate_prepare_device(const FmStrand& s, bool wide, uint32_t rate, LocateTables& out, std::string& err);
void locate_free_device(LocateTables& t);

} // namespace lrsc
