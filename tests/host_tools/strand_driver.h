// strand_driver.h -- what the drivers that run an index tool's per-lane code on the CPU share: how they end, how they read their
// input and how they come by a strand as the kernels see it.  A driver says `static const char kDriver[] = "its name";` before
// it includes this.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../longreadselfcorrect_amd/csrc/fm_layout.h"
#include "../../longreadselfcorrect_amd/csrc/fm_strand.h"

inline void die(const char* what)
{
    std::fprintf(stderr, "%s: %s\n", kDriver, what);
    std::exit(1);
}

inline void read_exact(void* p, size_t n)
{
    if(n && std::fread(p, 1, n, stdin) != n) die("short input");
}

// u64 N, u64 n_units, the RL units of a strand's BWT -> its image from build_strand_image (fm_layout.cpp), Block64 where wide,
// as lrsc_index_upload would hold it
inline void read_image(bool wide, lrsc::StrandImage& im)
{
    uint64_t hdr[2];
    read_exact(hdr, 16);
    std::vector<uint8_t> units(hdr[1]);
    read_exact(units.data(), units.size());
    std::string err;
    if(lrsc::build_strand_image(units.data(), units.size(), hdr[0], wide, im, err) != 0) die(err.c_str());
}

inline lrsc::FmStrand strand_of(const lrsc::StrandImage& im, bool wide)
{
    lrsc::FmStrand fs;
    fs.blocks = im.blocks.data();
    fs.dollars = im.dollars.data();
    fs.dollar_dir = im.dollar_dir.data();
    fs.dollar_group_syms = (uint64_t)(wide ? lrsc::Block64::kSyms : lrsc::Block32::kSyms) << lrsc::kDollarDirShift;
    fs.n_dollars = im.dollars.size();
    fs.n_symbols = im.n_symbols;
    fs.n_blocks = im.n_blocks;
    for(int c = 0; c < 5; ++c) fs.pred[c] = im.pred[c];
    return fs;
}

// the layout's mask table, as a workgroup fills it in LDS
template <class Block>
std::vector<uint32_t> mask_table()
{
    std::vector<uint32_t> t(lrsc::MaskTab<Block>::kWords);
    for(uint32_t i = 0; i < t.size(); ++i) t[i] = lrsc::mask_word<Block>(i);
    return t;
}
