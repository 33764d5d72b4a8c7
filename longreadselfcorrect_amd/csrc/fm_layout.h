// fm_layout.h -- host image of the FM-index in the HBM block layout (see fm_device.h).
#pragma once
#include <cstddef>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "fm_device.h"

namespace lrsc {

// Host memory at the rank blocks' own alignment: the image's bytes are read and written as Block32 / Block64 (alignas(64)).
template <class T>
struct BlockAligned {
    using value_type = T;
    BlockAligned() = default;
    template <class U> BlockAligned(const BlockAligned<U>&) {}
    T* allocate(std::size_t n) { return static_cast<T*>(::operator new(n * sizeof(T), std::align_val_t(alignof(Block32)))); }
    void deallocate(T* p, std::size_t) { ::operator delete(p, std::align_val_t(alignof(Block32))); }
    template <class U> bool operator==(const BlockAligned<U>&) const { return true; }
    template <class U> bool operator!=(const BlockAligned<U>&) const { return false; }
};
static_assert(alignof(Block32) == alignof(Block64), "one alignment for both layouts");

struct StrandImage {
    std::vector<uint8_t, BlockAligned<uint8_t>> blocks;   // n_blocks * 64 bytes (Block32 or Block64)
    std::vector<uint64_t> dollars;    // sorted positions of '$' rows
    std::vector<uint32_t> dollar_dir; // '$' rows before every group of 2^kDollarDirShift blocks (+ one terminal entry)
    uint64_t n_blocks = 0;
    uint64_t n_symbols = 0;
    uint64_t n_runs = 0;
    uint64_t pred[5] = {0, 0, 0, 0, 0};
};

// Parse the 30-byte header + RL units of a .bwt/.rbwt file
// (format: SuffixTools/BWTWriterBinary.cpp:28-46,82-93 / BWTReaderBinary.cpp:55-85).
// Returns an lrsc_status.
int read_bwt_file(const std::string& path, std::vector<uint8_t>& units, uint64_t& num_strings,
                  uint64_t& num_symbols, std::string& err);

// Re-encode RL units ((rank<<5)|len, rank in $ACGT = 0..4) into rank blocks.
// wide=false -> Block32 (requires num_symbols < 2^31), wide=true -> Block64.
int build_strand_image(const uint8_t* units, uint64_t n_units, uint64_t num_symbols, bool wide,
                       StrandImage& out, std::string& err);

} // namespace lrsc
