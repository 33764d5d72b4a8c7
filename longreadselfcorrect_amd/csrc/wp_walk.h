// wp_walk.h -- device glue between the walk-parallel flow's slots (wp.h) and the walk (walk_device.h), shared by the extension
// kernels of wp.hip and wp_wave.hip.  Include after walk_device.h and wp.h.
#pragma once

namespace lrsc {

// the walk's fixed inputs: the query and the tables wp_prepare_kernel / wp_begin_kernel built in the slot's prepared workspace
template <bool WIDE, bool BIG>
__device__ __forceinline__ void wp_bind_static(Walk<WIDE, BIG>& W, const WpArgs& a, const WpSlot& s)
{
    using P = typename Lay<WIDE>::pos_t;
    const WpPrepLayout L = wp_prep_layout(s.lq, s.trg_len, a.seed_size, a.min_overlap, a.psz);
    uint8_t* ws = s.prep;
    W.q = s.q;
    W.Lq = s.lq; W.initk = s.k; W.path_len = s.gap; W.trg_len = s.trg_len; W.dis = (int32_t)s.gap;
    W.it9f = reinterpret_cast<SortItem*>(ws + L.item9f);
    W.it9r = reinterpret_cast<SortItem*>(ws + L.item9r);
    W.next9f = reinterpret_cast<uint16_t*>(ws + L.next9f);
    W.next9r = reinterpret_cast<uint16_t*>(ws + L.next9r);
    W.head9f = reinterpret_cast<uint16_t*>(ws + L.head9);
    W.head9r = W.head9f + 256;
    W.head5 = reinterpret_cast<uint16_t*>(ws + L.head5);
    W.next5 = reinterpret_cast<uint16_t*>(ws + L.next5);
    W.flags5 = ws + L.flags5;
    W.term = reinterpret_cast<const P*>(ws + L.term);
    W.n_term = s.trg_len >= a.min_overlap ? s.trg_len - a.min_overlap + 1 : 0;
}

} // namespace lrsc
