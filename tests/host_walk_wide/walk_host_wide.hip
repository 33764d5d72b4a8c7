// walk_host_wide.hip -- TEST INFRASTRUCTURE ONLY (never linked into or loaded by the product).
//
// The serial wide walk, Walk<WIDE, true> of longreadselfcorrect_amd/csrc/walk_device.h (capacity from -l at run time, slot masks
// as bitsets), run on the CPU one walk at a time over the device's rank-block image and k-mer tables, so that `pytest -m "not gpu"`
// can hold -l above 32 against the CPU oracle without a device.  The index half is tests/host_walk's (included as is); this file
// adds hww_extend_walk.  wp_wide.hip's kernels run the same member functions with the frontier spread over a wavefront.
#include "../host_walk/walk_host.hip"
#include "../../longreadselfcorrect_amd/csrc/wp.h"

// mode 0: Walk::run (general step only); 1: the loop of the wide kernel (begin_static, begin_root, fast path with hand-over)
template <bool WIDE>
static int run_wide(HostIndex* ix, const HwParams& p, const uint8_t* codes, uint32_t initk, uint32_t path_len, uint32_t trg_len, int32_t dis,
                    uint32_t max_overlap, uint32_t min_sa, int mode, uint8_t* out, uint32_t out_cap, uint32_t* out_len, uint32_t* steps,
                    uint32_t* max_front)
{
    using P = typename Lay<WIDE>::pos_t;
    const uint32_t cap = (uint32_t)p.max_leaves;
    const uint32_t lq = initk + path_len + trg_len;
    const uint32_t seed = (uint32_t)p.idmer_len, mino = (uint32_t)p.min_kmer_len;
    const double maxLength = (1.2 * (dis + 10)) + (double)(2 * (uint64_t)initk);
    const uint32_t pathw = (uint32_t)(((uint64_t)maxLength + 4 + 15) / 16 + 1);
    const uint32_t n9 = lq - seed + 1, n5 = lq - 5 + 1, nT = trg_len - mino + 1;
    std::vector<SortItem> it9f(n9), it9r(n9);
    std::vector<P> term((size_t)nT * 4);
    std::vector<uint16_t> next9f(n9), next9r(n9), head9(512), head5(1024), next5(n5);
    std::vector<uint8_t> flags5(n5);
    // the wavefront workspace of wp_wide.hip (leaves, rings, results, paths) and the bitsets it keeps in LDS
    const WpWideLayout WL = wp_wide_layout((uint32_t)sizeof(Leaf<P>), pathw, cap);
    std::vector<uint64_t> wsv(WL.total / 8 + 1);
    uint8_t* ws = reinterpret_cast<uint8_t*>(wsv.data());
    std::vector<uint64_t> bits(5 * bits_words(cap) + bits_words(4 * cap));
    std::vector<uint32_t> outw(pathw);
    double freqs[101];
    for(int i = 0; i <= 100; ++i) freqs[i] = 0;
    for(int i = p.min_kmer_len; i <= 100; i++) freqs[i] = pow(1 - p.error_rate, i) * (size_t)p.pb_coverage;

    const FmIndexDev& fm = ix->dev;
    const StrandC<P> sf = strand_consts<P>(fm.strand[LRSC_RBWT]);
    const StrandC<P> sr = strand_consts<P>(fm.strand[LRSC_BWT]);
    uint32_t cr = 0, cb = 0;
    for(uint32_t i = 0; i < lq; ++i)
        prepare_offset<WIDE>(fm, sf, sr, ix->mtab.data(), codes, i, lq, initk + path_len, seed, mino, it9f.data(), it9r.data(), flags5.data(),
                             term.data(), cr, cb);

    Walk<WIDE, true> W;
    W.sF = sf; W.sR = sr; W.fm = &fm; W.mtab = ix->mtab.data();
    W.q = codes;
    W.Lq = lq; W.initk = initk; W.path_len = path_len; W.trg_len = trg_len; W.dis = dis;
    W.seedSize = seed; W.minOverlap = mino; W.maxOverlap = max_overlap; W.maxLeaves = cap;
    W.min_SA_threshold = min_sa;
    W.PBcoverage = (uint64_t)p.pb_coverage; W.PacBioErrorRate = p.error_rate; W.errorRate = 0.25; W.localK = 100;
    W.freqsOfKmerSize = freqs;
    W.set_lengths(dis, initk);
    W.it9f = it9f.data(); W.it9r = it9r.data();
    W.next9f = next9f.data(); W.next9r = next9r.data();
    W.head9f = head9.data(); W.head9r = head9.data() + 256;
    W.head5 = head5.data(); W.next5 = next5.data(); W.flags5 = flags5.data();
    W.term = term.data();
    W.n_term = trg_len >= mino ? trg_len - mino + 1 : 0;
    W.cap = cap; W.cap_children = 4 * cap; W.cap_results = wide_results(cap);
    const uint32_t bw = bits_words(cap);
    W.ring_bits = bits.data(); W.path_bits = W.ring_bits + bw; W.child_bits = W.path_bits + bw; W.seen_bits = W.child_bits + bw;
    W.alive_bits = W.seen_bits + bw;
    W.leaf_small = reinterpret_cast<Leaf<P>*>(ws + WL.leaves);
    W.cur = W.leaf_small; W.nxt = W.leaf_small + cap;
    W.rings = reinterpret_cast<double*>(ws + WL.rings);
    W.results = reinterpret_cast<WalkResultRec*>(ws + WL.results);
    W.paths = reinterpret_cast<uint32_t*>(ws + WL.paths); W.pathw = pathw; W.rpaths = W.paths + (uint64_t)cap * pathw;
    W.n_rank = 0; W.n_blk = 0; W.steps = 0; W.leaf_steps = 0; W.max_front = 1; W.error = 0; W.cyc_setup = 0; W.cyc_loop = 0; W.prof = nullptr;
    W.profile = false;

    uint32_t len = 0, mi = 0;
    int code;
    if(mode == 0) code = W.run(&len, outw.data(), &mi);
    else {
        W.begin_static();
        W.begin_root(nullptr);
        Leaf<P> L;
        uint32_t pw = 0;
        bool fast = false;
        while(true) {
            if(!fast && W.can_fast()) { W.enter_fast(L, pw); fast = true; }
            int r = 2;
            if(fast) {
                r = W.step_fast(L, pw);
                if(r != 1) fast = false;
            }
            if(r == 2) r = W.step() ? 1 : 0;
            if(r != 1) break;
        }
        code = W.finish(&len, outw.data(), &mi);
    }
    *steps = (uint32_t)W.steps;
    *max_front = W.max_front;
    *out_len = 0;
    if(code > 0) {
        const uint32_t tail_from = mi + mino;
        const uint32_t tail = trg_len > mino && tail_from <= trg_len ? trg_len - tail_from : 0;
        if(len + tail > out_cap) return -1000;
        for(uint32_t i = 0; i < len; ++i) out[i] = (uint8_t)path_get(outw.data(), i);
        const uint8_t* trg = codes + initk + path_len;
        for(uint32_t i = 0; i < tail; ++i) out[len + i] = trg[tail_from + i];
        *out_len = len + tail;
    }
    return code;
}

// codes: beginning k-mer | raw read segment | target seed, as 0..3; p->max_leaves is the capacity (1..256)
extern "C" int hww_extend_walk(void* h, const HwParams* p, const uint8_t* codes, uint32_t initk, uint32_t path_len, uint32_t trg_len, int32_t dis,
                               uint32_t max_overlap, uint32_t min_sa, int mode, uint8_t* out, uint32_t out_cap, uint32_t* out_len, uint32_t* steps,
                               uint32_t* max_front)
{
    HostIndex* ix = static_cast<HostIndex*>(h);
    if(p->max_leaves < 1 || p->max_leaves > (int)kWideMaxLeaves) return -1001;
    return ix->wide ? run_wide<true>(ix, *p, codes, initk, path_len, trg_len, dis, max_overlap, min_sa, mode, out, out_cap, out_len, steps, max_front)
                    : run_wide<false>(ix, *p, codes, initk, path_len, trg_len, dis, max_overlap, min_sa, mode, out, out_cap, out_len, steps, max_front);
}
