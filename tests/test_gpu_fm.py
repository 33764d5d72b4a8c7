"""GPU parity of the FM primitives: HIP kernels (through the C ABI) vs the CPU oracle, bit-exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def gpu_ctx(api, small_ds):
    idx = api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")
    idx.upload(0)
    ctx = idx.ctx(api.params_default(5, 90), 0)
    yield ctx
    ctx.close()
    idx.close()


def test_index_info(api, gpu_ctx, oracle, small_ds):
    info = gpu_ctx.index.info()
    for s, ext in enumerate(["bwt", "rbwt"]):
        ob = oracle.bwt_load(f"{small_ds.prefix}.{ext}")
        assert info.num_strings == ob.num_strings and info.num_symbols == ob.num_symbols
        assert info.num_runs[s] == ob.num_runs
        for c, ch in enumerate("$ACGT"):
            assert info.pred_count[s][c] == ob.pc(ch)
        ob.close()
    assert info.block_bytes == 64 and info.block_symbols in (128, 192)


@pytest.mark.parametrize("strand,ext", [(0, "bwt"), (1, "rbwt")])
def test_rank_matches_oracle(gpu_ctx, oracle, small_ds, strand, ext):
    ob = oracle.bwt_load(f"{small_ds.prefix}.{ext}")
    n = ob.num_symbols
    rng = np.random.default_rng(11 + strand)
    edge = np.array([-1, 0, 1, 127, 128, 129, 191, 192, 193, 383, 384, n - 2, n - 1], dtype=np.int64)
    idx = np.concatenate([edge, rng.integers(-1, n, size=300_000)])
    # every block boundary region once as well
    idx = np.concatenate([idx, np.arange(-1, min(n, 4096), dtype=np.int64)])
    bases = rng.choice(ACGT, size=idx.size)
    got = gpu_ctx.rank(bases, idx, strand)
    np.testing.assert_array_equal(got, ob.occ(bases, idx))
    ob.close()


@pytest.mark.parametrize("strand,ext", [(0, "bwt"), (1, "rbwt")])
def test_bwt_chars_match_oracle(gpu_ctx, oracle, small_ds, strand, ext):
    ob = oracle.bwt_load(f"{small_ds.prefix}.{ext}")
    n = ob.num_symbols
    pos = np.arange(0, n, dtype=np.uint64)          # the whole BWT, '$' rows included
    got = gpu_ctx.bwt_chars(strand, pos)
    np.testing.assert_array_equal(got, ob.decode())
    assert (got == ord("$")).sum() == ob.num_strings
    ob.close()


@pytest.mark.parametrize("k", [1, 5, 9, 13, 19, 31])
def test_find_kmers_matches_oracle(gpu_ctx, oracle, small_ds, k):
    """findBiInterval: fwd in the rbwt with reverse(w), rvc in the bwt with revcomp(w) (BWTAlgorithms.cpp:32-38)."""
    rng = np.random.default_rng(100 + k)
    bases, off = small_ds.bases, small_ds.off
    # half real k-mers from the reads (present), half random (mostly absent for large k -> early exit path)
    starts = rng.integers(0, bases.size - k, size=4000)
    real = np.stack([bases[s:s + k] for s in starts if not np.any((off > s) & (off < s + k))])
    rand = rng.choice(ACGT, size=(4000, k))
    kmers = np.concatenate([real, rand]).astype(np.uint8)
    got = gpu_ctx.find_kmers(kmers.reshape(-1), k)

    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    ob, orb = oracle.bwt_load(small_ds.prefix + ".bwt"), oracle.bwt_load(small_ds.prefix + ".rbwt")
    fwd = orb.find_intervals(kmers[:, ::-1].copy().reshape(-1), k)          # reverse(w) in the rbwt
    rvc = ob.find_intervals(comp[kmers[:, ::-1]].copy().reshape(-1), k)     # revcomp(w) in the bwt
    np.testing.assert_array_equal(got["fwd_lower"], fwd[:, 0])
    np.testing.assert_array_equal(got["fwd_upper"], fwd[:, 1])
    np.testing.assert_array_equal(got["rvc_lower"], rvc[:, 0])
    np.testing.assert_array_equal(got["rvc_upper"], rvc[:, 1])
    if k >= 13:
        assert (fwd[len(real):, 0] > fwd[len(real):, 1]).any()      # the invalid/early-exit path was exercised
    ob.close(); orb.close()


def _grid_case(gpu_ctx, oracle, small_ds, bases, off, ks):
    ob, orb = oracle.bwt_load(small_ds.prefix + ".bwt"), oracle.bwt_load(small_ds.prefix + ".rbwt")
    want_iv, want_size, want_cnt = oracle.kmer_grid(ob, orb, bases, off, ks)
    got_iv, got_size, got_cnt = gpu_ctx.kmer_grid(bases, off, ks)
    for f in ("fwd_lower", "fwd_upper", "rvc_lower", "rvc_upper"):
        np.testing.assert_array_equal(got_iv[f], want_iv[f], err_msg=f)
    np.testing.assert_array_equal(got_size, want_size)
    np.testing.assert_array_equal(got_cnt, want_cnt)
    ob.close(); orb.close()
    return want_iv


@pytest.mark.parametrize("ks", [[5, 9, 15, 17, 19], [5, 9, 15, 19, 23], [5, 9, 19, 21, 25], [3, 4, 40]])
def test_kmer_grid_matches_oracle_on_real_reads(gpu_ctx, oracle, small_ds, ks):
    """LongReadProbe's per-position KmerFeature grid (LongReadProbe.cpp:146-150): intervals, sizes
    (incl. 'fake' k-mers at the read end) and composition counters, every record bit-exact."""
    n = 6
    off = small_ds.off[: n + 1].copy()
    bases = small_ds.bases[: int(off[-1])]
    _grid_case(gpu_ctx, oracle, small_ds, bases, off, np.array(ks, dtype=np.uint8))


def test_kmer_grid_edge_cases(gpu_ctx, oracle, small_ds):
    """Ragged batch: empty reads, reads shorter than every k, a read absent from the index (findInterval's
    early exit, then expand() on invalid intervals), homopolymers, and a read ending exactly at k."""
    from oracle.oracle_py import pack_reads

    rng = np.random.default_rng(5)
    foreign = "".join(rng.choice(list("ACGT"), size=400))         # random: k-mers >= ~11 are absent
    real = small_ds.reads[3]
    reads = ["", "A", "ACG", real[:5], real[10:28], real[:19], real[:20], "", foreign, "A" * 60, "ACAC" * 15,
             real[100:400], "T", ""]
    bases, off = pack_reads(reads)
    ks = np.array([5, 9, 15, 17, 19], dtype=np.uint8)
    want = _grid_case(gpu_ctx, oracle, small_ds, bases, off, ks)
    # the foreign read really exercised invalid intervals in the large slots
    s, e = int(off[8]), int(off[9])
    assert (want["fwd_lower"][s:e, 4] > want["fwd_upper"][s:e, 4]).mean() > 0.9


def test_non_acgt_is_rejected(gpu_ctx):
    from longreadselfcorrect_amd import LrscError

    bases = np.frombuffer(b"ACGTNACGT", dtype=np.uint8)
    off = np.array([0, 9], dtype=np.uint64)
    with pytest.raises(LrscError) as ei:
        gpu_ctx.kmer_grid(bases, off, np.array([5], dtype=np.uint8))
    assert ei.value.status == -3      # LRSC_ERR_ARG, mirrors SeqReader's exit on non-ACGT (Util/SeqReader.cpp:115-126)


def test_stats_count_block_loads(gpu_ctx, small_ds):
    from longreadselfcorrect_amd.capi import K_GRID

    gpu_ctx.stats_reset()
    off = small_ds.off[:3].copy()
    bases = small_ds.bases[: int(off[-1])]
    ks = np.array([5, 9, 15, 17, 19], dtype=np.uint8)
    gpu_ctx.kmer_grid(bases, off, ks, want_iv=False, want_count=False)
    st = gpu_ctx.stats(K_GRID)
    total = int(off[-1])
    # 74 Occ per interior position for pool {5,9,15,17,19}: 2 + 4*18
    assert st.launches == 1 and st.total_ms > 0
    assert 0.97 * 74 * total <= st.rank_queries <= 74 * total
    assert (st.rank_queries - 2 * total) // 2 <= st.block_loads <= st.rank_queries


# ---- LongReadProbe seeds --------------------------------------------------------------------------
def _seed_case(api, gpu_index, oracle, small_ds, params, bases, off):
    ctx = gpu_index.ctx(params, 0)
    b = ctx.batch(bases, off)
    b.find_seeds()
    count, seeds, attr = b.seeds()
    b.close(); ctx.close()
    ob, orb = oracle.bwt_load(small_ds.prefix + ".bwt"), oracle.bwt_load(small_ds.prefix + ".rbwt")
    wcount, wseeds, wattr = oracle.find_seeds(ob, orb, params, bases, off)
    ob.close(); orb.close()
    np.testing.assert_array_equal(attr, wattr)
    np.testing.assert_array_equal(count, wcount)
    got = np.stack([seeds[f] for f in seeds.dtype.names], axis=1)
    np.testing.assert_array_equal(got, wseeds)
    return wcount, wseeds, wattr


@pytest.fixture(scope="module", params=["default", "11", "0"], ids=["ktab-default", "ktab-11", "ktab-off"])
def gpu_index(request, api, small_ds):
    """The same index with the k-mer interval tables at their default size, forced to T = 11, and disabled:
    every parity test below runs against all three (results must not depend on the tables)."""
    import os

    old = os.environ.get("LRSC_KTAB_K")
    if request.param != "default":
        os.environ["LRSC_KTAB_K"] = request.param
    idx = api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")
    idx.upload(0)
    if old is None:
        os.environ.pop("LRSC_KTAB_K", None)
    else:
        os.environ["LRSC_KTAB_K"] = old
    yield idx
    idx.close()


@pytest.mark.parametrize("genome,cov", [(5, 90), (10, 90), (100, 90), (5, 60), (10, 30)])
def test_seeds_match_oracle(api, gpu_index, oracle, small_ds, genome, cov):
    """searchSeedsWithHybridKmers + estimateBestKmerSize + removeHitchhikingSeeds, every field bit-exact,
    plus getSeqAttribute per base, over the whole small read set."""
    p = api.params_default(genome, cov)
    wcount, wseeds, _ = _seed_case(api, gpu_index, oracle, small_ds, p, small_ds.bases, small_ds.off)
    if (genome, cov) == (5, 90):
        assert wcount.sum() > 3 * small_ds.n_reads            # the regime the bench uses really finds seeds


def test_seeds_edge_cases(api, gpu_index, oracle, small_ds):
    """Reads shorter than k, reads absent from the index (zero-frequency scan k-mers drive box[-1] negative:
    LongReadProbe.cpp:152-156 vs :163-168), homopolymers / low complexity, a repeat-rich chimera."""
    from oracle.oracle_py import pack_reads

    rng = np.random.default_rng(17)
    real = small_ds.reads
    foreign = "".join(rng.choice(list("ACGT"), size=900))
    chimera = real[2][:400] + foreign[:300] + real[5][200:700] + "A" * 40 + real[7][:300]
    reads = ["ACGT", real[0][:16], real[0][:17], real[0][:19], real[1][:60], foreign, chimera, "A" * 300, "AC" * 200,
             real[3], real[4][100:101], real[6][:500] + real[6][:500]]
    bases, off = pack_reads(reads)
    for g in (5, 10):
        p = api.params_default(g, 90)
        _seed_case(api, gpu_index, oracle, small_ds, p, bases, off)


def test_seeds_manual_mode(api, gpu_index, oracle, small_ds):
    p = api.params_default(5, 90)
    p.manual, p.mode = 1, 2
    n = 30
    off = small_ds.off[: n + 1].copy()
    _seed_case(api, gpu_index, oracle, small_ds, p, small_ds.bases[: int(off[-1])], off)


# ---- seed-to-seed FM-extend -------------------------------------------------------------------------
_COMP = str.maketrans("ACGT", "TGCA")


def _revcomp(s):
    return s.translate(_COMP)[::-1]


def _walk_descs(params, reads, count, seeds, max_per_read=1000):
    """The descriptors correctByFMExtension builds (PacBioSelfCorrectionProcess.cpp:159-190) for consecutive seed
    pairs, taking every source seed as found (no accumulated state) -- arbitrary but realistic walk inputs."""
    descs = []
    k = 0
    for r, n in enumerate(count):
        ss = seeds[k: k + n]
        k += n
        read = reads[r]
        for i in range(min(max(int(n) - 1, 0), max_per_read)):
            s, t = ss[i], ss[i + 1]
            s_start, s_len, t_start, t_len = int(s[0]), int(s[1]), int(t[0]), int(t[1])
            s_end = s_start + s_len - 1
            interval = t_start - s_end - 1
            ext = min(int(s[5]), int(t[4])) - 2                      # min(source.endBest, target.startBest) - 2
            if s[3] or t[3]:
                ext = min(min(s_len, t_len), params.start_kmer_len + 2)
            src = read[s_start: s_start + s_len][s_len - ext:]
            trg = read[t_start: t_start + t_len]
            path = read[s_end + 1: s_end + 1 + interval]
            min_sa = (params.pb_coverage // 60) * 3 if params.pb_coverage > 60 else 3
            if s[3] and not t[3]:                                     # isFromRtoU: walk from the unique side
                src, trg = _revcomp(trg), _revcomp(src)
                path = _revcomp(path)
            descs.append((src, path, trg, interval, ext, ext + 2, min_sa))
    return descs


@pytest.mark.parametrize("genome,cov", [(5, 90), (10, 90)])
def test_extend_walks_match_oracle(api, gpu_index, oracle, small_ds, genome, cov):
    """LongReadSelfCorrectByOverlap::extendOverlap: return code and merged sequence identical for every walk."""
    p = api.params_default(genome, cov)
    ob, orb = oracle.bwt_load(small_ds.prefix + ".bwt"), oracle.bwt_load(small_ds.prefix + ".rbwt")
    n_reads = 40
    off = small_ds.off[: n_reads + 1].copy()
    bases = small_ds.bases[: int(off[-1])]
    count, seeds, _ = oracle.find_seeds(ob, orb, p, bases, off)
    descs = _walk_descs(p, small_ds.reads[:n_reads], count, seeds)
    assert len(descs) > 100
    ctx = gpu_index.ctx(p, 0)
    got = ctx.extend_walks(descs)
    ctx.close()
    codes = {}
    for d, (code, merged, steps) in zip(descs, got):
        wcode, wmerged, wst = oracle.extend_walk(ob, orb, p, *d)
        assert (code, merged) == (wcode, wmerged), d
        assert steps == wst[0]
        codes[wcode] = codes.get(wcode, 0) + 1
    ob.close(); orb.close()
    assert codes.get(1, 0) > len(descs) // 2          # most walks succeed ...
    if (genome, cov) == (5, 90):
        assert codes.get(-1, 0) > 0                    # ... and the failure path is exercised too


# ---- the whole per-read path (--nodp) ---------------------------------------------------------------------
def _fasta(results, pieces, reads, split):
    correct, discard = [], []
    for r, (res, ps) in enumerate(zip(results, pieces)):
        if res.merge:
            for i, p in enumerate(ps):
                correct.append(f">r{r}{'_' + str(i) if split else ''}\n{p}\n")
        else:
            discard.append(f">r{r}\n{reads[r]}\n")
    return "".join(correct), "".join(discard)


@pytest.fixture(params=["device", "rounds"])
def correct_mode(request, monkeypatch):
    """device = the persistent per-read kernel (default); rounds = per-walk launches stitched on the host."""
    if request.param == "rounds":
        monkeypatch.setenv("LRSC_CORRECT_MODE", "rounds")
    else:
        monkeypatch.delenv("LRSC_CORRECT_MODE", raising=False)
    return request.param


def _check_whole_path(api, index, oracle, ds, p, n_reads=None, min_fm=500, min_dp=0, want=None, fail_cols=(4, 5)):
    """`want`: the oracle's run on these reads with these params where the caller keeps one (correct_fa, discard_fa, counters);
    computed here otherwise.  `fail_cols`: the counters that hold this setting's failed walks."""
    off = ds.off if n_reads is None else ds.off[: n_reads + 1].copy()
    bases = ds.bases[: int(off[-1])]
    reads = ds.reads[: len(off) - 1]
    own = want is None
    if own:
        ob, orb = oracle.bwt_load(ds.prefix + ".bwt"), oracle.bwt_load(ds.prefix + ".rbwt")
        want = oracle.correct_reads(ob, orb, p, bases, off)
    ctx = index.ctx(p, 0)
    results, pieces = ctx.correct_reads(bases, off)
    ctx.close()
    cfa, dfa = _fasta(results, pieces, reads, p.split)
    assert cfa == want.correct_fa
    assert dfa == want.discard_fa
    names = ("total_reads_len", "corrected_len", "total_seed_num", "total_walk_num", "high_error_num", "exceed_depth_num",
             "exceed_leave_num", "fm_num", "dp_num", "seed_dis", "merge")
    got = np.array([[getattr(r, n) for n in names] for r in results], dtype=np.int64)
    np.testing.assert_array_equal(got, want.counters)
    assert got[:, 7].sum() > min_fm and got[:, list(fail_cols)].sum() > 0      # many FM walks, some failures
    assert got[:, 8].sum() >= min_dp
    if own:
        want.close(); ob.close(); orb.close()
    return got


@pytest.mark.parametrize("genome,cov,split,next_target", [(5, 90, 0, 1), (5, 90, 1, 1), (10, 90, 0, 1), (5, 90, 0, 2)])
def test_whole_path_with_dp_fallback_matches_oracle_fasta(api, gpu_index, oracle, small_ds, genome, cov, split, next_target):
    """The DEFAULT pbcorrect flow (no --nodp): walks the FM-extension gives up on go through correctByMSAlignment
    (LF-walk retrieval, banded DP, multiple alignment, consensus -- all on the device); correct.fa / discard.fa and all
    counters incl. DPNum bit-identical to the oracle."""
    p = api.params_default(genome, cov)
    p.no_dp, p.split, p.next_target = 0, split, next_target
    _check_whole_path(api, gpu_index, oracle, small_ds, p, min_fm=300, min_dp=20)


@pytest.mark.parametrize("genome,cov,split,next_target", [(5, 90, 0, 1), (5, 90, 1, 1), (10, 90, 0, 1), (5, 90, 0, 3), (5, 90, 1, 2)])
def test_whole_path_nodp_matches_oracle_fasta(api, gpu_index, oracle, small_ds, genome, cov, split, next_target, correct_mode):
    """correct.fa / discard.fa and every integer counter of PacBioSelfCorrectionResult, bit-identical to the
    CPU oracle (--nodp: failed walks copy the raw segment, PacBioSelfCorrectionProcess.cpp:146-147)."""
    p = api.params_default(genome, cov)
    p.no_dp, p.split, p.next_target = 1, split, next_target
    ob, orb = oracle.bwt_load(small_ds.prefix + ".bwt"), oracle.bwt_load(small_ds.prefix + ".rbwt")
    want = oracle.correct_reads(ob, orb, p, small_ds.bases, small_ds.off)
    ctx = gpu_index.ctx(p, 0)
    results, pieces = ctx.correct_reads(small_ds.bases, small_ds.off)
    ctx.close()
    cfa, dfa = _fasta(results, pieces, small_ds.reads, split)
    assert cfa == want.correct_fa
    assert dfa == want.discard_fa
    names = ("total_reads_len", "corrected_len", "total_seed_num", "total_walk_num", "high_error_num", "exceed_depth_num",
             "exceed_leave_num", "fm_num", "dp_num", "seed_dis", "merge")
    got = np.array([[getattr(r, n) for n in names] for r in results], dtype=np.int64)
    np.testing.assert_array_equal(got, want.counters)
    assert got[:, 7].sum() > 500 and (got[:, 4].sum() + got[:, 5].sum()) > 0      # many FM walks, some failures
    want.close(); ob.close(); orb.close()


# ---- repeat-rich data: mode-2 attributes, isRepeat seeds, repeat-to-unique (reverse-strand) walks ---------------
@pytest.fixture(scope="module")
def rep_index(api, repeat_ds):
    idx = api.index_open(repeat_ds.prefix + ".bwt", repeat_ds.prefix + ".rbwt")
    idx.upload(0)
    yield idx
    idx.close()


@pytest.mark.parametrize("genome", [5, 10])
def test_repeat_dataset_seeds_walks_and_fasta(api, rep_index, oracle, repeat_ds, genome, correct_mode):
    p = api.params_default(genome, 90)
    p.no_dp = 1
    ob, orb = oracle.bwt_load(repeat_ds.prefix + ".bwt"), oracle.bwt_load(repeat_ds.prefix + ".rbwt")
    n_reads = 200
    off = repeat_ds.off[: n_reads + 1].copy()
    bases = repeat_ds.bases[: int(off[-1])]
    # seeds + attribute
    ctx = rep_index.ctx(p, 0)
    b = ctx.batch(bases, off)
    b.find_seeds()
    count, seeds, attr = b.seeds()
    b.close()
    wcount, wseeds, wattr = oracle.find_seeds(ob, orb, p, bases, off)
    np.testing.assert_array_equal(attr, wattr)
    np.testing.assert_array_equal(count, wcount)
    np.testing.assert_array_equal(np.stack([seeds[f] for f in seeds.dtype.names], axis=1), wseeds)
    assert (wattr == 2).mean() > 0.01 and wseeds[:, 3].sum() > 5           # repeat mode + repeat seeds really occur
    # walks, including the reversed ones
    reads = repeat_ds.reads[:n_reads]
    descs = _walk_descs(p, reads, wcount, wseeds)
    n_rtou = 0
    k = 0
    for r, n in enumerate(wcount):
        ss = wseeds[k: k + n]; k += n
        n_rtou += int(sum(1 for i in range(max(int(n) - 1, 0)) if ss[i][3] and not ss[i + 1][3]))
    assert n_rtou >= 1
    got = ctx.extend_walks(descs)
    for d, (code, merged, steps) in zip(descs, got):
        wcode, wmerged, wst = oracle.extend_walk(ob, orb, p, *d)
        assert (code, merged, steps) == (wcode, wmerged, wst[0]), d
    # whole path
    want = oracle.correct_reads(ob, orb, p, bases, off)
    results, pieces = ctx.correct_reads(bases, off)
    cfa, dfa = _fasta(results, pieces, reads, 0)
    assert cfa == want.correct_fa and dfa == want.discard_fa
    names = ("total_reads_len", "corrected_len", "total_seed_num", "total_walk_num", "high_error_num", "exceed_depth_num",
             "exceed_leave_num", "fm_num", "dp_num", "seed_dis", "merge")
    np.testing.assert_array_equal(np.array([[getattr(r, n) for n in names] for r in results], dtype=np.int64), want.counters)
    ctx.close(); want.close(); ob.close(); orb.close()


def test_lf_walk_matches_oracle(gpu_ctx, oracle, small_ds):
    """retrieveStr's LF-walk (LongReadOverlap.cpp:696-749): char by char vs getChar/getPC/getOcc of the oracle,
    from '$'-adjacent rows, interval rows of real k-mers and random rows, on both strands."""
    rng = np.random.default_rng(21)
    for strand, ext in ((0, "bwt"), (1, "rbwt")):
        ob = oracle.bwt_load(f"{small_ds.prefix}.{ext}")
        n = ob.num_symbols
        rows = np.concatenate([np.arange(0, 6), np.arange(small_ds.n_reads - 3, small_ds.n_reads + 3),
                               rng.integers(0, n, size=40)]).astype(np.uint64)
        steps = rng.integers(1, 400, size=rows.size).astype(np.uint32)
        got = gpu_ctx.lf_walk(rows, np.full(rows.size, strand, dtype=np.uint8), steps)
        for row, ms, g in zip(rows, steps, got):
            idx, want = int(row), []
            for _ in range(int(ms)):
                c = chr(int(ob.chars(np.array([idx], dtype=np.uint64))[0]))
                if c == "$":
                    break
                want.append(c)
                idx = ob.pc(c) + int(ob.occ(np.frombuffer(c.encode(), dtype=np.uint8), np.array([idx - 1], dtype=np.int64))[0])
            assert g == "".join(want)
        ob.close()


# ---- DP/MSA fallback: Overlapper::extendMatch --------------------------------------------------------------------
def _mutate(rng, s, sub, ins, dele):
    out = []
    for c in s:
        u = rng.random()
        if u < dele:
            continue
        if u < dele + sub:
            c = "ACGT"[rng.integers(4)]
        out.append(c)
        while rng.random() < ins:
            out.append("ACGT"[rng.integers(4)])
    return "".join(out)


def _dp_pairs(rng, small_ds, n):
    """(s1, s2, start1, start2) the way retrieveMatches calls extendMatch (LongReadOverlap.cpp:635-643): forward pairs
    share their first k-mer, reverse pairs their last one; error profiles from identical to hopeless, homopolymer runs,
    short / truncated s2 (the LF-walk hit a '$'), s2 longer than the band."""
    g = small_ds.genome.tobytes().decode()
    pairs = []
    for t in range(n):
        L = int(rng.integers(30, 420))
        p = int(rng.integers(0, len(g) - 2 * L - 50))
        q = g[p: p + L]
        if t % 7 == 3:                                    # homopolymer-rich query
            q = "".join(c * int(rng.integers(1, 5)) for c in q[: L // 2])
        k = 17
        err = [(0, 0, 0), (0.01, 0.03, 0.02), (0.015, 0.09, 0.045), (0.05, 0.15, 0.1), (0.3, 0.3, 0.3)][t % 5]
        if t % 2 == 0:                                    # forward: same first k-mer, s2 runs ~1.1 |q| + 20 or stops early
            tail = _mutate(rng, q[k:] + g[p + L: p + L + 60], *err)
            m = int(len(q) * 1.1 + 20) if t % 3 else int(rng.integers(k, len(q)))
            s2 = (q[:k] + tail)[:m]
            pairs.append((q, s2, 0, 0))
        else:                                             # reverse: same last k-mer
            head = _mutate(rng, g[max(p - 60, 0): p] + q[:-k], *err)
            m = int(len(q) * 1.1 + 20) if t % 3 else int(rng.integers(k, len(q)))
            s2 = (head + q[-k:])[-m:]
            pairs.append((q, s2, len(q) - k, len(s2) - k))
    # the band (201) cut by both matrix edges, and one-column / one-row corner cases
    pairs += [("ACGTACGTACGTACGTACGT", "ACGTACGTACGTACGTACGT", 0, 0), ("A" * 40, "A" * 25, 0, 0), ("ACGT" * 80, "ACGT" * 20, 0, 0),
              ("ACGT" * 20, "ACGT" * 100, 0, 0), ("ACGTTGCA" * 4, "T", 0, 0), ("G", "ACGTTGCA" * 4, 0, 0),
              ("ACGT" * 90, "TTGCA" * 90, 343, 433)]
    return pairs


def test_dp_align_matches_oracle_extend_match(gpu_ctx, oracle, small_ds):
    """Every field of SequenceOverlap and the cigar, bit-identical to the oracle's extend_match (itself checked against
    the reference's overlapper.cpp object code in tests/test_oracle_vs_ref.py)."""
    rng = np.random.default_rng(77)
    pairs = _dp_pairs(rng, small_ds, 240)
    got = gpu_ctx.dp_align(pairs)
    n_gapped = 0
    for (s1, s2, a, b), g in zip(pairs, got):
        want = oracle.extend_match(s1, s2, a, b)
        assert g == want, (s1, s2, a, b)
        n_gapped += ("I" in want["cigar"]) + ("D" in want["cigar"])
    assert n_gapped > 100
    for bw in (2, 11, 64, 254):                           # other band widths: the band edges move through the matrix
        sub = pairs[:40] + pairs[-7:]
        got = gpu_ctx.dp_align(sub, band_width=bw, scores=(2, -3, -5))
        for (s1, s2, a, b), g in zip(sub, got):
            assert g == oracle.extend_match(s1, s2, a, b, bandwidth=bw, scores=(2, -3, -5)), (bw, s1, s2, a, b)


def _dp_queries(rng, ds, n):
    """(query, k, min_overlap, min_identity, min_call_coverage) the way correctByMSAlignment builds them
    (PacBioSelfCorrectionProcess.cpp:208-236): query = a read substring (source k-mer + gap + target seed)."""
    out = []
    for t in range(n):
        r = int(rng.integers(len(ds.reads)))
        read = ds.reads[r]
        L = int(rng.integers(60, 400))
        if len(read) < L + 2:
            continue
        p = int(rng.integers(0, len(read) - L))
        q = read[p: p + L]
        k = int(rng.choice([13, 15, 17, 19]))
        ident = [0.65, 0.65 + 0.05, 0.65 + 0.05 + 0.05][t % 3]
        out.append((q, k, len(q) // 10, ident, [15, 15, 24, 40][t % 4]))
    return out


@pytest.mark.parametrize("cov,force_global,row_batch", [(90, False, True), (20, False, True), (90, True, True),
                                                        (90, False, False), (20, True, False)])
def test_dp_consensus_matches_oracle(api, gpu_index, oracle, small_ds, cov, force_global, row_batch, monkeypatch):
    """retrieveStr + extendMatch + MultipleAlignment + calculateBaseConsensus: rows, retrieved-string count and the
    consensus string, bit-identical to the oracle's line-by-line restatement of LongReadOverlap.cpp / multiple_alignment.cpp.
    row_batch False keeps the kernel's step-by-step cigar walk (the path the corner-case rows take) under test."""
    if force_global:
        monkeypatch.setenv("LRSC_MSA_FORCE_GLOBAL", "1")       # the pile-up state in global memory instead of LDS (very wide pile-ups)
    if not row_batch:
        monkeypatch.setenv("LRSC_MSA_BATCH", "0")
    rng = np.random.default_rng(1234 + cov)
    qs = _dp_queries(rng, small_ds, 60)
    p = api.params_default(5, cov)
    ctx = gpu_index.ctx(p, 0)
    got = ctx.dp_consensus(qs)
    walked, added = ctx.msa_rows_by_step_walk, sum(g[0] - 1 for g in got)
    ctx.close()
    assert walked == added if not row_batch else walked * 10 < added      # the switch selects the path it says
    ob, orb = oracle.bwt_load(small_ds.prefix + ".bwt"), oracle.bwt_load(small_ds.prefix + ".rbwt")
    n_multi = 0
    for (q, k, mo, mi, mc), g in zip(qs, got):
        want = oracle.dp_consensus(ob, orb, q, k, mo, mi, cov, mc)
        assert g == want, (q, k, mo, mi, mc)
        n_multi += want[0] > 3
    assert n_multi >= 10                                   # real pile-ups, not only "too few rows"
    ob.close(); orb.close()


def test_repeat_dataset_with_dp_fallback(api, rep_index, oracle, repeat_ds):
    p = api.params_default(5, 90)
    p.no_dp = 0
    _check_whole_path(api, rep_index, oracle, repeat_ds, p, n_reads=120, min_fm=100, min_dp=5)


# ---- the wide layout (Block64: 64-bit counters, 128 symbols per block; indexes of >= 2^31 symbols per strand) --------
@pytest.fixture(scope="module")
def wide_index(api, small_ds):
    import os
    os.environ["LRSC_FORCE_WIDE"] = "1"
    try:
        idx = api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")
    finally:
        del os.environ["LRSC_FORCE_WIDE"]
    idx.upload(0)
    assert idx.info().block_symbols == 128
    yield idx
    idx.close()


def test_wide_layout_rank_chars_kmers_seeds(api, wide_index, oracle, small_ds):
    p = api.params_default(5, 90)
    ctx = wide_index.ctx(p, 0)
    ob, orb = oracle.bwt_load(small_ds.prefix + ".bwt"), oracle.bwt_load(small_ds.prefix + ".rbwt")
    rng = np.random.default_rng(5)
    n = ob.num_symbols
    for strand, o in ((0, ob), (1, orb)):
        idx = np.concatenate([rng.integers(-1, n, 50000), np.array([-1, 0, 1, 127, 128, 129, 255, 256, n - 2, n - 1]),
                              np.arange(-1, min(n, 2048))]).astype(np.int64)
        base = rng.choice(ACGT, size=idx.size)
        np.testing.assert_array_equal(ctx.rank(base, idx, strand), o.occ(base, idx))
        rows = np.arange(0, n, 7, dtype=np.uint64)
        np.testing.assert_array_equal(ctx.bwt_chars(strand, rows), o.chars(rows))
    count, seeds, attr = None, None, None
    b = ctx.batch(small_ds.bases, small_ds.off)
    b.find_seeds()
    count, seeds, attr = b.seeds()
    b.close()
    wcount, wseeds, wattr = oracle.find_seeds(ob, orb, p, small_ds.bases, small_ds.off)
    np.testing.assert_array_equal(attr, wattr)
    np.testing.assert_array_equal(count, wcount)
    np.testing.assert_array_equal(np.stack([seeds[f] for f in seeds.dtype.names], axis=1), wseeds)
    ctx.close(); ob.close(); orb.close()


@pytest.mark.parametrize("nodp", [1, 0])
def test_wide_layout_whole_path(api, wide_index, oracle, small_ds, nodp):
    p = api.params_default(5, 90)
    p.no_dp = nodp
    _check_whole_path(api, wide_index, oracle, small_ds, p, min_fm=300, min_dp=0 if nodp else 20)


@pytest.mark.parametrize("nodp", [1, 0])
def test_whole_path_ragged_and_foreign_reads(api, gpu_index, oracle, small_ds, nodp):
    """The whole per-read path on awkward inputs: reads shorter than k, one base, absent from the index, homopolymers, a chimera
    with a long unseeded stretch (a long DP query), duplicated halves -- FASTA and counters identical to the oracle."""
    from oracle.oracle_py import pack_reads

    rng = np.random.default_rng(23)
    real = small_ds.reads
    foreign = "".join(rng.choice(list("ACGT"), size=900))
    chimera = real[2][:400] + foreign[:600] + real[5][200:900] + "A" * 40 + real[7][:300]
    reads = ["ACGT", real[0][:16], real[0][:19], real[1][:60], foreign, chimera, "A" * 300, "AC" * 200, real[3], real[4][100:101],
             real[6][:500] + real[6][:500], real[8], real[9][:1200], real[10][300:]]
    bases, off = pack_reads(reads)
    p = api.params_default(5, 90)
    p.no_dp = nodp
    ob, orb = oracle.bwt_load(small_ds.prefix + ".bwt"), oracle.bwt_load(small_ds.prefix + ".rbwt")
    want = oracle.correct_reads(ob, orb, p, bases, off)
    ctx = gpu_index.ctx(p, 0)
    results, pieces = ctx.correct_reads(bases, off)
    ctx.close()
    cfa, dfa = _fasta(results, pieces, reads, 0)
    assert cfa == want.correct_fa and dfa == want.discard_fa
    names = ("total_reads_len", "corrected_len", "total_seed_num", "total_walk_num", "high_error_num", "exceed_depth_num",
             "exceed_leave_num", "fm_num", "dp_num", "seed_dis", "merge")
    np.testing.assert_array_equal(np.array([[getattr(r, n) for n in names] for r in results], dtype=np.int64), want.counters)
    assert want.counters[:, 10].sum() >= 5 and (want.counters[:, 10] == 0).sum() >= 5        # corrected and discarded reads both occur
    want.close(); ob.close(); orb.close()


def test_per_read_capacity_limits_do_not_fail_the_batch(api, gpu_index, oracle, small_ds):
    """A read whose walk query would be >= 65535 bases comes back uncorrected with a per-read status; every other read of the batch
    is corrected exactly as the oracle does -- including one whose DP-fallback query (a 36 kb gap between two seeds) is beyond the
    alignment kernel's LDS staging: its alignments run through the global-workspace variant of the kernel (the reference has no
    bound there: Thirdparty/overlapper.cpp:421-701, PacBio/LongReadOverlap.cpp:17-55)."""
    from oracle.oracle_py import pack_reads

    rng = np.random.default_rng(99)
    reads = list(small_ds.reads[:12])
    junk = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    far = reads[0][:1000] + junk(70000) + reads[1][-1000:]          # the only seeds are 70 kb apart: walk query too long
    dpl = reads[2][:1000] + junk(36000) + reads[3][-1000:]          # 36 kb gap: FM-extension fails, the DP query is beyond the LDS staging
    batch = reads[:6] + [far] + reads[6:9] + [dpl] + reads[9:]
    bases, off = pack_reads(batch)
    p = api.params_default(5, 90)
    ctx = gpu_index.ctx(p, 0)
    results, pieces = ctx.correct_reads(bases, off)
    ctx.close()
    assert results[6].status == 1 and results[6].merge == 0 and pieces[6] == []
    ok = [i for i in range(len(batch)) if i != 6]
    assert all(results[i].status == 0 for i in ok)
    ob, orb = oracle.bwt_load(small_ds.prefix + ".bwt"), oracle.bwt_load(small_ds.prefix + ".rbwt")
    b2, o2 = pack_reads([batch[i] for i in ok])
    want = oracle.correct_reads(ob, orb, p, b2, o2)
    names = ("total_reads_len", "corrected_len", "total_seed_num", "total_walk_num", "high_error_num", "exceed_depth_num",
             "exceed_leave_num", "fm_num", "dp_num", "seed_dis", "merge")
    got = np.array([[getattr(results[i], f) for f in names] for i in ok], dtype=np.int64)
    np.testing.assert_array_equal(got, want.counters)
    assert [pieces[i][0] for i in ok if results[i].merge] == want.correct_fa.split("\n")[1::2]
    want.close(); ob.close(); orb.close()
