"""The product's hash-guided seed-pair merge (csrc/saipb_device.h: the source saipb_merge_kernel compiles for gfx950), compiled for
the host by tests/host_saipb and run on the CPU with one lane against the oracle's restatement of SAIPBSelfCorrectTree: return code,
merged sequence, step count, widest frontier, result count, hash entries and both seed frequencies of every seed pair, over the
narrow and the wide rank-block layout, with and without k-mer tables; and the device alignment helper against the reference's
known answers.  The GPU parity tests (test_gpu_saipb_kernel.py) run the same source on the device.

Return code -2 (search depth exceeded) occurs in none of the seed-pair sets themselves: it needs a frontier that survives beyond
maxLength without ever meeting the target.  A wrong target gives that: wrong_target_pairs() takes the first 120 merged small_ds
pairs and replaces each target by a pseudo-random string of the same length, once with the pair's gap and once with a third of it,
so the walk follows the reads past a target it can never meet.  On the oracle 2 of those 240 inputs end -2 (both from pair 166: 55
and 51 steps, at most 3 leaves), the others -1 or -4; the test asserts that at least one -2 occurs.

Coverage that does NOT exist: -5 is unreachable by construction (the loop only ends on one of the other conditions)."""
from __future__ import annotations

import json

import numpy as np
import pytest

from tests.host_saipb import HostSaipb

from .conftest import GOLDEN
from .test_saipb_oracle import _pairs


@pytest.fixture(scope="module")
def hs():
    return HostSaipb()


def _units(ds):
    u = [np.fromfile(f"{ds.prefix}.{ext}", dtype=np.uint8)[30:] for ext in ("bwt", "rbwt")]
    return u, int(ds.off[-1]) + ds.n_reads


def wrong_target_pairs(pairs, codes, n=120):
    """The first n merged pairs (codes: the oracle's return codes of `pairs`) with a target the reads do not contain, each with its
    own gap and with a third of it, at least 1, as an empty rawSeq is an argument error (`between` cut to the gap used).  The generator is spelled out so that the inputs never change."""
    x, out = 1, []
    for (s, b, t, d), _ in [pc for pc in zip(pairs, codes) if pc[1] == 1][:n]:
        wrong = ""
        for _ in t:
            x = (x * 1103515245 + 12345) & 0x7FFFFFFF
            wrong += "ACGT"[(x >> 16) & 3]
        out += [(s, b[:dd], wrong, dd) for dd in (d, max(d // 3, 1))]
    return out


def _want(oracle, ob, orb, pairs, max_leaves):
    return [oracle.saipb_merge(ob, orb, s, b, t, d, max_leaves) for s, b, t, d in pairs]


def _compare(got, want, pairs):
    assert len(got) == len(want)
    for g, w, p in zip(got, want, pairs):
        assert g[3] == 0, ("status", g[3], p)
        assert (g[0], g[1], g[2]) == (w[0], w[1], w[2]), p


def _run(hs, api, oracle, ds, max_leaves=32, wide=False, tables=(5, 9, 11), limit=None, min_target=0, wrong_target=False):
    ob, orb, _, raw = _pairs(oracle, api, ds, 60)
    pairs = [(s, b, t, d) for _, s, b, t, d in raw if len(t) >= min_target]
    if limit:
        pairs = pairs[:limit]
    if wrong_target:
        pairs = wrong_target_pairs(pairs, [w[0] for w in _want(oracle, ob, orb, pairs, 32)])
    (u0, u1), n_sym = _units(ds)
    h = hs.index(u0, u1, n_sym, wide=wide, tables=tables)
    got = hs.merge_pairs(h, pairs, max_leaves)
    hs.index_free(h)
    want = _want(oracle, ob, orb, pairs, max_leaves)
    ob.close(); orb.close()
    _compare(got, want, pairs)
    return pairs, want


def test_host_saipb_matches_oracle_on_all_small_pairs(hs, api, oracle, small_ds):
    pairs, want = _run(hs, api, oracle, small_ds)
    codes = [w[0] for w in want]
    assert len(pairs) == 672
    # the shape of the set, so that no path goes untested unnoticed: merges, failures, and the alignment among several results
    assert sum(c == 1 for c in codes) > 250 and sum(c != 1 for c in codes) > 20
    assert sum(w[2]["results"] > 1 for w in want) >= 50
    assert set(codes) <= {1, -1, -3, -4}                       # -2 needs the wrong targets below; -5 does not occur (module docstring)


def test_host_saipb_matches_oracle_on_wrong_targets_with_search_depth_exceeded(hs, api, oracle, small_ds):
    """A target the reads do not contain: the walk runs on until it dies (-1, -4) or passes maxLength (-2)."""
    pairs, want = _run(hs, api, oracle, small_ds, wrong_target=True)
    codes = [w[0] for w in want]
    assert len(pairs) == 240 and 1 not in codes
    assert sum(c == -2 for c in codes) >= 1
    _run(hs, api, oracle, small_ds, wide=True, tables=(), wrong_target=True)


def test_host_saipb_matches_oracle_with_eight_leaves(hs, api, oracle, small_ds):
    pairs, want = _run(hs, api, oracle, small_ds, max_leaves=8)
    assert len(pairs) == 672 and sum(w[0] == -3 for w in want) >= 10


def test_host_saipb_matches_oracle_on_the_repeat_set(hs, api, oracle, repeat_ds):
    """Targets of at least 17 bases (shorter ones make the reference's substr throw): -3 at 32 leaves, and seeds the repeat guard
    skips (hash_entries == 0)."""
    pairs, want = _run(hs, api, oracle, repeat_ds, tables=(5, 9), min_target=17)
    assert len(pairs) == 736
    assert sum(w[0] == -3 for w in want) > 0 and sum(w[2]["hash_entries"] == 0 for w in want) > 0


def test_host_saipb_without_tables_and_wide_layout(hs, api, oracle, small_ds):
    _run(hs, api, oracle, small_ds, tables=(), limit=150)
    _run(hs, api, oracle, small_ds, wide=True, tables=(5, 9), limit=150)
    _run(hs, api, oracle, small_ds, wide=True, tables=(), limit=60)


def test_host_saipb_alignment_matches_reference_kats(hs):
    kats = json.loads((GOLDEN / "stdaln_kats.json").read_text())["cases"]
    assert len(kats) == 160
    for c in kats:
        if set(c["s1"] + c["s2"]) <= set("ACGT"):
            assert hs.align(c["s1"], c["s2"]) == (c["matches"], c["score"], c["path_len"]), (c["s1"], c["s2"])
        else:
            pytest.fail("the device helper takes A, C, G, T only; every known answer is expected to be of that alphabet")


def test_host_saipb_rejects_what_the_reference_throws_on(hs, api, oracle, small_ds):
    from longreadselfcorrect_amd.capi import saipb_pair_jobs

    (u0, u1), n_sym = _units(small_ds)
    h = hs.index(u0, u1, n_sym, tables=(5,))
    src = "ACGT" * 15
    seq, seeds, jobs = saipb_pair_jobs([(src, "ACGTACGTAC", "ACGTACGTACGTACGTACG", 10)])
    seeds[3].len = 16                                      # shorter than its large k-mer of 17
    assert hs.merge(h, seq, seeds, jobs)[0] == -3          # LRSC_ERR_ARG
    seq, seeds, jobs = saipb_pair_jobs([(src, "ACGTACGTAC", "ACGTACGTACGTACGTACG", 10)])
    jobs[0].hash_kmer = 32
    assert hs.merge(h, seq, seeds, jobs)[0] == -7          # LRSC_ERR_UNSUPPORTED
    jobs[0].hash_kmer, jobs[0].max_leaves = 15, 65
    assert hs.merge(h, seq, seeds, jobs)[0] == -7
    # matches and columns of an alignment share a word: rawSeq against the longest candidate must stay within 65 535 columns
    seq, seeds, jobs = saipb_pair_jobs([(src, "ACGT" * 7000, "ACGTACGTACGTACGTACG", 28000)])
    assert jobs[0].raw_len == 28000 and jobs[0].max_length < 32000
    assert hs.merge(h, seq, seeds, jobs)[0] == 0                # 28 000 + 30 865 + 19 columns at most
    jobs[0].max_length = 31999
    seeds[3].max_length = 31999
    assert jobs[0].raw_len + jobs[0].max_length + jobs[0].dest_len == 60018 and hs.merge(h, seq, seeds, jobs)[0] == 0
    seq, seeds, jobs = saipb_pair_jobs([(src, "ACGT" * 7000, "ACGTACGTACGTACGTACG" * 400, 28000)])
    jobs[0].max_length = seeds[3].max_length = 31999             # every string and length within 32 000, the sum is not
    assert jobs[0].raw_len + jobs[0].max_length + jobs[0].dest_len == 67599 and hs.merge(h, seq, seeds, jobs)[0] == -7
    hs.index_free(h)


def test_cpp_recipe_equals_python_recipe(tmp_path):
    """stride::saipbPairJob (host/SAIPBSelfCTree.h) and capi.saipb_pair_jobs fill the same records for the same pairs."""
    import subprocess

    from longreadselfcorrect_amd.capi import saipb_pair_jobs

    from .conftest import REPO

    src = tmp_path / "recipe.cpp"
    src.write_text(r'''
#include <iostream>
#include "longreadselfcorrect_amd/host/SAIPBSelfCTree.h"
int main() {
    std::string s, b, t, seq; int dis; uint32_t n = 0;
    while(std::cin >> s >> b >> t >> dis) {
        lrsc_saipb_seed sd[4]; lrsc_saipb_job j;
        stride::saipbPairJob(s, b, t, dis, 32, 4 * n, seq, sd, j);
        for(int q = 0; q < 4; ++q) std::cout << sd[q].seq_off << ' ' << sd[q].len << ' ' << sd[q].large_kmer << ' ' << sd[q].max_length << ' '
                                             << sd[q].expected_length << ' ' << sd[q].skip_repeat << ' ';
        std::cout << j.raw_off << ' ' << j.raw_len << ' ' << j.src_off << ' ' << j.src_len << ' ' << j.dest_off << ' ' << j.dest_len << ' '
                  << j.seed_first << ' ' << j.n_seeds << ' ' << j.hash_kmer << ' ' << j.max_leaves << ' ' << j.min_length << ' ' << j.max_length
                  << ' ' << j.expected_length << ' ' << j.min_sa_threshold << '\n';
        ++n;
    }
    std::cout << seq << '\n';
}
''')
    exe = tmp_path / "recipe"
    subprocess.run(["g++", "-std=c++14", "-O1", f"-I{REPO}", "-o", str(exe), str(src)], check=True)
    pairs = [("ACGT" * 16, "ACGTTGCA" * n, "TTGACCA" * 3, 8 * n + d) for n, d in ((1, 0), (3, -5), (9, 4), (40, 30), (2, -14))]
    out = subprocess.run([str(exe)], input="".join(f"{s} {b} {t} {d}\n" for s, b, t, d in pairs), capture_output=True, text=True,
                         check=True).stdout.split("\n")
    seq, seeds, jobs = saipb_pair_jobs(pairs)
    assert out[len(pairs)] == seq.decode()
    for i in range(len(pairs)):
        want = []
        for q in range(4):
            sd = seeds[4 * i + q]
            want += [sd.seq_off, sd.len, sd.large_kmer, sd.max_length, sd.expected_length, sd.skip_repeat]
        j = jobs[i]
        want += [j.raw_off, j.raw_len, j.src_off, j.src_len, j.dest_off, j.dest_len, j.seed_first, j.n_seeds, j.hash_kmer, j.max_leaves,
                 j.min_length, j.max_length, j.expected_length, j.min_sa_threshold]
        assert [int(x) for x in out[i].split()] == want, i
