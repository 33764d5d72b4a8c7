"""bench.py --dump-outputs on CPU: what dump_outputs writes for hand-made correct / seeds results (the GPU run fills the same
structures from the batch API)."""
from __future__ import annotations

import zlib

import numpy as np

import bench
from longreadselfcorrect_amd.capi import SEED_DTYPE, ReadResult


def _part(reads):
    """reads: list of (merge, [piece bytes]) -> (ReadResult[n], piece offsets, corrected bytes) as Batch.correct returns them."""
    res = (ReadResult * len(reads))()
    pieces = []
    for r, (merge, ps) in zip(res, reads):
        r.merge, r.n_pieces, r.piece_first = merge, len(ps), len(pieces)
        r.corrected_len, r.total_walk_num, r.status = sum(map(len, ps)), 7, 0
        pieces += ps
    poff = np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.uint64)
    return res, poff, np.frombuffer(b"".join(pieces), dtype=np.uint8)


def test_correct_outputs_join_the_parts_in_read_order(tmp_path):
    a = _part([(1, [b"ACGT", b"GG"]), (0, [])])
    b = _part([(1, [b"TTTTA"])])
    sizes = bench.dump_outputs(tmp_path, "correct", [a, b])
    got = {n: np.load(tmp_path / f"{n}.npy") for n in sizes}
    assert set(got) == {"read_results", "piece_lengths", "piece_crc32", "sample_reads", "sample_bases"}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    rr = got["read_results"]
    assert rr.shape == (3, len(bench.READ_RESULT_COLUMNS))
    col = bench.READ_RESULT_COLUMNS.index
    assert rr[:, col("merge")].tolist() == [1, 0, 1] and rr[:, col("n_pieces")].tolist() == [2, 0, 1]
    assert rr[:, col("corrected_len")].tolist() == [6, 0, 5]
    assert got["piece_lengths"].tolist() == [4, 2, 5]
    assert got["piece_crc32"].tolist() == [zlib.crc32(p) for p in (b"ACGT", b"GG", b"TTTTA")]
    assert got["sample_reads"].tolist() == [0, 1, 2]                 # fewer reads than the sample size: all of them
    assert bytes(got["sample_bases"].astype(np.uint8)) == b"ACGTGGTTTTA"


def test_sample_is_fixed_and_bounded():
    nbytes = np.full(100_000, 4 * 10_000, dtype=np.int64)           # 10 kb reads as float32
    s1, s2 = bench.dump_sample(nbytes.size, nbytes), bench.dump_sample(nbytes.size, nbytes)
    assert np.array_equal(s1, s2) and s1.size == bench.DUMP_SAMPLE_READS and np.all(np.diff(s1) > 0)
    assert nbytes[s1].sum() <= bench.DUMP_SAMPLE_BYTES
    big = np.full(100_000, 4 * 1_000_000, dtype=np.int64)            # 1 Mb reads: the sample shrinks to the byte budget
    assert 0 < big[bench.dump_sample(big.size, big)].sum() <= bench.DUMP_SAMPLE_BYTES


def test_seed_outputs(tmp_path):
    count = np.array([2, 0, 1], dtype=np.uint32)
    seeds = np.zeros(3, dtype=SEED_DTYPE)
    seeds["start"], seeds["len"] = [0, 50, 7], [17, 19, 15]
    bench.dump_outputs(tmp_path, "seeds", [(count, seeds)])
    assert np.load(tmp_path / "seed_count.npy").tolist() == [2, 0, 1]
    ss = np.load(tmp_path / "sample_seeds.npy")
    assert ss.dtype == np.float64 and ss.shape == (3, 8)
    assert ss[:, 0].tolist() == [0, 50, 7] and ss[:, 1].tolist() == [17, 19, 15]
