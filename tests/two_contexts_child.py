"""Child process of tests/test_gpu_two_contexts.py: corrects a read set on one device, first with one context, then as two halves
on two contexts from two host threads at once, and writes what came back as JSON.  The hardware queue count and the LRSC_* switches
are read when the runtime starts, hence a process of its own per setting:

    python tests/two_contexts_child.py PREFIX READS.npz OUT.json

PREFIX.bwt / PREFIX.rbwt: the index; READS.npz: bases, off."""
from __future__ import annotations

import json
import sys
import threading
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

NAMES = ("total_reads_len", "corrected_len", "total_seed_num", "total_walk_num", "high_error_num", "exceed_depth_num",
         "exceed_leave_num", "fm_num", "dp_num", "seed_dis", "merge", "status")


def rows(results, pieces):
    return [{"c": [int(getattr(r, n)) for n in NAMES], "p": list(ps)} for r, ps in zip(results, pieces)]


def main(prefix, reads_npz, out_json):
    from longreadselfcorrect_amd import Lrsc

    api = Lrsc()
    z = np.load(reads_npz)
    bases, off = z["bases"], z["off"].astype(np.uint64)
    n = len(off) - 1
    idx = api.index_open(prefix + ".bwt", prefix + ".rbwt")
    idx.upload(0)
    p = api.params_default(5, 90)
    p.no_dp = 0
    ctx = idx.ctx(p, 0)
    one = rows(*ctx.correct_reads(bases, off))
    ctx.close()

    cut = [0, n // 2, n]
    ctxs = [idx.ctx(p, 0) for _ in range(2)]
    halves, errors = [None, None], []

    def work(j):
        try:
            lo, hi = cut[j], cut[j + 1]
            sub_off = (off[lo: hi + 1] - off[lo]).astype(np.uint64)
            halves[j] = rows(*ctxs[j].correct_reads(bases[int(off[lo]): int(off[hi])], sub_off))
        except Exception as e:  # noqa: BLE001 - reported to the parent
            errors.append(f"part {j}: {e!r}")

    ths = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for t in ths: t.start()
    for t in ths: t.join()
    for c in ctxs: c.close()
    idx.close()
    if errors:
        sys.exit("; ".join(errors))
    Path(out_json).write_text(json.dumps({"one": one, "two": halves[0] + halves[1]}))


if __name__ == "__main__":
    main(*sys.argv[1:4])
