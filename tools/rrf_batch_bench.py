"""Composed queries/s of pvs_rrf_search_batch against pvs_rrf_search at the configs[4] shape: two 25M-row int8 indexes (512-d
cosine, rrf 5 / 1.0 and 1024-d L2, rrf 10 / 0.7), MIN per file, ~3 rows per file.  Per batch size: one warm-up call, then the
median of --calls calls; the first 8 pages of every batch are checked against single calls.

    python tools/rrf_batch_bench.py [--rows 25000000] [--batches 1,8,32,128] [--calls 10] [--only-batch 32] [--out FILE]

--only-batch B: build, warm up and time batch B alone (for a profiler run around it)."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import panoptikon_amd as pvs  # noqa: E402
from panoptikon_amd import _lib as L  # noqa: E402


def build_i8(n, dim, seed, gstride, chunk=1_000_000):
    """bench.py's configs[4] branch: rows from the device generator, the scale from their absmax (one pass), then the index."""
    lib = pvs.lib()
    stage = pvs.DeviceBuffer(chunk * dim * 4)
    amax = 0.0
    for off in range(0, n, chunk):
        m = min(chunk, n - off)
        L.check(lib.pvs_synth_rows_f32(0, seed, off, m, dim, stage.ptr))
        out = C.c_float()
        L.check(lib.pvs_absmax(stage.ptr, m * dim, L.DEVICE, 0, C.byref(out)))
        amax = max(amax, float(out.value))
    ix = pvs.VectorIndex(pvs.I8, dim, capacity_rows=n)
    ix.set_scale(pvs.scale_from_absmax(amax))
    for off in range(0, n, chunk):
        m = min(chunk, n - off)
        L.check(lib.pvs_synth_rows_f32(0, seed, off, m, dim, stage.ptr))
        g = (np.arange(off, off + m, dtype=np.int64) // 3) * gstride
        L.check(lib.pvs_index_add_f32(ix._h, stage.ptr, m, None, g.ctypes.data, L.DEVICE))
    stage.free()
    return ix


SEED_QUERY = 0x5EED0000  # bench.py's query seed; branch b draws from SEED_QUERY + 17 b


def queries(branch, n, dim):
    """n f32 query vectors from the device generator, as bench.py draws them (rows 0..n-1 of the branch's query seed)."""
    qb = pvs.DeviceBuffer(n * dim * 4)
    L.check(pvs.lib().pvs_synth_rows_f32(0, SEED_QUERY + 17 * branch, 0, n, dim, qb.ptr))
    q = qb.to_numpy(np.float32, (n, dim)).copy()
    qb.free()
    return q


def median_ms(fn, calls):
    fn()  # warm-up
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=25_000_000)
    ap.add_argument("--batches", default="1,8,32,128")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--only-batch", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if pvs.device_count() < 1:
        sys.exit("needs a gfx950 device")
    t0 = time.perf_counter()
    img = build_i8(a.rows, 512, 11, 1)
    txt = build_i8(a.rows, 1024, 12, 2)
    build_s = time.perf_counter() - t0
    batches = [a.only_batch] if a.only_batch else [int(b) for b in a.batches.split(",")]
    qi, qt = queries(0, max(batches), 512), queries(1, max(batches), 1024)

    def branches(nq):
        return [dict(index=img, query=qi[:nq], metric=pvs.COSINE, agg=pvs.AGG_MIN, rrf_k=5, weight=1.0),
                dict(index=txt, query=qt[:nq], metric=pvs.L2, agg=pvs.AGG_MIN, rrf_k=10, weight=0.7)]

    res = dict(rows=a.rows, k=a.k, build_s=round(build_s, 1), calls=a.calls, batches={})
    if a.only_batch:
        ms, _ = median_ms(lambda: pvs.rrf_search_batch(branches(a.only_batch), a.k), a.calls)
        res["batches"][a.only_batch] = dict(ms=round(ms, 3), qps=round(a.only_batch / ms * 1e3, 1))
    else:
        one = [dict(b, query=b["query"][0]) for b in branches(1)]
        single_ms, _ = median_ms(lambda: pvs.rrf_search(one, a.k), a.calls)
        res["single"] = dict(ms=round(single_ms, 3), qps=round(1e3 / single_ms, 1), path=int(pvs.lib().pvs_rrf_last_path()))
        for nq in batches:
            brs = branches(nq)
            g, s, c = pvs.rrf_search_batch(brs, a.k)
            path = int(pvs.lib().pvs_rrf_last_path())
            for j in range(min(8, nq)):  # the first 8 pages against single calls
                g1, s1 = pvs.rrf_search([dict(b, query=b["query"][j]) for b in brs], a.k)
                if not (c[j] == len(g1) and np.array_equal(g[j, : c[j]], g1) and np.array_equal(s[j, : c[j]].view(np.uint64), s1.view(np.uint64))):
                    sys.exit(f"batch {nq}: page {j} differs from its single call")
            ms, all_ms = median_ms(lambda: pvs.rrf_search_batch(brs, a.k), a.calls)
            qps = nq / ms * 1e3
            res["batches"][nq] = dict(ms=round(ms, 3), qps=round(qps, 1), x_single=round(qps / res["single"]["qps"], 2), path=path,
                                      min_ms=round(min(all_ms), 3), max_ms=round(max(all_ms), 3))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    img.close()
    txt.close()


if __name__ == "__main__":
    main()
