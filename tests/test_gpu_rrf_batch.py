"""pvs_rrf_search_batch: every page of a batch of composed queries is pvs_rrf_search's page for that query, bit for bit (groups,
f64 scores, counts, the -1 / NaN tail), and a sample of them is the oracle's literal composition.  Covers the one-pass fused scorer
(int8, groups as runs; the <= 4-query fold), the dense matrix (scattered groups, f16, f32), chunk boundaries, order keys, a batch
whose queries take different fusion paths, the in-order rescore of int8 L2 beyond the closed form's range, empty branches and
multi-device branches."""
import ctypes as C

import numpy as np
import pytest

import oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pvs():
    import panoptikon_amd as p

    if p.device_count() < 1:
        pytest.fail("no gfx950 device visible: the gpu tests need an MI355X")
    return p


def _index(pvs, kind, n, dim, seed, rows_per_group=2, devices=None, dup_of=None):
    """(index, oracle branch fields).  kind: i8runs (groups are runs of rows), i8scatter (groups scattered over the rows), f16, f32."""
    rows = orc.synth_rows(seed, 0, n, dim)
    if dup_of is not None:
        rows = rows[np.arange(n) % dup_of]  # duplicate-heavy: every row repeats the first dup_of rows, in different files
    grp = np.arange(n, dtype=np.int64) // rows_per_group
    if kind == "i8scatter":
        grp = np.random.default_rng(seed).permutation(grp)
    grp = grp * 3 + (seed % 3)  # ids that are not slot numbers
    if kind.startswith("i8"):
        scale = orc.compute_int8_scale(rows)
        codes = orc.quantize_int8(rows, scale)
        ix = pvs.VectorIndex(pvs.I8, dim, devices=devices)
        ix.set_scale(scale)
        ix.add(codes, group_ids=grp)
        return ix, dict(dtype=orc.I8, corpus=codes, groups=grp), scale
    dt, odt, npdt = (pvs.F16, orc.F16, np.float16) if kind == "f16" else (pvs.F32, orc.F32, np.float32)
    ix = pvs.VectorIndex(dt, dim, devices=devices)
    ix.add_f32(rows, group_ids=grp)
    return ix, dict(dtype=odt, corpus=rows.astype(npdt), groups=grp), None


def _queries(kind, scale, batch, dim, seed):
    q = orc.synth_rows(seed, 0, batch, dim)
    return orc.quantize_int8(q, scale) if kind.startswith("i8") else q


def _check(pvs, brs, k, oracle_brs=None, sample=(), expect_path=None):
    """The batch against one pvs_rrf_search per query (bit for bit), and the oracle for the queries in `sample`."""
    batch = brs[0]["query"].shape[0]
    g, s, c = pvs.rrf_search_batch(brs, k)
    assert g.shape == (batch, k) and s.shape == (batch, k) and c.shape == (batch,)
    batch_path = pvs.lib().pvs_rrf_last_path()
    paths = []
    for j in range(batch):
        one = [dict(b, query=b["query"][j]) for b in brs]
        g1, s1 = pvs.rrf_search(one, k)
        paths.append(pvs.lib().pvs_rrf_last_path())
        n = len(g1)
        assert c[j] == n, f"query {j}: count {c[j]} != {n}"
        assert np.array_equal(g[j, :n], g1), f"query {j}: groups differ"
        assert np.array_equal(s[j, :n].view(np.uint64), s1.view(np.uint64)), f"query {j}: scores differ"
        assert (g[j, n:] == -1).all() and np.isnan(s[j, n:]).all(), f"query {j}: unused slots"
    if batch:
        assert batch_path == max(paths), (batch_path, paths)
    if expect_path is not None:
        assert batch_path == expect_path
    for j in sample:
        ora = [dict(o, query=b["query"][j], metric=b["metric"], agg=b.get("agg", pvs.AGG_MIN), weights=b.get("row_weights"),
                    descending=b.get("descending", False), rrf_k=b.get("rrf_k", 1), weight=b.get("weight", 1.0)) for b, o in zip(brs, oracle_brs)]
        eg, es = orc.rrf_search(ora, k)
        assert np.array_equal(g[j, : c[j]], eg) and np.array_equal(s[j, : c[j]].view(np.uint64), es.view(np.uint64)), f"query {j} vs the oracle"
    return g, s, c


def test_parity_sweep_int8_runs_and_scattered_over_batch_sizes(pvs):
    """int8 with groups as runs (fused scorer; <= 4 queries: the fold) beside int8 with scattered groups (dense matrix); both metrics;
    batch sizes across the fold limit and the 32-query chunks; 75k files per branch: the bounded fusion serves them."""
    a, oa, sa = _index(pvs, "i8runs", 150_000, 256, 21)
    b, ob, sb = _index(pvs, "i8scatter", 150_000, 128, 22)
    for batch in (1, 3, 4, 5, 32, 33, 70):
        brs = [dict(index=a, query=_queries("i8", sa, batch, 256, 100 + batch), metric=pvs.COSINE, agg=pvs.AGG_MIN, rrf_k=5, weight=1.0),
               dict(index=b, query=_queries("i8", sb, batch, 128, 200 + batch), metric=pvs.L2, agg=pvs.AGG_AVG, rrf_k=10, weight=0.7)]
        _check(pvs, brs, 10, [oa, ob], sample=(0, batch - 1) if batch in (5, 33) else ())
    for k in (1, 500):
        brs = [dict(index=a, query=_queries("i8", sa, 33, 256, 7), metric=pvs.L2, agg=pvs.AGG_MAX, rrf_k=3, weight=1.0, descending=True),
               dict(index=b, query=_queries("i8", sb, 33, 128, 8), metric=pvs.COSINE, agg=pvs.AGG_MIN, rrf_k=1, weight=2.0)]
        _check(pvs, brs, k, [oa, ob], sample=(17,))
    a.close()
    b.close()


def test_parity_float_indexes_weights_and_three_branches(pvs):
    """f16 and f32 rows (dense matrix), MAX / AVG / weighted AVG, row_n descending; three branches, two of them on one index."""
    h, oh, _ = _index(pvs, "f16", 120_000, 96, 31)
    f, of, _ = _index(pvs, "f32", 100_000, 64, 32, rows_per_group=3)
    w = np.random.default_rng(5).uniform(0.1, 2.0, 100_000).astype(np.float32)
    for batch, k in ((5, 10), (33, 500), (4, 1)):
        brs = [dict(index=h, query=_queries("f16", None, batch, 96, 300 + batch), metric=pvs.COSINE, agg=pvs.AGG_MAX, rrf_k=5, weight=1.0, descending=True),
               dict(index=f, query=_queries("f32", None, batch, 64, 400 + batch), metric=pvs.L2, agg=pvs.AGG_AVG, rrf_k=10, weight=0.7, row_weights=w),
               dict(index=h, query=_queries("f16", None, batch, 96, 500 + batch), metric=pvs.L2, agg=pvs.AGG_AVG, rrf_k=2, weight=0.5)]
        _check(pvs, brs, k, [oh, of, oh], sample=(batch - 1,))
    h.close()
    f.close()


def test_order_keys_break_ties_of_duplicate_files(pvs):
    """Duplicate rows in different files tie on the fused score: the order keys (key DESC) decide, as in pvs_rrf_search."""
    a, oa, sa = _index(pvs, "i8runs", 120_000, 128, 41, dup_of=20_000)
    b, ob, sb = _index(pvs, "i8scatter", 120_000, 64, 42, dup_of=30_000)
    a.set_order_keys(np.random.default_rng(1).integers(0, 1000, 120_000).astype(np.int64))
    b.set_order_keys(np.random.default_rng(2).integers(0, 1000, 120_000).astype(np.int64))
    brs = [dict(index=a, query=_queries("i8", sa, 37, 128, 600), metric=pvs.COSINE, agg=pvs.AGG_MIN, rrf_k=5, weight=1.0),
           dict(index=b, query=_queries("i8", sb, 37, 64, 601), metric=pvs.L2, agg=pvs.AGG_MIN, rrf_k=5, weight=1.0)]
    _check(pvs, brs, 20)
    a.close()
    b.close()


def test_mixed_fusion_paths_in_one_batch_and_forced_full_ranking(pvs):
    """A zero query under cosine (every distance NULL: every file ties, the full ranking) among ordinary queries: each page is still
    its single call's, and the batch reports path 2.  Then the whole batch with the full ranking forced."""
    a, oa, sa = _index(pvs, "i8runs", 150_000, 128, 51)
    b, ob, sb = _index(pvs, "i8runs", 150_000, 64, 52)
    qa, qb = _queries("i8", sa, 9, 128, 700), _queries("i8", sb, 9, 64, 701)
    qa[4] = 0
    qb[4] = 0
    brs = [dict(index=a, query=qa, metric=pvs.COSINE, agg=pvs.AGG_MIN, rrf_k=5, weight=1.0),
           dict(index=b, query=qb, metric=pvs.COSINE, agg=pvs.AGG_MIN, rrf_k=10, weight=0.7)]
    _check(pvs, brs, 10, [oa, ob], sample=(4,), expect_path=2)
    _check(pvs, [dict(x, query=x["query"][:4]) for x in brs], 10, expect_path=1)
    pvs.debug_set("rrf_full", 1)
    try:
        _check(pvs, brs, 10, expect_path=2)
    finally:
        pvs.debug_set("rrf_full", 0)
    a.close()
    b.close()


def test_int8_l2_beyond_the_closed_form_range(pvs):
    """Rows at -128 against queries at +127: L2 sums past 2^24 raise the scorer's out-of-range flag and the chunk is scored again in
    order, as the single call's scorer does."""
    n, dim = 80_000, 512
    rng = np.random.default_rng(61)
    codes = rng.integers(-20, 20, (n, dim)).astype(np.int8)
    codes[::7] = -128
    grp = np.arange(n, dtype=np.int64) // 2
    ix = pvs.VectorIndex(pvs.I8, dim)
    ix.set_scale(0.01)
    ix.add(codes, group_ids=grp)
    q = rng.integers(-20, 20, (6, dim)).astype(np.int8)
    q[1] = 127
    q[4] = 127
    brs = [dict(index=ix, query=q, metric=pvs.L2, agg=pvs.AGG_MAX, rrf_k=5, weight=1.0)]
    _check(pvs, brs, 10, [dict(dtype=orc.I8, corpus=codes, groups=grp)], sample=(1, 2))
    ix.close()


def test_fold_path_out_of_range_flag(pvs):
    """Two queries (the <= 4-query fold scorer), one of them at +127 against rows at -128: the fold raises the flag, the pair is scored
    again in order."""
    n, dim = 60_000, 512
    rng = np.random.default_rng(62)
    codes = rng.integers(-20, 20, (n, dim)).astype(np.int8)
    codes[::5] = -128
    grp = np.arange(n, dtype=np.int64) // 2
    ix = pvs.VectorIndex(pvs.I8, dim)
    ix.set_scale(0.01)
    ix.add(codes, group_ids=grp)
    q = rng.integers(-20, 20, (2, dim)).astype(np.int8)
    q[0] = 127
    _check(pvs, [dict(index=ix, query=q, metric=pvs.L2, agg=pvs.AGG_MIN, rrf_k=5, weight=1.0)], 10,
           [dict(dtype=orc.I8, corpus=codes, groups=grp)], sample=(0, 1))
    ix.close()


def test_chunks_below_32_queries_under_the_matrix_cap(pvs):
    """17M rows: the [n][nq] matrix cap (2 GiB) allows 31 queries per pass, so a batch of 33 runs as 31 + 2 (the second through the
    fold scorer) — every page still its single call's."""
    from panoptikon_amd import _lib as L

    n, dim, chunk = 17_000_000, 64, 1_000_000
    lib = pvs.lib()
    ix = pvs.VectorIndex(pvs.I8, dim, capacity_rows=n)
    ix.set_scale(0.02)
    stage = pvs.DeviceBuffer(chunk * dim * 4)
    for off in range(0, n, chunk):
        m = min(chunk, n - off)
        L.check(lib.pvs_synth_rows_f32(0, 73, off, m, dim, stage.ptr))
        g = np.arange(off, off + m, dtype=np.int64) // 3
        L.check(lib.pvs_index_add_f32(ix._h, stage.ptr, m, None, g.ctypes.data, L.DEVICE))
    stage.free()
    q = orc.synth_rows(74, 0, 33, dim)
    _check(pvs, [dict(index=ix, query=q, metric=pvs.COSINE, agg=pvs.AGG_MIN, rrf_k=5, weight=1.0)], 20)
    ix.close()


def test_scale_two_2M_row_branches_batch_40(pvs):
    n = 2_000_000
    a, oa, sa = _index(pvs, "i8runs", n, 512, 71, rows_per_group=3)
    b, ob, sb = _index(pvs, "i8runs", n, 1024, 72, rows_per_group=3)
    brs = [dict(index=a, query=_queries("i8", sa, 40, 512, 800), metric=pvs.COSINE, agg=pvs.AGG_MIN, rrf_k=5, weight=1.0),
           dict(index=b, query=_queries("i8", sb, 40, 1024, 801), metric=pvs.L2, agg=pvs.AGG_MIN, rrf_k=10, weight=0.7)]
    g, s, c = pvs.rrf_search_batch(brs, 50)
    assert (c == 50).all()
    for j in range(8):
        g1, s1 = pvs.rrf_search([dict(x, query=x["query"][j]) for x in brs], 50)
        assert np.array_equal(g[j], g1) and np.array_equal(s[j].view(np.uint64), s1.view(np.uint64)), j
    for j in (0, 39):
        ora = [dict(oa, query=brs[0]["query"][j], metric=orc.COSINE, agg=orc.AGG_MIN, rrf_k=5, weight=1.0),
               dict(ob, query=brs[1]["query"][j], metric=orc.L2, agg=orc.AGG_MIN, rrf_k=10, weight=0.7)]
        eg, es = orc.rrf_search(ora, 50)
        assert np.array_equal(g[j], eg) and np.array_equal(s[j].view(np.uint64), es.view(np.uint64)), f"query {j} vs the oracle"
    a.close()
    b.close()


def test_edge_cases_match_the_single_call(pvs):
    from panoptikon_amd import _lib as L
    from panoptikon_amd.host import _branch_struct

    a, oa, sa = _index(pvs, "i8runs", 5_000, 64, 81)
    empty = pvs.VectorIndex(pvs.I8, 32)
    empty.set_scale(0.01)
    brs = [dict(index=a, query=_queries("i8", sa, 6, 64, 900), metric=pvs.COSINE, agg=pvs.AGG_MIN, rrf_k=5, weight=1.0),
           dict(index=empty, query=np.zeros((6, 32), np.int8), metric=pvs.L2, agg=pvs.AGG_MIN, rrf_k=5, weight=1.0)]
    _check(pvs, brs, 10)
    # batch = 0: PVS_OK, nothing written
    lib = pvs.lib()
    keep = []
    arr = (L.RrfBranch * 9)()
    for i in range(9):
        arr[i] = _branch_struct(brs[0], keep)
    og = np.full(10, 7, np.int64)
    ov = np.full(10, 7.0)
    oc = np.full(1, 7, np.uint32)
    P = lambda x: x.ctypes.data_as(C.c_void_p)
    assert lib.pvs_rrf_search_batch(C.byref(arr), 1, 0, 10, P(og), P(ov), P(oc)) == 0
    assert (og == 7).all() and (ov == 7.0).all() and oc[0] == 7
    # invalid arguments: the single call's status
    cnt = C.c_uint32()

    def both(nb, k, arr_):
        single = lib.pvs_rrf_search(C.byref(arr_), nb, k, P(og), P(ov), C.byref(cnt))
        batch = lib.pvs_rrf_search_batch(C.byref(arr_), nb, 2, k, P(og), P(ov), P(oc))
        return single, batch

    s1, b1 = both(1, 0, arr)  # k = 0
    assert s1 != 0 and s1 == b1
    s1, b1 = both(9, 10, arr)  # 9 branches
    assert s1 != 0 and s1 == b1
    nullq = (L.RrfBranch * 1)()
    nullq[0] = _branch_struct(brs[0], keep)
    nullq[0].query = None
    s1, b1 = both(1, 10, nullq)
    assert s1 != 0 and s1 == b1
    if pvs.device_count() >= 2:
        other = pvs.VectorIndex(pvs.I8, 64, device=1)
        other.set_scale(sa)
        other.add(oa["corpus"][:100], group_ids=oa["groups"][:100])
        two = (L.RrfBranch * 2)()
        two[0] = _branch_struct(brs[0], keep)
        two[1] = _branch_struct(dict(brs[0], index=other), keep)
        s1, b1 = both(2, 10, two)
        assert s1 != 0 and s1 == b1
        other.close()
    a.close()
    empty.close()


def test_two_shard_branches_answer_per_query(pvs):
    a, oa, sa = _index(pvs, "i8runs", 60_000, 64, 91, devices=[0, 0])
    b, ob, _ = _index(pvs, "f16", 40_000, 32, 92, devices=[0, 0])
    brs = [dict(index=a, query=_queries("i8", sa, 5, 64, 950), metric=pvs.COSINE, agg=pvs.AGG_MIN, rrf_k=5, weight=1.0),
           dict(index=b, query=_queries("f16", None, 5, 32, 951), metric=pvs.L2, agg=pvs.AGG_AVG, rrf_k=10, weight=0.7)]
    _check(pvs, brs, 20, [oa, ob], sample=(3,))
    a.close()
    b.close()
