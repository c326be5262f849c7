"""Per-ticket completion of a joined pass (csrc/pvs_search_device.hip, pvs_search.hip enqueue_fast_chunk): pass C of a held pair runs
as two launches, the held ticket's queries first with its done event behind them, the partner's beside them.  Every page must be
the one the same queries get as one 256-query batch, as two batches alone and from the oracle, with the light (side stream) and
the in-stream finaliser alike, when the partner comes late, when one ticket of the pair is handed to the fallbacks, and when the
held ticket's context is reused while the partner's part still runs."""
import numpy as np
import pytest

import oracle as orc

pytestmark = pytest.mark.gpu

DIM = 768
N = 24000
K = 40


@pytest.fixture(scope="module")
def pvs():
    import panoptikon_amd as p

    if p.device_count() < 1:
        pytest.fail("no gfx950 device visible: the gpu tests need an MI355X")
    return p


class knobs:
    """pvs_debug_set for the duration of a block; the previous values come back afterwards."""

    def __init__(self, pvs, **kv):
        self.pvs, self.kv = pvs, kv

    def __enter__(self):
        self.old = {k: self.pvs.debug_get(k) for k in self.kv}
        for k, v in self.kv.items():
            self.pvs.debug_set(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.pvs.debug_set(k, v)


def counters(pvs):
    return {k: pvs.debug_get(k) for k in ("joined_passes", "joined_queries", "join_alone_passes", "join_window_launches")}


def delta(pvs, before):
    now = counters(pvs)
    return {k: now[k] - before[k] for k in now}


class Batch:
    """f32 queries in device memory and the three output buffers of their page (poisoned: the search must write every word)."""

    def __init__(self, pvs, q, k=K):
        self.q, self.b, self.k = q, q.shape[0], k
        self.dq = pvs.DeviceBuffer.from_numpy(q)
        self.oi = pvs.DeviceBuffer.from_numpy(np.full(self.b * k, -7, np.int64))
        self.od = pvs.DeviceBuffer.from_numpy(np.full(self.b * k, 3.0, np.float32))
        self.oc = pvs.DeviceBuffer.from_numpy(np.full(self.b, 999, np.uint32))

    def submit(self, pvs, ix, metric=None):
        return ix.search_device(self.dq, pvs._lib.F32, self.b, self.k, pvs.COSINE if metric is None else metric, self.oi, self.od, self.oc)

    def page(self):
        return (self.oi.to_numpy(np.int64, (self.b, self.k)), self.od.to_numpy(np.float32, (self.b, self.k)),
                self.oc.to_numpy(np.uint32, (self.b,)))


def same(a, b):
    """Two pages (ids, distances, counts) are identical: ids and counts exactly, distances bit for bit (NULL = NaN alike)."""
    ai, ad, ac = a
    bi, bd, bc = b
    if not np.array_equal(ac, bc):
        return False
    for q in range(len(ac)):
        c = int(ac[q])
        if not np.array_equal(ai[q, :c], bi[q, :c]):
            return False
        x, y = ad[q, :c], bd[q, :c]
        if not (np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(x[~np.isnan(x)].view(np.uint32), y[~np.isnan(y)].view(np.uint32))):
            return False
    return True


def rows_of(page, lo, hi):
    i, d, c = page
    return i[lo:hi], d[lo:hi], c[lo:hi]


def oracle_page(rows, scale, q, k, metric):
    ei, ed = orc.search(orc.I8, metric, orc.quantize_int8(rows, scale), orc.quantize_int8(q, scale), k, threads=8)
    return ei, ed, np.full(q.shape[0], ei.shape[1], np.uint32)


def alone(pvs, ix, batch, metric=None):
    with knobs(pvs, join_us=0):
        ix.wait(batch.submit(pvs, ix, metric))
    return batch.page()


@pytest.fixture(scope="module")
def corpus(pvs):
    rows = orc.synth_rows(71, 0, N, DIM)
    scale = orc.compute_int8_scale(rows)
    ix = pvs.VectorIndex(pvs.I8, DIM)
    ix.set_scale(scale)
    ix.add_f32(rows)
    yield rows, scale, ix
    ix.close()


FINALIZERS = {"side": {}, "in_stream": {"no_side_finalize": 1}, "light_everywhere": {"force_light_finalize": 1},
              "no_light": {"no_light_finalize": 1}}


@pytest.mark.parametrize("fin", sorted(FINALIZERS))
def test_pair_pages_equal_one_batch_and_each_alone(pvs, corpus, fin):
    rows, scale, ix = corpus
    q = orc.synth_rows(0x7A0, 0, 256, DIM)
    whole, a, b = Batch(pvs, q), Batch(pvs, q[:128].copy()), Batch(pvs, q[128:].copy())
    exp = oracle_page(rows, scale, q, K, pvs.COSINE)
    with knobs(pvs, **FINALIZERS[fin]):
        one = alone(pvs, ix, whole)  # (256 queries: one pass, never held)
        solo_a, solo_b = alone(pvs, ix, a), alone(pvs, ix, b)
        assert same(one, exp)
        assert same(solo_a, rows_of(one, 0, 128)) and same(solo_b, rows_of(one, 128, 256))
        for first_waited in ("held", "partner"):
            a2, b2 = Batch(pvs, a.q), Batch(pvs, b.q)
            c0 = counters(pvs)
            with knobs(pvs, join_us=2_000_000):
                ta, tb = a2.submit(pvs, ix), b2.submit(pvs, ix)
                for t in ((ta, tb) if first_waited == "held" else (tb, ta)):
                    ix.wait(t)
            assert delta(pvs, c0)["joined_passes"] == 1
            assert same(a2.page(), solo_a) and same(b2.page(), solo_b)


@pytest.mark.parametrize("fin", sorted(FINALIZERS))
def test_pipelined_pairs_reuse_the_held_context(pvs, corpus, fin):
    """bench.py's loop (wait for the oldest, submit the next): the next held search takes the context whose partner part of pass C
    may still be running.  Every page equals its batch alone."""
    rows, scale, ix = corpus
    qs = [orc.synth_rows(0x7B0 + i, 0, 128, DIM) for i in range(6)]
    with knobs(pvs, **FINALIZERS[fin]):
        solo = [alone(pvs, ix, Batch(pvs, q)) for q in qs]
        bs = [Batch(pvs, q) for q in qs]
        c0 = counters(pvs)
        with knobs(pvs, join_us=2_000_000):
            pending, got = [], {}
            for i in range(18):
                if len(pending) >= 2:
                    j, t = pending.pop(0)
                    ix.wait(t)
                    got[j] = bs[j % 6].page()
                    assert same(got[j], solo[j % 6]), f"search {j}"
                    bs[j % 6] = Batch(pvs, qs[j % 6])
                pending.append((i, bs[i % 6].submit(pvs, ix)))
            for j, t in pending:
                ix.wait(t)
                assert same(bs[j % 6].page(), solo[j % 6]), f"search {j}"
        assert delta(pvs, c0)["joined_passes"] >= 8


def test_partner_arriving_after_the_window(pvs, corpus):
    """The window launches the held search alone; the search that comes after it is held in turn (no pair) and both pages are
    their batches' alone."""
    rows, scale, ix = corpus
    a, b = Batch(pvs, orc.synth_rows(0x7C0, 0, 128, DIM)), Batch(pvs, orc.synth_rows(0x7C1, 0, 128, DIM))
    solo_a, solo_b = alone(pvs, ix, a), alone(pvs, ix, b)
    a, b = Batch(pvs, a.q), Batch(pvs, b.q)
    c0 = counters(pvs)
    import time

    with knobs(pvs, join_us=20_000):
        ta = a.submit(pvs, ix)
        deadline = time.time() + 10
        while counters(pvs)["join_window_launches"] == c0["join_window_launches"] and time.time() < deadline:
            time.sleep(0.005)
        tb = b.submit(pvs, ix)
        ix.wait(ta)
        ix.wait(tb)
    d = delta(pvs, c0)
    assert d["join_window_launches"] >= 1 and d["joined_passes"] == 0
    assert same(a.page(), solo_a) and same(b.page(), solo_b)


def test_held_ticket_launched_alone_by_wait(pvs, corpus):
    rows, scale, ix = corpus
    a = Batch(pvs, orc.synth_rows(0x7D0, 0, 128, DIM))
    exp = oracle_page(rows, scale, a.q, K, pvs.COSINE)
    for fin in sorted(FINALIZERS):
        a = Batch(pvs, a.q)
        c0 = counters(pvs)
        with knobs(pvs, join_us=2_000_000, **FINALIZERS[fin]):
            ix.wait(a.submit(pvs, ix))
        d = delta(pvs, c0)
        assert d["join_alone_passes"] == 1 and d["joined_passes"] == 0
        assert same(a.page(), exp), fin


@pytest.mark.parametrize("fallback_in", ["held", "partner"])
def test_one_ticket_of_the_pair_takes_the_fallback(pvs, fallback_in):
    """One ticket's queries are handed back by pass C (all-NULL zero queries: flag 3; queries over duplicated rows: the dense path
    or the rerun), the other's are not.  The fallbacks run at their own ticket's pvs_wait, into its buffers, while the other's pass C
    part may still be running; the next pair reuses the contexts."""
    base = orc.synth_rows(81, 0, 4000, DIM)
    rows = np.concatenate([base, base[:2000], np.zeros((5, DIM), np.float32), base[:600], base[:600]])
    scale = orc.compute_int8_scale(rows)
    ix = pvs.VectorIndex(pvs.I8, DIM)
    ix.set_scale(scale)
    ix.add_f32(rows)
    hard = np.concatenate([base[:60] * 0.5 + base[1:61] * 0.5, orc.synth_rows(0x7E0, 0, 68, DIM)]).astype(np.float32)
    hard[[5, 77]] = 0.0
    easy = orc.synth_rows(0x7E1, 0, 128, DIM)
    qa, qb = (hard, easy) if fallback_in == "held" else (easy, hard)
    try:
        for metric in (pvs.COSINE, pvs.L2):
            a, b = Batch(pvs, qa, k=300), Batch(pvs, qb, k=300)
            solo_a, solo_b = alone(pvs, ix, a, metric), alone(pvs, ix, b, metric)
            assert same(solo_a if fallback_in == "held" else solo_b, oracle_page(rows, scale, hard, 300, metric))
            for first_waited in ("held", "partner"):
                a, b = Batch(pvs, qa, k=300), Batch(pvs, qb, k=300)
                c0 = counters(pvs)
                with knobs(pvs, join_us=2_000_000):
                    ta, tb = a.submit(pvs, ix, metric), b.submit(pvs, ix, metric)
                    for t in ((ta, tb) if first_waited == "held" else (tb, ta)):
                        ix.wait(t)
                    # the held context again at once (its fallbacks ran on it; the partner's part may still be running)
                    a3 = Batch(pvs, qa, k=300)
                    ix.wait(a3.submit(pvs, ix, metric))
                assert delta(pvs, c0)["joined_passes"] == 1
                assert same(a.page(), solo_a) and same(b.page(), solo_b) and same(a3.page(), solo_a)
    finally:
        ix.close()
