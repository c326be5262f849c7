"""Held tickets of pvs_search_device (csrc/pvs_search_device.hip): two stream-ordered int8 searches on one index share one corpus
pass.  Every page must be the one the same batch gets alone (joining off, pvs_debug "join_us" = 0) and the oracle's, in the
buffers of the caller that asked for it; held tickets are launched when waited on, by the window, by a search that cannot join
and by a writer."""
import threading
import time

import numpy as np
import pytest

import oracle as orc

pytestmark = pytest.mark.gpu

DIM = 768
N = 20000
K = 50


@pytest.fixture(scope="module")
def pvs():
    import panoptikon_amd as p

    if p.device_count() < 1:
        pytest.fail("no gfx950 device visible: the gpu tests need an MI355X")
    return p


class knob:
    """pvs_debug_set for the duration of a block; the previous value comes back afterwards."""

    def __init__(self, pvs, key, value):
        self.pvs, self.key, self.value = pvs, key, value

    def __enter__(self):
        self.old = self.pvs.debug_get(self.key)
        self.pvs.debug_set(self.key, self.value)

    def __exit__(self, *exc):
        self.pvs.debug_set(self.key, self.old)


def counters(pvs):
    return {k: pvs.debug_get(k) for k in ("joined_passes", "joined_queries", "join_alone_passes", "join_window_launches")}


def delta(pvs, before):
    now = counters(pvs)
    return {k: now[k] - before[k] for k in now}


@pytest.fixture(scope="module")
def corpus(pvs):
    rows = orc.synth_rows(41, 0, N, DIM)
    scale = orc.compute_int8_scale(rows)
    ix = pvs.VectorIndex(pvs.I8, DIM)
    ix.set_scale(scale)
    ix.add_f32(rows)
    yield rows, scale, ix
    ix.close()


class Batch:
    """f32 queries in device memory and the three output buffers of their page."""

    def __init__(self, pvs, q, k=K):
        self.q, self.b, self.k = q, q.shape[0], k
        self.dq = pvs.DeviceBuffer.from_numpy(q)
        self.oi = pvs.DeviceBuffer(self.b * k * 8)
        self.od = pvs.DeviceBuffer(self.b * k * 4)
        self.oc = pvs.DeviceBuffer(self.b * 4)

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


def oracle_page(rows, scale, q, k, metric, ids=None):
    ei, ed = orc.search(orc.I8, metric, orc.quantize_int8(rows, scale), orc.quantize_int8(q, scale), k, ids=ids, threads=8)
    return ei, ed, np.full(q.shape[0], ei.shape[1], np.uint32)


def alone(pvs, ix, batch, metric=None):
    """The page of one batch with joining off."""
    with knob(pvs, "join_us", 0):
        ix.wait(batch.submit(pvs, ix, metric))
    return batch.page()


def test_pair_shares_one_pass_and_matches_alone_and_oracle(pvs, corpus):
    rows, scale, ix = corpus
    a = Batch(pvs, orc.synth_rows(0x10A, 0, 128, DIM))
    b = Batch(pvs, orc.synth_rows(0x10B, 0, 100, DIM))
    exp_a, exp_b = oracle_page(rows, scale, a.q, K, pvs.COSINE), oracle_page(rows, scale, b.q, K, pvs.COSINE)
    solo_a, solo_b = alone(pvs, ix, a), alone(pvs, ix, b)
    assert same(solo_a, exp_a) and same(solo_b, exp_b)
    st0, c0 = ix.stats(), counters(pvs)
    ix.set_profiling(True)
    ix.profile(reset=True)
    with knob(pvs, "join_us", 2_000_000):  # (a window far beyond the gap between the two calls: they must join)
        for first_waited in ("a", "b"):
            ta, tb = a.submit(pvs, ix), b.submit(pvs, ix)
            for t in ((ta, tb) if first_waited == "a" else (tb, ta)):
                ix.wait(t)
            assert same(a.page(), exp_a) and same(b.page(), exp_b)
    prof = ix.profile()
    ix.set_profiling(False)
    d, st = delta(pvs, c0), ix.stats()
    assert d["joined_passes"] == 2 and d["joined_queries"] == 2 * 228 and d["join_alone_passes"] == 0
    assert prof.scan_launches == 2, "one pass B per pair"
    # counters per search, as without joining
    assert st.searches - st0.searches == 4
    assert st.fast_queries - st0.fast_queries == 2 * 228 and st.dense_queries == st0.dense_queries


def test_pipelined_caller_pages_equal_joining_off(pvs, corpus):
    """bench.py's loop: two slots in flight, wait for the oldest, submit the next.  Same pages with and without joining."""
    rows, scale, ix = corpus
    bs = [Batch(pvs, orc.synth_rows(0x200 + i, 0, 128, DIM)) for i in range(4)]

    def run():
        pages, pending = [], []
        for i in range(8):
            if len(pending) >= 2:
                j, t = pending.pop(0)
                ix.wait(t)
                pages.append(bs[j % 4].page())
            pending.append((i, bs[i % 4].submit(pvs, ix)))
        while pending:
            j, t = pending.pop(0)
            ix.wait(t)
            pages.append(bs[j % 4].page())
        return pages

    with knob(pvs, "join_us", 0):
        off = run()
    c0 = counters(pvs)
    with knob(pvs, "join_us", 2_000_000):
        on = run()
    assert delta(pvs, c0)["joined_passes"] >= 3
    for x, y in zip(off, on):
        assert same(x, y)
    assert same(on[0], oracle_page(rows, scale, bs[0].q, K, pvs.COSINE))


def test_held_ticket_waited_alone_and_left_to_the_window(pvs, corpus):
    rows, scale, ix = corpus
    a = Batch(pvs, orc.synth_rows(0x30A, 0, 64, DIM))
    exp = oracle_page(rows, scale, a.q, K, pvs.COSINE)
    c0 = counters(pvs)
    with knob(pvs, "join_us", 2_000_000):  # waited at once: launched by pvs_wait, long before the window
        t0 = time.perf_counter()
        ix.wait(a.submit(pvs, ix))
        assert time.perf_counter() - t0 < 1.0
    assert same(a.page(), exp)
    d = delta(pvs, c0)
    assert d["join_alone_passes"] == 1 and d["join_window_launches"] == 0 and d["joined_passes"] == 0
    c0 = counters(pvs)
    with knob(pvs, "join_us", 20_000):  # nobody waits: the window launches it
        t = a.submit(pvs, ix)
        deadline = time.time() + 10
        while counters(pvs)["join_window_launches"] == c0["join_window_launches"] and time.time() < deadline:
            time.sleep(0.01)
        assert counters(pvs)["join_window_launches"] == c0["join_window_launches"] + 1, "the window did not launch the held search"
        ix.wait(t)
    assert same(a.page(), exp)
    # pvs_sync launches and completes a held ticket as well
    with knob(pvs, "join_us", 2_000_000):
        a.submit(pvs, ix)
        ix.sync()
    assert same(a.page(), exp)


def test_incompatible_searches_do_not_join(pvs, corpus):
    rows, scale, ix = corpus
    a = Batch(pvs, orc.synth_rows(0x40A, 0, 64, DIM))
    b20 = Batch(pvs, orc.synth_rows(0x40B, 0, 64, DIM), k=20)
    b = Batch(pvs, orc.synth_rows(0x40B, 0, 64, DIM))
    big = Batch(pvs, orc.synth_rows(0x40C, 0, 200, DIM))
    exp_a = oracle_page(rows, scale, a.q, K, pvs.COSINE)
    with knob(pvs, "join_us", 2_000_000):
        c0 = counters(pvs)
        ta, tb = a.submit(pvs, ix), b20.submit(pvs, ix)  # other k
        ix.wait(tb)
        ix.wait(ta)
        assert same(a.page(), exp_a) and same(b20.page(), oracle_page(rows, scale, b20.q, 20, pvs.COSINE))
        ta, tb = a.submit(pvs, ix), b.submit(pvs, ix, pvs.L2)  # other metric
        ix.wait(ta)
        ix.wait(tb)
        assert same(a.page(), exp_a) and same(b.page(), oracle_page(rows, scale, b.q, K, pvs.L2))
        ta, tb = a.submit(pvs, ix), big.submit(pvs, ix)  # 200 queries: never held; the held one is launched first
        ix.wait(tb)
        ix.wait(ta)
        assert same(a.page(), exp_a) and same(big.page(), oracle_page(rows, scale, big.q, K, pvs.COSINE))
        d = delta(pvs, c0)
        assert d["joined_passes"] == 0 and d["join_alone_passes"] == 5
        # a masked search beside a held ticket: answered on its own, the held page unchanged
        c0 = counters(pvs)
        allowed = np.zeros(N, bool)
        allowed[::3] = True
        ta = a.submit(pvs, ix)
        mi, md, mc = ix.search_filtered(b.q, K, allowed)
        ix.wait(ta)
        assert same(a.page(), exp_a)
        ids = np.arange(N, dtype=np.int64)[allowed]
        assert same((mi, md, mc), oracle_page(rows[allowed], scale, b.q, K, pvs.COSINE, ids=ids))
        assert delta(pvs, c0)["joined_passes"] == 0


def test_fallback_queries_land_in_their_callers_buffers(pvs):
    """Queries pass C hands back (all-NULL zero queries; tie-heavy L2 pages over duplicated rows) inside a joined pair are answered
    at their own ticket's pvs_wait, into their own caller's buffers."""
    base = orc.synth_rows(51, 0, 3000, DIM)
    rows = np.concatenate([base, base[:1500], np.zeros((5, DIM), np.float32), base[:500], base[:500]])
    scale = orc.compute_int8_scale(rows)
    ix = pvs.VectorIndex(pvs.I8, DIM)
    ix.set_scale(scale)
    ix.add_f32(rows)
    qa = orc.synth_rows(0x50A, 0, 96, DIM)
    qb = np.concatenate([base[:40] * 0.5 + base[1:41] * 0.5, orc.synth_rows(0x50B, 0, 56, DIM)]).astype(np.float32)
    qa[[3, 50]] = 0.0
    qb[[7, 90]] = 0.0
    try:
        for metric in (pvs.COSINE, pvs.L2):
            a, b = Batch(pvs, qa, k=300), Batch(pvs, qb, k=300)
            st0 = ix.stats()
            solo_a, solo_b = alone(pvs, ix, a, metric), alone(pvs, ix, b, metric)
            st1 = ix.stats()
            solo_counts = (st1.fast_queries - st0.fast_queries, st1.dense_queries - st0.dense_queries)
            exp_b = oracle_page(rows, scale, qb, 300, metric)
            assert same(solo_b, exp_b)
            for x in (a, b):  # poison the outputs: the pair must write every word of both pages
                x.oi.free(), x.od.free(), x.oc.free()
                x.oi, x.od, x.oc = (pvs.DeviceBuffer.from_numpy(np.full(x.b * x.k, -7, np.int64)),
                                    pvs.DeviceBuffer.from_numpy(np.full(x.b * x.k, 3.0, np.float32)),
                                    pvs.DeviceBuffer.from_numpy(np.full(x.b, 999, np.uint32)))
            st0, c0 = ix.stats(), counters(pvs)
            with knob(pvs, "join_us", 2_000_000):
                ta, tb = a.submit(pvs, ix, metric), b.submit(pvs, ix, metric)
                ix.wait(tb)
                ix.wait(ta)
            assert delta(pvs, c0)["joined_passes"] == 1
            assert same(a.page(), solo_a) and same(b.page(), solo_b)
            st = ix.stats()
            assert (st.fast_queries - st0.fast_queries, st.dense_queries - st0.dense_queries) == solo_counts, "counted per search as alone" 
    finally:
        ix.close()


def test_writer_between_submit_and_wait(pvs):
    """remove_rows while held / joined tickets are in flight: every page is the oracle's over the index as it stood at some point
    inside its call's window (a writer completes the searches in flight before it changes a row)."""
    rows = orc.synth_rows(61, 0, 12000, DIM)
    scale = orc.compute_int8_scale(rows)
    ix = pvs.VectorIndex(pvs.I8, DIM)
    ix.set_scale(scale)
    ix.add_f32(rows)
    ids = np.arange(len(rows), dtype=np.int64)
    dr0 = ids[200:260]  # removed in one thread between submit and wait
    drops = [ids[1000:1600], ids[5000:5300], ids[9000:9900]]  # removed by a writer thread beside a pipelined caller
    full = np.ones(len(rows), bool)
    states = [full.copy()]
    states[0][dr0] = False
    for dr in drops:
        s = states[-1].copy()
        s[dr] = False
        states.append(s)
    qs = [orc.synth_rows(0x600 + i, 0, 64, DIM) for i in range(2)]
    exp_full = [oracle_page(rows, scale, q, K, pvs.COSINE, ids=ids) for q in qs]
    exp = [[oracle_page(rows[s], scale, q, K, pvs.COSINE, ids=ids[s]) for s in states] for q in qs]
    bs = [Batch(pvs, q) for q in qs]
    done = [0]
    errors = []

    def writer():
        try:
            for dr in drops:
                time.sleep(0.02)
                assert ix.remove_rows(dr) == len(dr)
                done[0] += 1
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    try:
        with knob(pvs, "join_us", 2_000_000):
            # in one thread: submit, mutate, wait — the pages are the state before the removal
            ta, tb = bs[0].submit(pvs, ix), bs[1].submit(pvs, ix)  # joined
            tc_batch = Batch(pvs, qs[0])
            tc = tc_batch.submit(pvs, ix)  # held
            assert ix.remove_rows(dr0) == len(dr0)
            for t in (ta, tb, tc):
                ix.wait(t)
            assert same(bs[0].page(), exp_full[0]) and same(bs[1].page(), exp_full[1]) and same(tc_batch.page(), exp_full[0])
            # ... and the next pair sees the removal
            ta, tb = bs[0].submit(pvs, ix), bs[1].submit(pvs, ix)
            ix.wait(tb)
            ix.wait(ta)
            assert same(bs[0].page(), exp[0][0]) and same(bs[1].page(), exp[1][0])
            # a writer thread beside a pipelined caller
            w = threading.Thread(target=writer)
            w.start()
            checked = 0
            while w.is_alive() or checked < 4:
                lo = done[0]
                ta, tb = bs[0].submit(pvs, ix), bs[1].submit(pvs, ix)
                ix.wait(ta)
                ix.wait(tb)
                hi = min(done[0] + 1, len(drops))  # (a removal may have taken effect before the writer counted it)
                for j in range(2):
                    page = bs[j].page()
                    assert any(same(page, exp[j][s]) for s in range(lo, hi + 1)), f"page {j} is no state in [{lo}, {hi}]"
                checked += 1
                if checked > 400:
                    break
            w.join()
            assert not errors, errors
    finally:
        ix.close()
