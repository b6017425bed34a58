"""The sampled streaming mode decided on the device (cooc_sampling_enable_device, sample_on="device"): every fired
window and the state after it against the pure-Python model (tests/_sampled_model.py) and, byte for byte, against
a host-mode context fed the same log; the draw keyed by the user's id where the state is indexed by its slot; the
sizes at which the flat kernels, the scan tile, the wave-sized steps and the per-user bitmap change shape; windows
that change nothing; the regrowth of the per-slot device state; determinism; the entry points a sampled context
refuses."""
import numpy as np
import pytest

import _sampled_model as sm
from test_gpu_sampled import _check_invariant, _check_window, _fire

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE
SST_SLOTS0 = 1024  # kSstSlots0 of cooc_sample_stream.h: the slots of a new context's per-slot device state


def _dev(pkg, **kw):
    return pkg.CooccurrenceCore(sample_seed=SEED, sample_on="device", **kw)


def _same_window(a, b):
    """every array of two fired windows, the heaps within their sizes (scores bit for bit, NaN == NaN)"""
    assert a.ts == b.ts and a.observed == b.observed
    for f in ("rows", "row_ptr", "cols", "exact", "v16", "rs_items", "rs_exact", "rs_v32", "topk_rows", "topk_sizes"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert a.topk_values.shape == b.topk_values.shape and a.topk_scores.shape == b.topk_scores.shape
    if a.topk_values.size:
        live = np.arange(a.topk_values.shape[1])[None, :] < a.topk_sizes[:, None]
        assert np.array_equal(a.topk_values[live], b.topk_values[live])
        assert np.array_equal(a.topk_scores[live], b.topk_scores[live], equal_nan=True)
        assert np.array_equal(np.signbit(a.topk_scores[live]), np.signbit(b.topk_scores[live]))


def _same_state(a, b, users):
    assert a.sampling_counters() == b.sampling_counters()
    assert a.op_counters() == b.op_counters()
    assert a.last_window_runs() == b.last_window_runs()
    for x, y in zip(a.global_rowsums(), b.global_rowsums()):
        assert np.array_equal(x, y)
    assert a.global_observed() == b.global_observed()
    for u in users:
        (ha, ta), (hb, tb) = a.user_history(u), b.user_history(u)
        assert np.array_equal(ha, hb) and ta == tb, f"user {u}"


def _random_log(n_windows=6):
    """the log of test_gpu_sampled.py::test_random_log_many_users: 300 users, windows of 3,000 records, 211 items"""
    rng = np.random.default_rng(11)
    out = []
    for _ in range(n_windows):
        users = np.where(rng.random(3000) < 0.5, rng.integers(0, 20, 3000), rng.integers(0, 300, 3000))
        items = np.minimum(rng.zipf(1.2, 3000) - 1, 210)
        out.append(list(zip(users.tolist(), items.tolist())))
    return out


# ---- 1. model parity on the reference log
@pytest.mark.parametrize("kind", ["dense", "slabs", "large"])
def test_reference_log_every_window(pkg, oracle, kind):
    M, spread = (40_500, 40_500 // 24) if kind == "large" else (24, 1)
    model = sm.SampledModel(M, 20, 4, SEED)
    with _dev(pkg, n_items=M, topk=5, user_cut=4, item_cut=20, planner="general" if kind == "slabs" else "auto") as core:
        for wi, recs in enumerate(sm.reference_log(spread=spread)):
            w, mw = _fire(core, wi, recs), model.window(recs)
            _check_window(core, model, w, mw, oracle, 5, rows_to_read=None if M == 24 else [0, M - 1])
            _check_invariant(core, model, oracle)
        c = core.sampling_counters()
    assert (c["fills"], c["replacements"], c["feedbacks"], c["item_cut_rejections"]) == (48, 55, 137, 240)


# ---- 2. host mode against device mode, byte for byte
@pytest.mark.parametrize("planner", ["auto", "general"])
def test_host_and_device_modes_agree(pkg, planner):
    kw = dict(n_items=211, topk=4, user_cut=40, item_cut=60, sample_seed=SEED, planner=planner)
    with pkg.CooccurrenceCore(sample_on="host", **kw) as host, pkg.CooccurrenceCore(sample_on="device", **kw) as dev:
        for wi, recs in enumerate(_random_log()):
            _same_window(_fire(host, wi, recs), _fire(dev, wi, recs))
            _same_state(host, dev, range(300))
        c = host.sampling_counters()
        assert min(c["fills"], c["replacements"], c["feedbacks"], c["item_cut_rejections"]) >= 100
        for a in range(0, 211, 7):
            for x, y in zip(host.global_row(a), dev.global_row(a)):
                assert np.array_equal(x, y)


# ---- 3. the draw is keyed by the user's id, the state by its slot
def test_draw_keyed_by_user_id(pkg, oracle):
    """descending ids (the slot of an id is its first-seen index) and one id on the hash-map path of slot_for"""
    ids = [(1 << 26) + 5] + list(range(900, 0, -100))
    rng = np.random.default_rng(5)
    M, cut = 24, 3
    windows = [[(ids[int(s)], int(i)) for s, i in zip(rng.integers(0, len(ids), 80), rng.integers(0, M, 80))]
               for _ in range(4)]
    model = sm.SampledModel(M, 32767, cut, SEED)
    by_slot = sm.SampledModel(M, 32767, cut, SEED)  # what a draw keyed by the first-seen index would decide
    slot_of: dict = {}
    differs = False
    with _dev(pkg, n_items=M, topk=3, user_cut=cut, item_cut=32767) as core:
        for wi, recs in enumerate(windows):
            w, mw = _fire(core, wi, recs), model.window(recs)
            sw = by_slot.window([(slot_of.setdefault(u, len(slot_of)), i) for u, i in recs])
            differs |= mw.decisions != sw.decisions
            _check_window(core, model, w, mw, oracle, 3)
        assert model.replacements >= 20 and differs
        assert [slot_of[u] for u in ids] != ids
        _check_invariant(core, model, oracle)


# ---- 4. kernel-boundary sizes
@pytest.mark.parametrize("sizes", [(255, 256, 257), (4095, 4096, 4097)])
def test_window_sizes_around_the_block_and_the_scan_tile(pkg, oracle, sizes):
    """windows one below, at and one above the 256-thread flat kernels' block and the scans' 4,096-element tile"""
    rng = np.random.default_rng(sizes[0])
    M, cut = 48, 5
    model = sm.SampledModel(M, 150, cut, SEED)
    with _dev(pkg, n_items=M, topk=3, user_cut=cut, item_cut=150) as core:
        for wi, n in enumerate(sizes):
            recs = list(zip(rng.integers(0, 90, n).tolist(), np.minimum(rng.zipf(1.3, n) - 1, M - 1).tolist()))
            w, mw = _fire(core, wi, recs), model.window(recs)
            _check_window(core, model, w, mw, oracle, 3)
        c = model.counters()
        assert min(c["fills"], c["replacements"], c["feedbacks"], c["item_cut_rejections"]) > 0
        _check_invariant(core, model, oracle)


@pytest.mark.parametrize("n_rep", [63, 64, 65])
def test_one_user_many_replacements(pkg, oracle, n_rep):
    """one user with 63, 64 and 65 replacements in one window (the wave-sized steps of the per-user kernel), in a
    reservoir of 65 slots, among other users' records"""
    M, cut, u = 61, 65, 7
    fill = [(u, (3 * s) % M) for s in range(cut)] + [(v, v % M) for v in range(20, 30)]
    recs, reps, total = [], 0, cut
    while reps < n_rep:  # the user's records until the model's draw has replaced n_rep times
        total += 1
        reps += sm.draw(SEED, u, total) < cut
        recs.append((u, (5 * total) % M))
        recs.append((20 + total % 10, total % M))  # (interleaved: the user's run is gathered by the sort)
    model = sm.SampledModel(M, 32767, cut, SEED)
    with _dev(pkg, n_items=M, topk=3, user_cut=cut, item_cut=32767) as core:
        for wi, r in enumerate((fill, recs)):
            w, mw = _fire(core, wi, r), model.window(r)
            _check_window(core, model, w, mw, oracle, 3)
        assert sum(1 for (x, _), d in zip(recs, mw.decisions) if x == u and d[0] == "k") == n_rep
        assert core.last_window_runs() == 2
        _check_invariant(core, model, oracle)


@pytest.mark.parametrize("cut", [1, 2, 65])
def test_slot_edges(pkg, oracle, cut):
    """a slot filled and replaced within one window; a slot of that window replaced twice; a slot that existed before
    the window replaced twice (two replacements, one distinct slot: the minus list's size); user_cut of 1 and 65;
    the user ids are found with the model's draw"""
    M = 37
    d = lambda u, t: sm.draw(SEED, u, t)  # noqa: E731
    fresh = sm.find_user_total(SEED, cut + 1, lambda k: k < cut)
    twice_new = fresh + 1  # fills and two replacements of one slot, all in one window
    while not (d(twice_new, cut + 1) < cut and d(twice_new, cut + 1) == d(twice_new, cut + 2)):
        twice_new += 1
    twice_old = twice_new + 1  # two replacements of one slot that an earlier window filled
    while not (d(twice_old, cut + 1) < cut and d(twice_old, cut + 1) == d(twice_old, cut + 2)):
        twice_old += 1
    item = lambda u, s: (7 * s + 3 * u) % M  # noqa: E731
    windows = [
        [(twice_old, item(twice_old, s)) for s in range(cut)],
        [(fresh, item(fresh, s)) for s in range(cut)] + [(twice_old, 30), (fresh, 35)]
        + [(twice_new, item(twice_new, s)) for s in range(cut)] + [(twice_new, 36), (twice_old, 31), (twice_new, 29)],
    ]
    model = sm.SampledModel(M, 32767, cut, SEED)
    with _dev(pkg, n_items=M, topk=3, user_cut=cut, item_cut=32767) as core:
        for wi, recs in enumerate(windows):
            w, mw = _fire(core, wi, recs), model.window(recs)
            _check_window(core, model, w, mw, oracle, 3)
        k_old, k_new = d(twice_old, cut + 1), d(twice_new, cut + 1)
        assert mw.decisions[cut:cut + 2] == [f"k{k_old}", f"k{d(fresh, cut + 1)}"]
        assert mw.decisions[-3:] == [f"k{k_new}", f"k{k_old}", f"k{k_new}"] and mw.twice == 4
        assert model.H[twice_old][k_old] == 31 and model.H[twice_new][k_new] == 29 and core.last_window_runs() == 2
        _check_invariant(core, model, oracle)


# ---- 5. degenerate windows
def test_degenerate_windows(pkg, oracle):
    """a window of one record; a window whose every record the item cut rejects (empty, but rejections and totals
    advance); a window whose sampled records all feed back (no changed user; the item counters go back down, which
    the next window's cut shows)"""
    M, cut, icut = 16, 2, 4
    idle = sm.find_user_total(SEED, cut + 1, lambda k: k >= cut, 50)
    model = sm.SampledModel(M, icut, cut, SEED)
    windows = [
        [(1, 3)],                                            # one record
        [(2, 3), (3, 3), (4, 3), (idle, 1), (idle, 2)],      # item 3 reaches the cut; idle's reservoir fills
        [(5, 3), (6, 3), (2, 3)],                            # every record rejected
        [(idle, 5)],                                         # sampled, then fed back: count[5] is 0 again
        [(10 + k, 5) for k in range(icut + 1)],              # so item 5 takes item_cut records, and one is rejected
    ]
    want = ["f", "fffff", "rrr", "b", "f" * icut + "r"]
    with _dev(pkg, n_items=M, topk=0, user_cut=cut, item_cut=icut) as core:
        for wi, recs in enumerate(windows):
            before = core.sampling_counters()
            w, mw = _fire(core, wi, recs), model.window(recs)
            assert "".join(mw.decisions) == want[wi]
            _check_window(core, model, w, mw, oracle, 0)
            if wi in (2, 3):
                assert len(w.rows) == 0 and len(w.cols) == 0 and w.observed == 0 and core.last_window_runs() == 0
                after = core.sampling_counters()
                assert after["item_cut_rejections"] - before["item_cut_rejections"] == (3 if wi == 2 else 0)
                assert after["feedbacks"] - before["feedbacks"] == (1 if wi == 3 else 0)
                assert after["item_counter_sum"] == before["item_counter_sum"]
        for u, total, held in ((5, 1, 0), (6, 1, 0), (2, 2, 1), (idle, cut + 1, cut)):  # (5, 6: no reservoir)
            items, t = core.user_history(u)
            assert (t, items.size) == (total, held)
        _check_invariant(core, model, oracle)


# ---- 6. the per-slot device state grows
def test_slot_state_regrows(pkg, oracle):
    """eight windows of 600 new users each (and 100 records of earlier ones): the per-slot lengths and totals start
    at SST_SLOTS0 slots and are regrown by doubling; earlier users' lengths and totals survive"""
    rng = np.random.default_rng(2)
    M, cut = 32, 3
    model = sm.SampledModel(M, 32767, cut, SEED)
    cap, regrown = SST_SLOTS0, 0
    with _dev(pkg, n_items=M, topk=0, user_cut=cut, item_cut=32767) as core:
        for wi in range(8):
            new = rng.permutation(np.arange(600 * wi, 600 * (wi + 1)))
            old = rng.integers(0, 600 * wi, 100) if wi else np.zeros(0, np.int64)
            users = rng.permutation(np.concatenate([new, new[:150], old]))
            recs = list(zip(users.tolist(), rng.integers(0, M, len(users)).tolist()))
            w, mw = _fire(core, wi, recs), model.window(recs)
            if wi < 7:  # (the whole state is read once, after the last window)
                assert core.sampling_counters() == model.counters() and w.observed == mw.observed
                assert w.rs_exact.tolist() == [mw.rowsum[a] for a in sorted(mw.rowsum)]
            slots = len(model.total)
            while slots > cap:
                cap, regrown = max(slots, 2 * cap), regrown + 1
        assert regrown >= 2 and len(model.total) == 4800
        _check_window(core, model, w, mw, oracle, 0)  # every user's reservoir and total, every global row
        _check_invariant(core, model, oracle)


# ---- 7. determinism
def test_two_device_contexts_agree(pkg):
    kw = dict(n_items=211, topk=4, user_cut=40, item_cut=60)
    with _dev(pkg, **kw) as a, _dev(pkg, **kw) as b:
        for wi, recs in enumerate(_random_log(3)):
            _same_window(_fire(a, wi, recs), _fire(b, wi, recs))
        _same_state(a, b, range(300))


# ---- 8. what a device-mode context refuses
def test_refusals(pkg):
    from flink_cooccurrence_amd import _lib
    from flink_cooccurrence_amd._lib import IllegalArgumentException, IllegalStateException

    L = _lib.load()
    with _dev(pkg, n_items=16, user_cut=3, item_cut=5) as core:
        for call in (core.snapshot, lambda: core.restore(b"\0" * 1024), lambda: core.restore_parts([b"\0" * 1024]),
                     lambda: core.comm_init(b"\0" * 128, 0, 1)):
            with pytest.raises(IllegalStateException, match="sampled"):
                call()
        assert L.cooc_comm_init_ops(core._h, 0, 1, _lib.CoocCommOps(), None) == _lib.COOC_ERR_STATE
        assert L.cooc_sampling_enable(core._h, 5, 1) == _lib.COOC_ERR_STATE  # a second enable of either kind
        assert L.cooc_sampling_enable_device(core._h, 5, 1) == _lib.COOC_ERR_STATE
    with pkg.CooccurrenceCore(n_items=16, user_cut=3, item_cut=5) as core:  # and on a host-mode context
        assert L.cooc_sampling_enable_device(core._h, 5, 1) == _lib.COOC_ERR_STATE
    with pytest.raises(IllegalStateException, match="user_cut"):
        _dev(pkg, n_items=16, user_cut=0, item_cut=5)
    with pytest.raises(IllegalArgumentException, match="item_cut"):
        _dev(pkg, n_items=16, user_cut=3, item_cut=32768)
    with pkg.CooccurrenceCore(n_items=16, user_cut=3) as core:
        assert L.cooc_sampling_enable_device(core._h, 0, 1) == _lib.COOC_ERR_ARG
        assert L.cooc_sampling_enable_device(core._h, 32768, 1) == _lib.COOC_ERR_ARG
        core.submit_batch(0, [1], [0, 1], [2])
        assert L.cooc_sampling_enable_device(core._h, 5, 1) == _lib.COOC_ERR_STATE  # after a submit
        core.finish_window(0)
        assert L.cooc_sampling_enable_device(core._h, 5, 1) == _lib.COOC_ERR_STATE
    with pkg.CooccurrenceCore(n_items=16, user_cut=3) as core:
        core.op_process_elements([1], [2], [5])
        assert L.cooc_sampling_enable_device(core._h, 5, 1) == _lib.COOC_ERR_STATE  # an element was processed
