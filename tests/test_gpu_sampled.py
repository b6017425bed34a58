"""Sampled streaming mode on the GPU (cooc_sampling_enable: item cut, per-user reservoir with retractions) against
the pure-Python model of its contract (tests/_sampled_model.py): every window's signed delta rows, row sums, info
and counters, every reservoir and total, every global row and row sum, the heaps; the state invariant through
oracle.closed_form over the reservoirs read back; the list builder (k_sm_lists) and the signed combine (k_sd_*)
at their edges, with the slots dictated by searching user ids with the model's draw; wrapped int16 views; the
entry points that refuse a sampled context."""
import numpy as np
import pytest

import _sampled_model as sm
from _helpers import assert_windows_equal

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE
SD_BLOCK = 256  # kSdBlock of cooc_sampled.hip: threads (one entry each) per workgroup of the combine's flat kernels


def _fire(core, wi, recs):
    """window wi (1 s windows) through the operator mirror: its records in arrival order, then its watermark"""
    users = np.array([u for u, _ in recs], np.int32)
    items = np.array([i for _, i in recs], np.int32)
    assert core.op_process_elements(users, items, np.full(len(recs), wi * 1000 + 1, np.int64)) == 0
    out = core.op_process_watermark(wi * 1000 + 999)
    assert len(out) == 1 and out[0].ts == wi * 1000 + 999
    return out[0]


def _check_window(core, model, w, mw, oracle, topk, rows_to_read=None):
    """one fired window and the state after it against the model"""
    rows = mw.rows()
    got = {}
    got16 = {}
    for r, a in enumerate(w.rows.tolist()):
        s, e = int(w.row_ptr[r]), int(w.row_ptr[r + 1])
        assert np.all(np.diff(w.cols[s:e]) > 0), "delta columns not ascending"
        got[a] = dict(zip(w.cols[s:e].tolist(), w.exact[s:e].tolist()))
        got16[a] = dict(zip(w.cols[s:e].tolist(), w.v16[s:e].tolist()))
    assert got == rows, "signed delta rows differ"
    assert got16 == {a: {b: sm.i16(v) for b, v in r.items()} for a, r in rows.items()}, "cnt16 differs"
    assert w.rs_items.tolist() == sorted(rows)
    assert w.rs_exact.tolist() == [mw.rowsum[a] for a in sorted(rows)]
    assert w.rs_v32.tolist() == [sm.i32(mw.rowsum[a]) for a in sorted(rows)]
    assert w.observed == mw.observed
    assert len(w.rows) == len(rows) and len(w.cols) == sum(len(r) for r in rows.values())  # info.n_rows, info.nnz
    assert core.sampling_counters() == model.counters()
    oc = core.op_counters()
    assert oc["UserInteractionCounterObservedCooccurrences"] == model.observed_exact
    assert oc["RowSumProcessWindowRowSum"] == model.rowsum_acc
    assert oc["ItemRowRescorerRescoredItems"] == model.rescored
    assert oc["rescorer_observed"] == model.observed_rescorer
    assert core.global_observed() == (model.observed_exact, model.observed_rescorer)
    for u, H in model.H.items():
        items, total = core.user_history(u)
        assert items.tolist() == H and total == model.total[u], f"user {u}"
    for u, t in model.total.items():  # users whose every record was rejected: no reservoir, but a total
        if u not in model.H:
            items, total = core.user_history(u)
            assert items.size == 0 and total == t
    grows = model.global_rows()
    M = model.n_items
    for a in (range(M) if rows_to_read is None else sorted(set(rows_to_read) | set(model.rs))):
        cols, cnt, cnt16 = core.global_row(a)
        want = grows.get(a, {})
        assert dict(zip(cols.tolist(), cnt.tolist())) == want, f"global row {a}"
        assert cnt16.tolist() == [sm.i16(v) for v in want.values()]
    ex, v32 = core.global_rowsums()
    want_rs = np.zeros(M, np.int64)
    for a, v in model.rs.items():
        want_rs[a] = v
    assert np.array_equal(ex, want_rs) and np.array_equal(v32, model.rs32())
    if topk:
        rp, cols, c16 = [0], [], []
        for a in sorted(rows):
            r = grows.get(a, {})
            cols += list(r)
            c16 += [sm.i16(v) for v in r.values()]
            rp.append(len(cols))
        sizes, vals, scores = oracle.rows_topk(sorted(rows), rp, cols, np.array(c16, np.int16), model.rs32(),
                                               model.observed_rescorer, topk)
        assert w.topk_rows.tolist() == sorted(rows)
        assert np.array_equal(w.topk_sizes, sizes)
        for r in range(len(sizes)):
            n = int(sizes[r])
            assert np.array_equal(w.topk_values[r, :n], vals[r, :n]), f"heap of row {w.topk_rows[r]}"
            assert np.array_equal(w.topk_scores[r, :n], scores[r, :n], equal_nan=True), f"scores of row {w.topk_rows[r]}"


def _check_invariant(core, model, oracle):
    """the draw aside: the global rows and row sums are the pair counts over the reservoirs read back"""
    users = sorted(model.total)
    hist = [core.user_history(u)[0] for u in users]
    assert all(len(h) <= model.user_cut for h in hist)
    up = np.concatenate([[0], np.cumsum([len(h) for h in hist])]).astype(np.int64)
    items = np.concatenate(hist + [np.zeros(0, np.int32)]).astype(np.int32)
    rp, cols, data, rowsums, _ = oracle.closed_form(up, items, model.n_items)
    ex, _ = core.global_rowsums()
    assert np.array_equal(ex, rowsums)
    for a in np.flatnonzero(np.diff(rp)).tolist() + [0, model.n_items - 1]:
        c, n, _ = core.global_row(a)
        assert np.array_equal(c, cols[rp[a]:rp[a + 1]]) and np.array_equal(n.astype(np.int64), data[rp[a]:rp[a + 1]])


@pytest.mark.parametrize("kind", ["dense", "slabs", "large"])
def test_reference_log_every_window(pkg, oracle, kind):
    """the reference log (48 fills, 55 replacements, 137 feedbacks, 240 item-cut rejections; 14 slots changed
    twice within a window, 20 zero-net delta keys) on the default planner (dense global rows), with
    planner="general" (row slabs) and at n_items = 40,500 with the item ids spread over the range"""
    M, spread = (40_500, 40_500 // 24) if kind == "large" else (24, 1)
    windows = sm.reference_log(spread=spread)
    model = sm.SampledModel(M, 20, 4, SEED)
    twice = zero = 0
    with pkg.CooccurrenceCore(n_items=M, topk=5, user_cut=4, item_cut=20, sample_seed=SEED,
                              planner="general" if kind == "slabs" else "auto") as core:
        for wi, recs in enumerate(windows):
            w = _fire(core, wi, recs)
            mw = model.window(recs)
            twice += mw.twice
            zero += mw.zero_nets
            _check_window(core, model, w, mw, oracle, 5, rows_to_read=None if M == 24 else [0, M - 1])
            _check_invariant(core, model, oracle)
        c = core.sampling_counters()
    assert (c["fills"], c["replacements"], c["feedbacks"], c["item_cut_rejections"]) == (48, 55, 137, 240)
    assert (twice, zero) == (14, 20)


def test_no_replacement_equals_the_fill_path(pkg, oracle):
    """item_cut = 32767 and no user beyond user_cut: every output equals OracleStream(user_cut=...), and no window
    runs the minus pass"""
    rng = np.random.default_rng(3)
    M, cut = 31, 6
    ref = oracle.OracleStream(1000, topk=4, user_cut=cut)
    seen: dict = {}
    with pkg.CooccurrenceCore(n_items=M, topk=4, user_cut=cut, item_cut=32767, sample_seed=SEED) as core:
        for wi in range(5):
            recs = []
            for _ in range(40):
                u = int(rng.integers(0, 30))
                if seen.get(u, 0) < cut:
                    seen[u] = seen.get(u, 0) + 1
                    recs.append((u, int(rng.integers(0, M))))
            users, items = np.array([r[0] for r in recs], np.int32), np.array([r[1] for r in recs], np.int32)
            ts = np.full(len(recs), wi * 1000 + 1, np.int64)
            ref.process_elements(users, items, ts)
            core.op_process_elements(users, items, ts)
            want = ref.process_watermark(wi * 1000 + 999)
            got = core.op_process_watermark(wi * 1000 + 999)
            assert len(got) == len(want) == 1
            assert_windows_equal(got[0], want[0])
            assert core.last_window_runs() == 1
        assert core.op_counters() == ref.counters()
        c = core.sampling_counters()
        assert c["replacements"] == c["feedbacks"] == c["item_cut_rejections"] == 0 and c["fills"] == sum(seen.values())


@pytest.mark.parametrize("planner", ["auto", "general"])
def test_random_log_many_users(pkg, oracle, planner):
    """300 users over 6 windows, reservoirs of 40 slots that fill over several windows (histories relocate as they
    grow), a hot item head that reaches the item cut: more than one workgroup in every kernel"""
    rng = np.random.default_rng(11)
    M, cut = 211, 40
    model = sm.SampledModel(M, 60, cut, SEED)
    with pkg.CooccurrenceCore(n_items=M, topk=4, user_cut=cut, item_cut=60, sample_seed=SEED, planner=planner) as core:
        for wi in range(6):
            users = np.where(rng.random(3000) < 0.5, rng.integers(0, 20, 3000), rng.integers(0, 300, 3000))
            items = np.minimum(rng.zipf(1.2, 3000) - 1, M - 1)
            recs = list(zip(users.tolist(), items.tolist()))
            w, mw = _fire(core, wi, recs), model.window(recs)
            _check_window(core, model, w, mw, oracle, 4)
        _check_invariant(core, model, oracle)
        c = core.sampling_counters()
        assert min(c["replacements"], c["feedbacks"], c["item_cut_rejections"], c["fills"]) > 100


def _find(total, want, lo=0):
    return sm.find_user_total(SEED, total, want, lo)


@pytest.mark.parametrize("cut,planner", [(c, "auto") for c in (1, 2, 63, 64, 65, 129, 500)]
                         + [(c, "general") for c in (2, 65, 500)])  # (the row-slab path takes the same lists)
def test_list_builder_edges(pkg, oracle, cut, planner):
    """k_sm_lists: one changed slot (first, last, slot 63, slot 64 where the reservoir has them), every slot changed,
    the same slot twice in a window, a slot filled and replaced in one window, a slot replaced by its own value, a
    user who is active but has nothing changed; user ids found with the model's draw"""
    M = 37
    d = lambda u, t: sm.draw(SEED, u, t)  # noqa: E731
    first = _find(cut + 1, lambda k: k == 0)
    while not d(first, cut + 2) < cut:  # (its next record is a replacement too: by its own value)
        first = _find(cut + 1, lambda k: k == 0, first + 1)
    last = _find(cut + 1, lambda k: k == cut - 1, first + 1)
    s63 = _find(cut + 1, lambda k: k == min(63, cut - 1), last + 1)
    s64 = _find(cut + 1, lambda k: k == min(64, cut - 1), s63 + 1)
    idle = _find(cut + 1, lambda k: k >= cut, s64 + 1)
    while not d(idle, cut + 2) >= cut:  # (two feedbacks in a row: the second one is a window of its own)
        idle = _find(cut + 1, lambda k: k >= cut, idle + 1)
    fresh = _find(cut + 1, lambda k: k < cut, idle + 1)
    twice = fresh + 1
    while not (d(twice, cut + 1) < cut and d(twice, cut + 1) == d(twice, cut + 2)):
        twice += 1
    both = None
    if cut == 2:  # two replacements that change both slots of a full reservoir
        both = twice + 1
        while not (d(both, 3) == 0 and d(both, 4) == 1):
            both += 1
    base = [first, last, s63, s64, idle, twice] + ([both] if both is not None else [])
    item = lambda u, s: (7 * s + 3 * u) % M  # noqa: E731
    windows = [
        [(u, item(u, s)) for s in range(cut) for u in base],                      # fills, interleaved across users
        [(first, 30), (last, 31), (s63, 32), (s64, 33), (idle, 34)]               # one slot each; idle: feedback only
        + [(fresh, item(fresh, s)) for s in range(cut)] + [(fresh, 35)]           # filled and replaced in one window
        + [(twice, 36), (twice, 29)]                                              # the same slot twice
        + ([(both, 28), (both, 27)] if both is not None else []),
        [],                                                                       # (filled in below)
    ]
    model = sm.SampledModel(M, 32767, cut, SEED)
    with pkg.CooccurrenceCore(n_items=M, topk=3, user_cut=cut, item_cut=32767, sample_seed=SEED,
                              planner=planner) as core:
        for wi, recs in enumerate(windows):
            if wi == 2:  # replaced by its own value: the item now in the slot the next draw names
                recs = [(first, model.H[first][d(first, cut + 2)])]
            w = _fire(core, wi, recs)
            mw = model.window(recs)
            if wi == 1:
                assert mw.decisions[:5] == ["k0", f"k{cut - 1}", f"k{min(63, cut - 1)}", f"k{min(64, cut - 1)}", "b"]
                assert mw.decisions[5:5 + cut] == ["f"] * cut and mw.decisions[5 + cut][0] == "k"
                assert mw.twice >= 2 and mw.decisions[6 + cut] == mw.decisions[7 + cut]  # (fresh's and twice's)
                assert core.last_window_runs() == 2
            if wi == 2:
                assert mw.decisions[-1] == f"k{d(first, cut + 2)}" and all(v == 0 for v in mw.delta.values())
                assert (len(mw.delta) > 0) == (cut > 1) and core.last_window_runs() == 2
            _check_window(core, model, w, mw, oracle, 3)
        _check_invariant(core, model, oracle)
        # a window in which only a feedback happens: empty, but the totals and the item counters move
        before = core.sampling_counters()
        w, mw = _fire(core, 3, [(idle, 2)]), model.window([(idle, 2)])
        assert mw.decisions == ["b"] and not mw.delta
        assert len(w.rows) == 0 and len(w.cols) == 0 and w.observed == 0 and core.last_window_runs() == 0
        after = core.sampling_counters()
        assert after["feedbacks"] == before["feedbacks"] + 1 and after == model.counters()
        assert core.user_history(idle)[1] == model.total[idle] == cut + 2


@pytest.mark.parametrize("n", [SD_BLOCK, SD_BLOCK + 1, SD_BLOCK + 2])
def test_combine_edges(pkg, oracle, n):
    """k_sd_*: a replacement of a unique item x by a new item y in a reservoir of n distinct items gives row y only
    in the plus run and row x only in the minus run, each of n - 1 entries -- one below, at and one above SD_BLOCK --
    and every other row one plus-only and one minus-only column; a replacement by the slot's own value gives
    identical plus and minus rows, all nets 0; a fill-only window skips the minus run"""
    M = 2 * n + 8
    u = _find(n + 1, lambda k: k < n)
    while not sm.draw(SEED, u, n + 2) < n:
        u = _find(n + 1, lambda k: k < n, u + 1)
    model = sm.SampledModel(M, 32767, n, SEED)
    with pkg.CooccurrenceCore(n_items=M, topk=2, user_cut=n, item_cut=32767, sample_seed=SEED) as core:
        recs = [(u, 2 * s + 1) for s in range(n)]
        w, mw = _fire(core, 0, recs), model.window(recs)
        assert core.last_window_runs() == 1  # no replacement: the minus run is skipped
        _check_window(core, model, w, mw, oracle, 2, rows_to_read=[0])
        y = M - 2
        w, mw = _fire(core, 1, [(u, y)]), model.window([(u, y)])
        assert core.last_window_runs() == 2
        x = 2 * sm.draw(SEED, u, n + 1) + 1
        rows = mw.rows()
        assert len(rows[y]) == len(rows[x]) == n - 1
        assert set(rows[y].values()) == {1} and set(rows[x].values()) == {-1}
        _check_window(core, model, w, mw, oracle, 2, rows_to_read=[0])
        own = model.H[u][sm.draw(SEED, u, n + 2)]
        w, mw = _fire(core, 2, [(u, own)]), model.window([(u, own)])
        assert core.last_window_runs() == 2 and len(mw.delta) == 2 * (n - 1) and not any(mw.delta.values())
        assert len(w.rows) == n and not w.exact.any() and not w.rs_exact.any()
        _check_window(core, model, w, mw, oracle, 2, rows_to_read=[0])
        _check_invariant(core, model, oracle)


def test_wrapped_views(pkg, oracle):
    """user_cut = 400, one user with 200 x a and 200 x b: the (a, b) count is 40,000 and wraps cnt16; then one a is
    replaced: the exact count, cnt16 and the top-k follow the model"""
    M, a, b, c = 8, 2, 5, 7
    u = _find(401, lambda k: k < 200)
    model = sm.SampledModel(M, 32767, 400, SEED)
    with pkg.CooccurrenceCore(n_items=M, topk=3, user_cut=400, item_cut=32767, sample_seed=SEED) as core:
        recs = [(u, a)] * 200 + [(u, b)] * 200
        w, mw = _fire(core, 0, recs), model.window(recs)
        assert mw.delta[(a, b)] == 40_000 and sm.i16(40_000) == -25_536
        _check_window(core, model, w, mw, oracle, 3)
        w, mw = _fire(core, 1, [(u, c)]), model.window([(u, c)])
        assert mw.delta[(a, b)] == -200 and model.G[(a, b)] == 39_800 and model.G[(c, b)] == 200
        _check_window(core, model, w, mw, oracle, 3)
        cols, cnt, cnt16 = core.global_row(a)
        assert dict(zip(cols.tolist(), cnt16.tolist()))[b] == sm.i16(39_800)
        _check_invariant(core, model, oracle)


def test_submit_batch_csr_order_is_the_arrival_order(pkg, oracle):
    """cooc_submit_batch: submit after submit, user after user, item after item"""
    windows = sm.reference_log()[:4]
    model = sm.SampledModel(24, 20, 4, SEED)
    with pkg.CooccurrenceCore(n_items=24, topk=0, user_cut=4, item_cut=20, sample_seed=SEED) as core:
        for wi, recs in enumerate(windows):
            order = []
            for half in (recs[:30], recs[30:]):  # two submits to the same window
                users = sorted({u for u, _ in half})
                by = {u: [i for v, i in half if v == u] for u in users}
                up = np.concatenate([[0], np.cumsum([len(by[u]) for u in users])]).astype(np.int64)
                core.submit_batch(wi, users, up, [i for u in users for i in by[u]])
                order += [(u, i) for u in users for i in by[u]]
            w = core.finish_window(wi)
            _check_window(core, model, w, model.window(order), oracle, 0)


def test_refusals(pkg):
    from flink_cooccurrence_amd import _lib
    from flink_cooccurrence_amd._lib import IllegalArgumentException, IllegalStateException

    L = _lib.load()
    with pkg.CooccurrenceCore(n_items=16, user_cut=3, item_cut=5, sample_seed=1) as core:
        for call in (core.snapshot, lambda: core.restore(b"\0" * 1024), lambda: core.restore_parts([b"\0" * 1024]),
                     lambda: core.comm_init(b"\0" * 128, 0, 1)):
            with pytest.raises(IllegalStateException, match="sampled"):
                call()
        ops = _lib.CoocCommOps()
        assert L.cooc_comm_init_ops(core._h, 0, 1, ops, None) == _lib.COOC_ERR_STATE
        with pytest.raises(IllegalStateException):  # already enabled
            _lib.check(L.cooc_sampling_enable(core._h, 5, 1), core._h)
    with pytest.raises(IllegalStateException, match="user_cut"):
        pkg.CooccurrenceCore(n_items=16, user_cut=0, item_cut=5)
    for bad in (32768, -1):
        with pytest.raises(IllegalArgumentException, match="item_cut"):
            pkg.CooccurrenceCore(n_items=16, user_cut=3, item_cut=bad)
    with pkg.CooccurrenceCore(n_items=16, user_cut=3) as core:
        assert L.cooc_sampling_enable(core._h, 0, 1) == _lib.COOC_ERR_ARG  # item_cut 0
        assert L.cooc_sampling_enable(core._h, 32768, 1) == _lib.COOC_ERR_ARG
        core.submit_batch(0, [1], [0, 1], [2])
        assert L.cooc_sampling_enable(core._h, 5, 1) == _lib.COOC_ERR_STATE  # after a submit
        core.finish_window(0)
        assert L.cooc_sampling_enable(core._h, 5, 1) == _lib.COOC_ERR_STATE
        # copy_user_history works in every mode
        items, total = core.user_history(1)
        assert items.tolist() == [2] and total == 1 and core.user_history(99)[0].size == 0
        assert core.last_window_runs() == 0
    with pkg.CooccurrenceCore(n_items=16, user_cut=3) as core:
        core.op_process_elements([1], [2], [5])
        assert L.cooc_sampling_enable(core._h, 5, 1) == _lib.COOC_ERR_STATE  # an element was processed
