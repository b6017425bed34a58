"""cooc_sample_device on the GPU: the item cut, the reservoirs and the feedback of a device-resident log, window
after window from empty state, against the pure-Python model of the sampled mode (tests/_sampled_model.py) fed the
same windows.  Every comparison is exact equality: the reservoirs in slot order, the totals, the item counters,
the decision counters, and the count over the reservoirs against the model's global rows."""
import ctypes
import functools

import numpy as np
import pytest

import _sampled_model as sm

pytestmark = pytest.mark.gpu

SEED = 0x5EED


@pytest.fixture(scope="module", autouse=True)
def torch_cuda():
    """torch's runtime comes up before the library's first context, as in the other device-tensor tests"""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _model(windows, n_items, item_cut, user_cut, seed):
    model = sm.SampledModel(n_items, item_cut, user_cut, seed)
    twice = sum(model.window(w).twice for w in windows)
    return model, twice


def _filled_then_replaced(windows, n_items, item_cut, user_cut, seed):
    """replacements of a slot that the same window filled (from the model's decisions)"""
    model = sm.SampledModel(n_items, item_cut, user_cut, seed)
    events = 0
    for w in windows:
        lens = {u: len(h) for u, h in model.H.items()}
        filled: dict = {}
        for (u, _), d in zip(w, model.window(w).decisions):
            if d == "f":
                filled.setdefault(u, set()).add(lens.get(u, 0))
                lens[u] = lens.get(u, 0) + 1
            elif d.startswith("k") and int(d[1:]) in filled.get(u, ()):
                events += 1
    return events


@functools.lru_cache(maxsize=None)
def _reference(split, spread=1, user_mul=1, n_items=24):
    """the reference log as 8 windows (split 8), one window (1) or 16 half windows (16), and its model"""
    base = [[(u * user_mul, i) for u, i in w] for w in sm.reference_log(spread=spread)]
    if split == 1:
        windows = [[r for w in base for r in w]]
    elif split == 16:
        windows = [h for w in base for h in (w[:30], w[30:])]
    else:
        windows = base
    return windows, _model(windows, n_items, 20, 4, SEED)


@functools.lru_cache(maxsize=None)
def _boundary_log():
    rng = np.random.default_rng(11)
    windows = []
    for _ in range(3):
        n = 9000
        u = np.where(rng.random(n) < .5, 0, rng.integers(1, 40, n))
        i = np.where(rng.random(n) < .5, 0, np.minimum(rng.zipf(1.2, n) - 1, 299))
        windows.append(list(zip(u.tolist(), i.tolist())))
    return windows, _model(windows, 300, 70, 5, SEED)


@functools.lru_cache(maxsize=None)
def _extremes_log():
    rng = np.random.default_rng(5)
    return [[(int(rng.integers(0, 7)), int(rng.integers(0, 9))) for _ in range(300)] for _ in range(4)]


def _expected(model, n_users, n_items):
    lens = np.zeros(n_users, np.int64)
    total = np.zeros(n_users, np.int32)
    for u, h in model.H.items():
        lens[u] = len(h)
    for u, t in model.total.items():
        total[u] = t
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    items = np.array([i for u in sorted(model.H) for i in model.H[u]], np.int32)
    count = np.zeros(n_items, np.int16)
    for i, c in model.item_count.items():
        count[i] = c
    c = model.counters()
    info = {"rejected": c["item_cut_rejections"], "fills": c["fills"], "replacements": c["replacements"],
            "feedbacks": c["feedbacks"], "users": c["users"], "item_counter_sum": c["item_counter_sum"],
            "reservoir_items": int(ptr[-1])}
    return ptr, items, total, count, info


def _sample(core, windows, n_users, item_cut, user_cut, seed, explicit=True, **kw):
    import torch

    dev = torch.device("cuda:0")
    recs = [r for w in windows for r in w]
    users = torch.tensor([u for u, _ in recs], dtype=torch.int32, device=dev)
    items = torch.tensor([i for _, i in recs], dtype=torch.int32, device=dev)
    wp = np.concatenate([[0], np.cumsum([len(w) for w in windows])]).astype(np.int64) if explicit else None
    return core.sample_device(users, items, n_users, item_cut, user_cut, seed=seed, window_ptr=wp, **kw)


def _assert_equals_model(out, model, n_users, n_items):
    res_ptr, res_items, total, item_count, info = out
    ptr, items, tot, count, want = _expected(model, n_users, n_items)
    assert info == want
    assert np.array_equal(res_ptr.cpu().numpy(), ptr)
    assert np.array_equal(res_items.cpu().numpy(), items), "reservoirs differ (slot order)"
    assert np.array_equal(total.cpu().numpy(), tot)
    assert np.array_equal(item_count.cpu().numpy(), count)
    assert int(count.max(initial=0)) <= model.item_cut and int(count.min(initial=0)) >= 0


def _batch_rows(core, res_ptr, res_items):
    res = core.count_device(res_ptr, res_items)
    b = core.copy_batch(res.nnz, res.observed)
    rows = {}
    for a in np.flatnonzero(np.diff(b.row_ptr)).tolist():
        s, e = int(b.row_ptr[a]), int(b.row_ptr[a + 1])
        rows[a] = dict(zip(b.cols[s:e].tolist(), b.cnt[s:e].tolist()))
    return rows, int(res.observed)


def test_reference_log(pkg):
    """8 windows, n_items = 24, item_cut = 20, user_cut = 4: 48 fills, 50 replacements, 139 feedbacks and 14 slots
    written twice within a window; the outputs equal the model and a sampled streaming context fed the same
    windows, and the count over the reservoirs is the global state of both"""
    windows, (model, twice) = _reference(8)
    assert (model.fills, model.replacements, model.feedbacks, twice) == (48, 50, 139, 14)
    with pkg.CooccurrenceCore(n_items=24) as core:
        out = _sample(core, windows, 12, 20, 4, SEED)
        _assert_equals_model(out, model, 12, 24)
        res_ptr, res_items, total, _, info = out
        rows, observed = _batch_rows(core, res_ptr, res_items)
    assert rows == model.global_rows()
    lens = np.diff(res_ptr.cpu().numpy())
    assert observed == int(np.sum(lens * (lens - 1)))
    rp, ri, tot = res_ptr.cpu().numpy(), res_items.cpu().numpy(), total.cpu().numpy()
    with pkg.CooccurrenceCore(n_items=24, user_cut=4, item_cut=20, sample_seed=SEED) as stream:
        for wi, recs in enumerate(windows):
            users = np.array([u for u, _ in recs], np.int32)
            items = np.array([i for _, i in recs], np.int32)
            assert stream.op_process_elements(users, items, np.full(len(recs), wi * 1000 + 1, np.int64)) == 0
            assert len(stream.op_process_watermark(wi * 1000 + 999)) == 1
        for u in range(12):
            h, t = stream.user_history(u)
            assert h.tolist() == ri[rp[u]:rp[u + 1]].tolist() and t == tot[u], f"user {u}"
        c = stream.sampling_counters()
        assert [c[k] for k in ("item_cut_rejections", "fills", "replacements", "feedbacks", "users",
                               "item_counter_sum")] == \
            [info[k] for k in ("rejected", "fills", "replacements", "feedbacks", "users", "item_counter_sum")]
        for a in range(24):
            cols, cnt, _ = stream.global_row(a)
            assert dict(zip(cols.tolist(), cnt.tolist())) == rows.get(a, {}), f"global row {a}"


def test_tile_and_wave_boundaries(pkg):
    """3 windows of 9,000 records with half of them on user 0 and half on item 0: both runs cross a 4,096-element
    scan and sort tile.  200 fills, 154 replacements, 5,235 feedbacks, 108 slots written twice in a window"""
    windows, (model, twice) = _boundary_log()
    for w in windows:
        assert sum(1 for u, _ in w if u == 0) >= 4481 and sum(1 for _, i in w if i == 0) >= 5252
    assert (model.fills, model.replacements, model.feedbacks, twice) == (200, 154, 5235, 108)
    assert _filled_then_replaced(windows, 300, 70, 5, SEED) == 105  # a fill and a replacement of one slot, one window
    with pkg.CooccurrenceCore(n_items=300) as core:
        out = _sample(core, windows, 40, 70, 5, SEED)
        _assert_equals_model(out, model, 40, 300)
        rows, _ = _batch_rows(core, out[0], out[1])
    assert rows == model.global_rows()


@pytest.mark.parametrize("case", ["tight", "no_item_cut", "no_draw"])
def test_extremes(pkg, case):
    """4 windows of 300 records over 7 users and 9 items: item_cut = 3 with a reservoir of one slot (seed 3: 7
    fills, 7 replacements, 52 feedbacks), item_cut = 32767 (nothing rejected), user_cut = 32767 (never a draw)"""
    windows = _extremes_log()
    item_cut, user_cut, seed = {"tight": (3, 1, 3), "no_item_cut": (32767, 2, SEED), "no_draw": (3, 32767, SEED)}[case]
    model, _ = _model(windows, 9, item_cut, user_cut, seed)
    if case == "tight":
        assert (model.fills, model.replacements, model.feedbacks) == (7, 7, 52)
    elif case == "no_item_cut":
        assert model.rejected == 0 and model.replacements > 0 and model.feedbacks > 0
    else:
        assert model.replacements == model.feedbacks == 0 and model.rejected > 0
    with pkg.CooccurrenceCore(n_items=9) as core:
        _assert_equals_model(_sample(core, windows, 7, item_cut, user_cut, seed), model, 7, 9)


def test_windows(pkg):
    """empty windows between full ones; window_ptr = None against one explicit window; no record at all; the
    reference log as 8 windows, as one and as 16 halves (three different results: the feedback's timing)"""
    import torch

    ref8, (m8, _) = _reference(8)
    ref1, (m1, _) = _reference(1)
    ref16, (m16, _) = _reference(16)
    with pkg.CooccurrenceCore(n_items=24) as core:
        gaps = [[], ref8[0], [], [], ref8[1], ref8[2], []] + ref8[3:] + [[]]
        _assert_equals_model(_sample(core, gaps, 12, 20, 4, SEED), m8, 12, 24)
        outs = []
        for windows, model in ((ref8, m8), (ref1, m1), (ref16, m16)):
            outs.append(_sample(core, windows, 12, 20, 4, SEED))
            _assert_equals_model(outs[-1], model, 12, 24)
        assert len({(o[4]["replacements"], o[4]["feedbacks"], o[4]["rejected"]) for o in outs}) == 3
        implicit = _sample(core, ref1, 12, 20, 4, SEED, explicit=False)
        assert implicit[4] == outs[1][4]
        assert all(torch.equal(a, b) for a, b in zip(implicit[:4], outs[1][:4]))
        for wp in (None, [0, 0], [0, 0, 0, 0]):
            empty = torch.zeros(0, dtype=torch.int32, device="cuda:0")
            res_ptr, res_items, total, item_count, info = core.sample_device(empty, empty, 5, 20, 4, window_ptr=wp)
            assert res_ptr.tolist() == [0] * 6 and res_items.numel() == 0 and total.tolist() == [0] * 5
            assert int(item_count.abs().sum()) == 0 and set(info.values()) == {0}


@pytest.mark.parametrize("ids", ["items", "users"])
def test_wide_ids(pkg, ids):
    """item ids past 16 bits (the reference log spread by 41,000 over 1,000,000 items), then also user ids past 16
    bits (u * 5,801 of 70,000): every radix pass of both sorts; the large-universe count over the reservoirs"""
    M = 1_000_000
    mul, n_users = (5_801, 70_000) if ids == "users" else (1, 12)
    windows, (model, _) = _reference(8, spread=41_000, user_mul=mul, n_items=M)
    with pkg.CooccurrenceCore(n_items=M) as core:
        out = _sample(core, windows, n_users, 20, 4, SEED)
        _assert_equals_model(out, model, n_users, M)
        rows, _ = _batch_rows(core, out[0], out[1])
    assert rows == model.global_rows()


def test_determinism(pkg):
    """two calls give byte-equal outputs (integer adds and max are the only atomics)"""
    import torch

    windows, _ = _boundary_log()
    with pkg.CooccurrenceCore(n_items=300) as core:
        a = _sample(core, windows, 40, 70, 5, SEED)
        b = _sample(core, windows, 40, 70, 5, SEED)
    assert a[4] == b[4]
    for x, y in zip(a[:4], b[:4]):
        assert x.dtype == y.dtype and torch.equal(x, y)


def _raw(core, n, users, items, n_users=12, n_windows=1, wp=None, item_cut=20, user_cut=4, res_ptr=None,
         res_items=None, res_cap=None, info=True):
    """cooc_sample_device as given (no wrapper in between): its status and info"""
    from flink_cooccurrence_amd import _lib

    inf = _lib.CoocSampleInfo()
    wp = None if wp is None else np.ascontiguousarray(wp, np.int64)
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = _lib.load().cooc_sample_device(
        core._h, n, vp(users), vp(items), n_users, n_windows,
        None if wp is None else wp.ctypes.data_as(_lib.i64p), item_cut, user_cut, SEED, vp(res_ptr), vp(res_items),
        (0 if res_items is None else res_items.numel()) if res_cap is None else res_cap, None, None, None,
        ctypes.byref(inf) if info else None)
    return st, inf


def test_errors(pkg):
    """every COOC_ERR_ARG case, each followed by a valid call on the same context"""
    import torch

    from flink_cooccurrence_amd import _lib

    windows, (model, _) = _reference(8)
    dev = torch.device("cuda:0")
    recs = [r for w in windows for r in w]
    users = torch.tensor([u for u, _ in recs], dtype=torch.int32, device=dev)
    items = torch.tensor([i for _, i in recs], dtype=torch.int32, device=dev)
    users_ok, items_ok = users.clone(), items.clone()
    n = len(recs)
    wp8 = np.arange(9, dtype=np.int64) * 60
    res_ptr = torch.empty(13, dtype=torch.int64, device=dev)
    res_items = torch.empty(n, dtype=torch.int32, device=dev)
    with pkg.CooccurrenceCore(n_items=24) as core:
        def still_works():
            out = core.sample_device(users_ok, items_ok, 12, 20, 4, seed=SEED, window_ptr=wp8)
            _assert_equals_model(out, model, 12, 24)

        def refused(match=None, **kw):
            args = dict(n=n, users=users, items=items, res_ptr=res_ptr, res_items=res_items, n_windows=8, wp=wp8)
            args.update(kw)
            st, inf = _raw(core, **args)
            assert st == _lib.COOC_ERR_ARG
            if match is not None:
                assert match in _lib.load().cooc_last_error(core._h).decode()
            still_works()
            return inf

        for cut in (0, -1, 32768):
            refused(item_cut=cut)
            refused(user_cut=cut)
        refused(n_users=0)
        refused(n_users=-3)
        # window_ptr: not from 0, not to n_records, decreasing, NULL with several windows, no window
        bad = wp8.copy()
        bad[0] = 1
        refused(wp=bad)
        bad = wp8.copy()
        bad[-1] = n - 1
        refused(wp=bad)
        bad = wp8.copy()
        bad[3], bad[4] = bad[4], bad[3]
        refused(wp=bad)
        refused(wp=None, n_windows=2)
        refused(n_windows=0)
        # required pointers
        refused(res_ptr=None)
        refused(res_items=None, res_cap=n)
        refused(users=None)
        refused(items=None)
        refused(info=False)
        refused(res_cap=-1)
        # n_records out of range (nothing is read before the check)
        refused(n=-1, wp=None, n_windows=1)
        refused(n=1 << 31, wp=None, n_windows=1)
        # ids out of range, in the middle of a window: found on the device, nothing written
        for where, col, value in ((200, users, 12), (333, items, -1), (100, items, 24), (45, users, -7)):
            keep = int(col[where])
            col[where] = value
            res_ptr.fill_(-5)
            res_items.fill_(-5)
            refused(match=f"record {where}:")
            assert int((res_ptr != -5).sum()) == 0 and int((res_items != -5).sum()) == 0
            col[where] = keep
        users[50], items[400] = 99, 99  # two bad records: the first one is named
        refused(match="record 50:")
        users[50], items[400] = recs[50][0], recs[400][1]
        # res_cap below the reservoirs' size: the size needed comes back
        need = sum(len(h) for h in model.H.values())
        inf = refused(res_cap=need - 1, wp=wp8)
        assert inf.reservoir_items == need
        with pytest.raises(_lib.IllegalArgumentException):
            core.sample_device(users, items, 12, 20, 4, seed=SEED, window_ptr=wp8, res_cap=0)
        assert core.last_sample_info["reservoir_items"] == need
        out = core.sample_device(users, items, 12, 20, 4, seed=SEED, window_ptr=wp8, res_cap=need)
        _assert_equals_model(out, model, 12, 24)
