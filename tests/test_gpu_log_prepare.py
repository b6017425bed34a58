"""cooc_log_prepare_device: every output equal to the numpy model (tests/_log_model.py, pinned by hand and against
the oracle in tests/test_ingest_device_cpu.py), and the prepared log through the existing counters and samplers equal
to the streaming operator fed the same text by run_text_source."""
import numpy as np
import pytest

import _log_model as lm
from test_ingest_device_cpu import E2E, SAMPLED

pytestmark = pytest.mark.gpu

SIZE, N_ITEMS = 1000, 300
INT32_MIN, INT32_MAX = lm.INT32_MIN, lm.INT32_MAX


@pytest.fixture(scope="module", autouse=True)
def torch_cuda():
    """torch's runtime comes up before the library's first context, as in the other device-tensor tests"""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def core(pkg, torch_cuda):
    with pkg.CooccurrenceCore(n_items=N_ITEMS, window_size_ms=SIZE) as c:
        yield c


def _dev(users, items, ts):
    import torch

    dev = torch.device("cuda:0")
    return (torch.tensor(np.asarray(users, np.int32), device=dev), torch.tensor(np.asarray(items, np.int32), device=dev),
            torch.tensor(np.asarray(ts, np.int64), device=dev))


KEYS = ("rec_user", "rec_item", "user_ids", "user_ptr", "user_items", "window_ptr", "window_ts")


def _check(core, users, items, ts, W, size=SIZE, n_items=N_ITEMS):
    want = lm.prepare(users, items, ts, W, size, n_items)
    got = core.prepare_log(*_dev(users, items, ts), records_per_watermark=W)
    assert got.info == {"n_kept": want["n_kept"], "n_late": want["n_late"], "n_users": want["n_users"],
                        "n_windows": want["n_windows"], "bad_record": -1}
    for k in KEYS:
        g = getattr(got, k)
        g = g if isinstance(g, np.ndarray) else g.cpu().numpy()
        assert g.dtype == want[k].dtype and np.array_equal(g, want[k]), (k, W, len(ts))
    return got, want


def _timestamps(rng, n, pattern):
    asc = 5_000 + np.sort(rng.integers(0, 4_000, n))  # a handful of windows
    if pattern == "ascending":
        return asc
    if pattern == "reversed":
        return asc[::-1].copy()
    if pattern == "shuffled":
        return rng.permutation(asc)
    return np.full(n, 7_777)  # all equal


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4095, 4096, 4097, 8193])
def test_equals_model_at_wave_and_tile_edges(core, n):
    rng = np.random.default_rng(100 + n)
    users = rng.integers(-50, 50, n) * 1_000_003
    items = rng.integers(0, N_ITEMS, n)
    sorted_paths = set()
    for pattern in ("ascending", "reversed", "shuffled", "equal"):
        ts = _timestamps(rng, n, pattern)
        for W in (0, 1, 7, 4096, n):
            got, want = _check(core, users, items, ts, W)
            if n > 64 and pattern in ("reversed", "shuffled"):
                assert want["n_late"] > 0 or W in (0, n) or W >= n
            sorted_paths.add(bool(np.all(np.diff(lm.window_end(ts[~want["late"]], SIZE)) >= 0)))
    if n > 64:
        assert sorted_paths == {True, False}  # both the skip-sort path and the radix sort ran


def test_one_window_and_300_windows_with_gaps(core):
    rng = np.random.default_rng(5)
    n = 3000
    users, items = rng.integers(0, 40, n), rng.integers(0, N_ITEMS, n)
    got, want = _check(core, users, items, rng.integers(2000, 3000, n), 0)
    assert want["n_windows"] == 1
    ends = np.cumsum(rng.integers(1, 4, 300)) * SIZE  # 300 window ends, gaps of up to two empty windows
    ts = rng.permutation(np.concatenate([ends - 1, rng.choice(ends, n - 300) - rng.integers(1, SIZE, n - 300)]))
    for W in (0, 1000):
        got, want = _check(core, users, items, ts, W)
        assert W or (want["n_windows"] == 300 and np.diff(want["window_ts"]).max() > SIZE)
    # negative timestamps: windows on both sides of 0
    _check(core, users, items, rng.integers(-5000, 5000, n), 0)


def test_user_id_edges(core):
    rng = np.random.default_rng(6)
    n = 5000
    items, ts = rng.integers(0, N_ITEMS, n), 1000 + np.arange(n)
    got, want = _check(core, rng.choice([INT32_MIN, -1, 0, INT32_MAX], n), items, ts, 500)
    assert want["user_ids"].tolist() == [INT32_MIN, -1, 0, INT32_MAX]
    _check(core, np.full(n, 42), items, ts, 500)  # one user for all records
    _check(core, np.full(n, INT32_MIN), items, ts, 500)
    got, want = _check(core, rng.permutation(n) - n // 2, items, ts, 500)  # every record its own user
    assert want["n_users"] == n


def test_checks_apply_to_kept_records_only(pkg, core):
    from flink_cooccurrence_amd import _lib

    users = np.zeros(6, np.int32)
    ts = np.array([100, 200, 150, 50, 300, 400], np.int64)  # W = 3: record 3 is late
    items = np.array([1, 2, 3, 99_999, 4, 5], np.int32)
    _check(core, users, items, ts, 3)  # the out-of-range item of a late record is ignored
    items[4], items[5] = -1, N_ITEMS
    with pytest.raises(_lib.IllegalArgumentException, match="record 4"):
        core.prepare_log(*_dev(users, items, ts), records_per_watermark=3)
    assert core.last_log_info["bad_record"] == 4 and core.last_log_info["n_late"] == 1
    # a timestamp beyond the overflow bound of the window expression, and the last one within it
    ok = np.ones(6, np.int32)
    for t5, bad in ((lm.INT64_MAX - 2 * SIZE + 1, True), (lm.INT64_MAX - 2 * SIZE, False),
                    (lm.INT64_MIN + 2 * SIZE - 1, True)):
        t2 = ts.copy()
        t2[5] = t5
        if bad and t5 > 0:
            with pytest.raises(_lib.IllegalArgumentException, match="record 5"):
                core.prepare_log(*_dev(users, ok, t2), records_per_watermark=3)
            assert core.last_log_info["bad_record"] == 5
        elif bad:  # (below the block maximum it is late, hence ignored; with W = 0 it is kept and refused)
            _check(core, users, ok, t2, 3)
            with pytest.raises(_lib.IllegalArgumentException, match="record 5"):
                core.prepare_log(*_dev(users, ok, t2), records_per_watermark=0)
        else:
            _check(core, users, ok, t2, 3)
    with pytest.raises(_lib.IllegalArgumentException):
        core.prepare_log(*_dev(users, ok, ts), records_per_watermark=-1)
    _check(core, users, ok, ts, 3)  # the context stays usable
    # Long.MIN_VALUE is late whatever the block
    t3 = ts.copy()
    t3[0] = lm.INT64_MIN
    assert _check(core, users, ok, t3, 0)[1]["n_late"] == 1


def test_cap_windows_two_phase(core):
    import ctypes

    from flink_cooccurrence_amd import _lib
    from flink_cooccurrence_amd.core import _p

    rng = np.random.default_rng(8)
    n = 4000
    users, items = rng.integers(0, 30, n), rng.integers(0, N_ITEMS, n)
    ts = rng.integers(0, 1500 * SIZE, n)  # more windows than prepare_log's first capacity
    got, want = _check(core, users, items, ts, 0)
    assert want["n_windows"] > 1024
    # the C call itself: too small a capacity reports the need and leaves the host lists alone
    du, di, dt = _dev(users, items, ts)
    info = _lib.CoocLogInfo()
    wp, wt = np.full(11, -3, np.int64), np.full(10, -3, np.int64)
    args = (core._h, n, ctypes.c_void_p(du.data_ptr()), ctypes.c_void_p(di.data_ptr()), ctypes.c_void_p(dt.data_ptr()),
            0, None, None, None, None, None)
    st = _lib.load().cooc_log_prepare_device(*args, _p(wp, _lib.i64p), _p(wt, _lib.i64p), 10, None, ctypes.byref(info))
    assert st == 1 and info.n_windows == want["n_windows"] and (wp == -3).all() and (wt == -3).all()
    wp, wt = np.zeros(info.n_windows + 1, np.int64), np.zeros(info.n_windows, np.int64)
    st = _lib.load().cooc_log_prepare_device(*args, _p(wp, _lib.i64p), _p(wt, _lib.i64p), info.n_windows, None,
                                             ctypes.byref(info))
    assert st == 0 and np.array_equal(wp, want["window_ptr"]) and np.array_equal(wt, want["window_ts"])
    # without the window lists no capacity is asked for
    st = _lib.load().cooc_log_prepare_device(*args, None, None, 0, None, ctypes.byref(info))
    assert st == 0 and info.n_windows == want["n_windows"] and info.n_users == want["n_users"]


def test_two_calls_are_bit_identical(core):
    import torch

    rng = np.random.default_rng(9)
    n = 8193
    d = _dev(rng.integers(-99, 99, n), rng.integers(0, N_ITEMS, n), rng.integers(0, 50_000, n))
    a, b = core.prepare_log(*d, records_per_watermark=700), core.prepare_log(*d, records_per_watermark=700)
    assert a.info == b.info and a.info["n_late"] > 0
    for k in KEYS:
        x, y = getattr(a, k), getattr(b, k)
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else torch.equal(x, y)


# ---- end to end against the streaming operator ------------------------------------------------------------------
@pytest.mark.parametrize("n_items,user_cut", [(300, 0), (300, 5), (40_500, 0), (40_500, 5)])
def test_text_to_counts_equals_streaming_operator(pkg, n_items, user_cut):
    c = E2E
    spread = n_items // c["n_items"]
    users, items, ts = lm.jitter_log(c["seed"], c["n"], c["n_users"], c["n_items"])
    text = lm.to_text(users, items * spread, ts)
    op = pkg.NonSampledUserInteractionCounterOneInputStreamOperator(1, "SECONDS", n_items=n_items, top_k=5,
                                                                    user_cut=user_cut)
    pkg.run_text_source(op, text, records_per_watermark=c["W"])
    with pkg.CooccurrenceCore(n_items=n_items, window_size_ms=c["size"], user_cut=user_cut) as core:
        log = core.prepare_log(*core.parse_interactions_device(text), records_per_watermark=c["W"])
        assert log.info["n_late"] == op.accumulators()["UserInteractionCounterLateElements"] > 0
        res = core.count_device(log.user_ptr, log.user_items)
        batch = core.copy_batch(res.nnz, res.observed)
    rs_exact, _ = op.core.global_rowsums()
    assert np.array_equal(batch.rowsum, rs_exact) and rs_exact.sum() > 0
    rows = range(n_items) if n_items == 300 else [int(a) for a in np.argsort(-rs_exact)[:40]] + [1, n_items - 1]
    for a in rows:
        cols, cnt, _ = op.core.global_row(a)
        e0, e1 = batch.row_ptr[a], batch.row_ptr[a + 1]
        assert np.array_equal(batch.cols[e0:e1], cols) and np.array_equal(batch.cnt[e0:e1], cnt), a


def test_prepared_log_through_the_sampler_equals_streaming(pkg):
    c = SAMPLED
    users, items, ts = lm.jitter_log(c["seed"], c["n"], c["n_users"], c["n_items"], negative_users=False)
    text = lm.to_text(users, items, ts)
    op = pkg.NonSampledUserInteractionCounterOneInputStreamOperator(
        1, "SECONDS", n_items=c["n_items"], top_k=5, user_cut=c["user_cut"], item_cut=c["item_cut"],
        sample_seed=c["draw_seed"])
    pkg.run_text_source(op, text, records_per_watermark=c["W"])
    with pkg.CooccurrenceCore(n_items=c["n_items"], window_size_ms=c["size"]) as core:
        log = core.prepare_log(*core.parse_interactions_device(text), records_per_watermark=c["W"])
        res_ptr, res_items, total, _, info = core.sample_owned(
            log.rec_user, log.rec_item, log.info["n_users"], log.user_ids, c["item_cut"], c["user_cut"],
            seed=c["draw_seed"], window_ptr=log.window_ptr)
    assert info["replacements"] > 0 and info["feedbacks"] > 0
    res_ptr, res_items, total = res_ptr.cpu().numpy(), res_items.cpu().numpy(), total.cpu().numpy()
    for j, uid in enumerate(log.user_ids.cpu().numpy()):
        h, t = op.user_history(int(uid))
        assert np.array_equal(res_items[res_ptr[j]:res_ptr[j + 1]], h) and total[j] == t, uid
