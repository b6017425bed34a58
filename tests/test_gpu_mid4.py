"""The any-order mid shape of k_sp_main (no block bitmaps in LDS: four workgroups per CU) and the lists' compact
bounds ({tile-0 start, end, tail start, end}: one 16-B record per list, read a batch ahead by the mid shapes'
walks) against rows summed directly from the lists and the closed form.  Needs an MI355X.

Every run is repeated with the A/B knobs off -- COOC_SP_MID4=0 (any-order runs keep the ranking mid shape),
COOC_SP_TBC=0 (bounds from the tile-start table), COOC_SP_MID=0 (mid rows in the big shape: batches of 512) --
and the results are compared bit for bit.  The knobs are read when a core is created.
"""
import numpy as np
import pytest

from tests.test_gpu_sparse import _Brute, _check_rows, _Rows

pytestmark = pytest.mark.gpu

_TW = 16384  # k_sp_main's tile width


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _csr(lists):
    up = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    it = np.concatenate([np.asarray(x, np.int32) for x in lists] + [np.zeros(0, np.int32)]).astype(np.int32)
    return up, it


def _pair_work(up, it, M):
    """W_a: the summed lengths of the lists holding a, once per position of a (the planner's row classes)."""
    lens = np.diff(up)
    return np.bincount(it, weights=np.repeat(lens, lens).astype(np.float64), minlength=M).astype(np.int64)


def _set_knobs(monkeypatch, env):
    for k in ("COOC_SP_MID4", "COOC_SP_TBC", "COOC_SP_MID"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---- mid rows ------------------------------------------------------------------------------------------
_HEAD = np.arange(100, 2500)                        # 2,400 head items
_PROBES = {3000: 45, 3001: 150, 3002: 300, 3003: 450, 200_000: 45, 200_001: 150, 200_002: 300, 200_003: 450}
_BIG = np.arange(4000, 4048)  # 48 rows above the mid class (600 holders each), for the big shape's launch
_OVF_ROW = 5


def _mid_log(U=2000, M=300_000, seed=23):
    """Rows in the mid class (4,096 < W <= 65,535 pairs), planned as a dense tile 0 plus hash chunks:
    every user holds 80 of the 2,400 head items and 40 uniform tail items (lists of ~135 with the probes), so a
    head item's row has c ~ 67 contributions, W ~ 9,000, about 2,500 expected distinct keys among the hot columns
    (above the mid shape's 1,843-key hash fill: tile 0 is dense) and ~150 per tail tile (about 12 tiles to a
    1,843-key chunk: two hash chunks over the 18 tail tiles).  Probe items held by 45 .. 450 users reach
    W ~ 6,000 .. 62,000, the upper ones with four or more chunks (gather mode).  48 items held by 600 users each
    are rows above the class: with a big-shape launch beside the mid one the planner sizes the output slabs as
    in a mixed log (without one it reserves a 4M-entry slab per workgroup, seconds of allocation per core).
    Row 5 is in three lists of 2,500 ids that occur nowhere else, all within one tile's width: ~7,500 distinct
    keys where the estimate sees a few hundred, in a 4,096-slot table -- its hash chunk overflows and the row
    is deferred to the sort path."""
    rng = np.random.default_rng(seed)
    lists = []
    for _ in range(U):
        lists.append(np.concatenate([rng.choice(_HEAD, 80, replace=False), rng.integers(_TW, 100_000, 20),
                                     rng.integers(120_000, M, 20)]))
    for p, c in list(_PROBES.items()) + [(int(b), 600) for b in _BIG]:
        for u in rng.choice(U, c, replace=False):
            lists[u] = np.append(lists[u], p)
    lists = [rng.permutation(x) for x in lists]
    own = rng.permutation(np.arange(100_000, 100_000 + _TW))[:7500].reshape(3, 2500)  # (no other list draws these)
    for k in range(3):
        lists.append(np.concatenate([[_OVF_ROW], own[k], [7, 7]]))
    up, it = _csr(lists)
    return up, it, M


@pytest.fixture(scope="module")
def mid_log():
    up, it, M = _mid_log()
    return up, it, M, _Brute(up, it, M)


def test_mid_rows_any_order_and_knobs_vs_brute(pkg, torch_cuda, monkeypatch, mid_log):
    """The mid-row log with any_order off and on, with the knobs on and each knob off where it acts (COOC_SP_MID4
    only changes any-order runs).  Every run: the overflowing row is deferred (asserted for the any-order runs),
    sampled rows of every class equal the rows summed from the lists bit for bit, and the whole result, copied
    to the host with every row sorted by column, equals the first run's entry by entry."""
    torch = torch_cuda
    up, it, M, brute = mid_log
    W = _pair_work(up, it, M)
    mid = (W > 4096) & (W <= 65535)
    assert np.all(mid[list(_PROBES)]) and mid[_OVF_ROW] and np.mean(mid[_HEAD]) > 0.99 and np.all(W[_BIG] > 65535)
    lens = np.diff(up)
    dev = torch.device("cuda")
    up_d, it_d = torch.from_numpy(up).to(dev), torch.from_numpy(it).to(dev)
    rng = np.random.default_rng(2)
    sample = np.concatenate([list(_PROBES), [_OVF_ROW, 7, int(_BIG[0])], rng.choice(_HEAD, 4, replace=False),
                             rng.choice(np.unique(it[it >= _TW]), 4, replace=False)])
    runs = [(False, {}), (True, {}), (True, {"COOC_SP_MID4": "0"}), (True, {"COOC_SP_TBC": "0"}),
            (False, {"COOC_SP_TBC": "0"})]
    first = None
    for any_order, env in runs:
        where = f"any_order={any_order} {env}"
        _set_knobs(monkeypatch, env)
        with pkg.CooccurrenceCore(n_items=M, device=0, any_order=any_order) as core:
            res = core.count_device(up_d, it_d)
            torch.cuda.current_stream().synchronize()
            assert res.observed == int(np.sum(lens * (lens - 1)))
            if any_order:
                assert core.last_sort_rows()[0] >= 1, "the overflowing row was not deferred"
            rows = _Rows(res, M)
            assert int(rows.nnz.sum()) == res.nnz, where
            _check_rows(rows, brute, sample)
            got = core.copy_batch(res.nnz, res.observed)
        if first is None:
            first = got
            continue
        assert np.array_equal(got.row_ptr, first.row_ptr) and np.array_equal(got.cols, first.cols), where
        assert np.array_equal(got.cnt, first.cnt) and np.array_equal(got.rowsum, first.rowsum), where


# ---- compact bounds ------------------------------------------------------------------------------------
_TARGETS = {10: 256, 11: 257, 12: 512, 13: 513, 90_000: 256, 90_001: 257, 90_002: 512, 90_003: 513}
_SINGLES = (20, 95_000, 95_001)  # rows of one contribution (in the 5,000-id list)
_POOL0 = np.arange(200, 1700)                     # tile-0 ids (columns are ids: column_order=True)
_POOL1 = _TW + 7 + 37 * np.arange(1500)           # tail ids
# (other tile-0 ids, other tail ids) of a target's first holders; the target itself adds one to its own side
_SHAPES0 = [(0, 0), (7, 0), (0, 4), (7, 4), (8, 5), (6, 3), (15, 0), (0, 8)]   # target in tile 0
_SHAPES1 = [(0, 0), (0, 3), (8, 3), (8, 0), (0, 7), (1, 0), (16, 4), (7, 2)]   # target in the tail


def _edge_log(M=100_000, seed=17):
    """Lists at the edges of the arenas' 16-B groups (8 tile-0 ids as u16, 4 tail ids as u32): no tile-0 ids, only
    tile-0 ids, lengths 0 and 1, exactly 8 tile-0 ids, exactly 4 tail ids; rows of exactly 256, 257, 512 and 513
    contributions (a walk batch of either shape, and one more: the read-ahead ends past the last batch) whose
    lists are ~25 long (W ~ 6,400 .. 13,000: mid rows), in tile 0 and in the tail; rows of ONE contribution
    with W = 5,000 (the items 20, 95,000 and 95,001 of one 5,000-id list).  The pools' items make small rows
    (k_sp_small), the two-id lists tiny rows (k_sp_tiny)."""
    rng = np.random.default_rng(seed)
    lists = [[], [], [150], [40_000], list(rng.choice(_POOL0, 8, replace=False)),
             list(rng.choice(_POOL1, 4, replace=False)), []]
    for x, c in _TARGETS.items():
        shapes = _SHAPES0 if x < _TW else _SHAPES1
        for i in range(c):
            n0, n1 = shapes[i] if i < len(shapes) else (3 + i % 17, 2 + (5 * i) % 23)
            lists.append(rng.permutation(np.concatenate([[x], rng.choice(_POOL0, n0, replace=False),
                                                         rng.choice(_POOL1, n1, replace=False)])))
    long_pool = np.concatenate([np.arange(3000, 3400), np.arange(80_000, 80_400)])
    lists.append(rng.permutation(np.concatenate([_SINGLES, rng.choice(long_pool, 4997)])))
    rare = np.arange(60_000, 60_400)
    for k in range(200):  # tiny rows: lists of 2 and 3 rare ids (a tail-only list, a mixed one)
        lists.append([rare[2 * k], rare[2 * k + 1]] if k % 2 else [rare[2 * k], rare[2 * k + 1], 5000 + k])
    lists.append([])
    up, it = _csr(lists)
    return up, it, M


@pytest.fixture(scope="module")
def edge_log(oracle):
    up, it, M = _edge_log()
    return up, it, M, oracle.closed_form(up, it, M)


def test_compact_bounds_edges_vs_closed_form(pkg, torch_cuda, monkeypatch, edge_log):
    """The edge log, whole CSR against the closed form: columns = ids (tile 0 = ids below 16,384) with any_order off
    and on, the compact bounds on and off, mid rows in the mid shapes (batches of 256) and, COOC_SP_MID=0, in the
    big shape (batches of 512); once more with the column relabel (every id hot: lists of tile-0 ids only)."""
    up, it, M, (rp, cols, data, rowsums, observed) = edge_log
    W, c = _pair_work(up, it, M), np.bincount(it, minlength=M)
    for x, n in _TARGETS.items():
        assert c[x] == n and 4096 < W[x] <= 65535
    for x in _SINGLES:
        assert c[x] == 1 and 4096 < W[x] <= 65535
    runs = [(dict(column_order=True, any_order=ao), env) for ao in (False, True)
            for env in ({}, {"COOC_SP_TBC": "0"}, {"COOC_SP_MID": "0"}, {"COOC_SP_MID": "0", "COOC_SP_TBC": "0"})]
    runs.append((dict(), {}))
    for kw, env in runs:
        _set_knobs(monkeypatch, env)
        with pkg.CooccurrenceCore(n_items=M, device=0, **kw) as core:
            got = core.count(up, it)
        where = f"{kw} {env}"
        assert got.observed == observed, where
        assert np.array_equal(got.row_ptr, rp) and np.array_equal(got.cols, cols), where
        assert np.array_equal(got.cnt.astype(np.int64), data) and np.array_equal(got.rowsum, rowsums), where


@pytest.mark.parametrize("tbc", ["1", "0"])
def test_compact_bounds_streaming_window_vs_oracle(pkg, oracle, torch_cuda, monkeypatch, edge_log, tbc):
    """The edge log's lists as a stream over two windows (n_items = 100,000: the sparse global rows; two lists per
    user, its whole history and the window's new items, each with a bounds record): every list's first half
    arrives in window 0, the rest in window 1.  Delta rows, row sums, observed and top-k of both windows and the
    final global rows against the oracle's record-by-record operator."""
    from flink_cooccurrence_amd import datagen
    from tests._helpers import INT64_MAX, assert_windows_equal

    up, it, M, _ = edge_log
    lens = np.diff(up)
    pos = np.arange(len(it)) - np.repeat(up[:-1], lens)
    ts = np.where(2 * pos < np.repeat(lens, lens), 100, 1100).astype(np.int64) + pos % 50
    users, items, ts = datagen.to_records(up, it, ts)
    _set_knobs(monkeypatch, {"COOC_SP_TBC": tbc})
    op = pkg.NonSampledUserInteractionCounterOneInputStreamOperator(1, "SECONDS", n_items=M, top_k=10)
    ref = oracle.OracleStream(1000, topk=10)
    got, want = [], []
    for lo in range(0, len(users), 20_000):
        sl = slice(lo, lo + 20_000)
        op.process_elements(users[sl], items[sl], ts[sl])
        ref.process_elements(users[sl], items[sl], ts[sl])
    got += op.process_watermark(INT64_MAX)
    want += ref.process_watermark(INT64_MAX)
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert_windows_equal(g, w)
    rows, rp, cols, exact, v16 = ref.global_rows()
    for r in list(range(0, len(rows), max(1, len(rows) // 100))) + [len(rows) - 1]:
        a = int(rows[r])
        c, n, n16 = op.core.global_row(a)
        assert np.array_equal(c, cols[rp[r]:rp[r + 1]]), f"global row {a}"
        assert np.array_equal(n.astype(np.int64), exact[rp[r]:rp[r + 1]])
        assert np.array_equal(n16, v16[rp[r]:rp[r + 1]])
    op.close()
