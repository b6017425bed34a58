"""The counting walk of k_sp_main at the edges of the arenas' 16-B groups, in every walk mode: dense adds into
u32 counters (the big shape) and into packed u16 counters (the mid shapes), the gather walk (arena0 counted,
arena1 appended to the tiles' buckets), bucket walks into dense tiles and into hash tables.  The dense adds go
by the lane mask alone (a masked id adds 0 at an address folded into the counter array), so the log has
segments that start and end at every lane of a group, pads read by masked lanes, and counts at both halves of
the first and the last packed word.  Against rows summed directly from the lists.  Needs an MI355X.
"""
import numpy as np
import pytest

from tests.test_gpu_sparse import _Brute, _check_rows, _Rows

_M = 100_000
_TW = 16384  # k_sp_main's tile width: 7 tiles at 100,000 columns (columns are ids: column_order=True)
_T = (_M + _TW - 1) // _TW
_EDGE_COLS = (0, 1, _TW - 2, _TW - 1)  # both halves of the first and of the last packed-u16 word

# target rows, one in tile 0 and one in the tail per class; their holders are the lists of a group below
_MID_G = (3000, 50_000)   # mid rows (u16 counters) of >= 4 chunks: gather mode, hash chunks read the buckets
_MID_S = (3002, 50_002)   # mid rows of fewer chunks: every chunk walks the lists
_MID_D = (3001, 50_001)   # mid rows whose tail tiles are dense too: bucket walks into u16 counters
_BIG = (3003, 50_003)     # rows above 65,535 pairs (u32 counters): gather mode, dense tail tiles
# how many of a group's lists hold each edge column: distinct counts, in the mid groups an odd column whose even
# neighbour's count is zero and the reverse
_EDGE_G1 = {0: 310, 1: 0, _TW - 2: 0, _TW - 1: 270}
_EDGE_G2 = {0: 0, 1: 230, _TW - 2: 190, _TW - 1: 0}
_EDGE_G3 = {0: 300, 1: 200, _TW - 2: 250, _TW - 1: 150}

_HEAD = np.arange(6000, 12000)          # the background's 6,000 head items
_POOL0 = np.arange(4000, 5500)          # the groups' other tile-0 ids
_POOL_T = 600                           # ... and their tail ids: the first 600 of every tail tile (hash chunks stay
                                        # well inside their tables)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _group_list(rng, i, targets, edge, tail_per_tile, min0=0):
    """List i of a group: a tile-0 part of max(i % 18, min0) ids (the tile-0 target among them; a list with none
    does not hold it) unless its edge columns need more, and per tail tile a part of tail_per_tile - 2 .. + 2 ids (over a group the
    parts start and end at each lane of a u32 group), the tail target in its tile."""
    n0 = max(i % 18, min0)
    part0 = [c for c, n in edge.items() if i < n]
    if n0 > 0:
        part0.append(targets[0])
    if len(part0) < n0:
        part0 += list(rng.choice(_POOL0, n0 - len(part0), replace=False))
    parts = [np.asarray(part0, np.int64)]
    for t in range(1, _T):
        n = tail_per_tile + int(rng.integers(-2, 3))
        ids = t * _TW + rng.choice(_POOL_T, max(n, 0), replace=False)
        if t == targets[1] // _TW:
            ids = np.append(ids, targets[1])
        parts.append(ids)
    return rng.permutation(np.concatenate(parts))


def _walk_log(seed=29):
    """2,000 background lists (120 of 6,000 head items and 40 uniform tail ids each: they set the tiles' masses and
    expected distinct keys, by which the planner picks dense and hash chunks) and three groups of crafted lists:
    G1, 800 lists of ~25 ids, holds _MID_G; G2, 263 of ~25, holds _MID_S; G3, 700 of ~240, holds _BIG, and its
    first 235 lists hold _MID_D as well.  The last list has 3 tile-0 ids and 2 tail ids: both arenas end in pads."""
    rng = np.random.default_rng(seed)
    lists = [np.concatenate([rng.choice(_HEAD, 120, replace=False), rng.integers(_TW, _M, 40)]) for _ in range(2000)]
    lists = [rng.permutation(x) for x in lists]
    for i in range(700):
        x = _group_list(rng, i, _BIG, _EDGE_G3, 38)
        if i < 235:
            x = np.concatenate([x, [_MID_D[1]], [_MID_D[0]] if i % 18 else []])
        lists.append(x.astype(np.int64))
    for i in range(263):
        lists.append(_group_list(rng, i, _MID_S, _EDGE_G2, 3, min0=1))  # (both targets in every list: equal W)
    for i in range(800):
        lists.append(_group_list(rng, i, _MID_G, _EDGE_G1, 3))
    lists.append(np.array([_MID_G[0], 70_001, 4001, _MID_G[1], 4002]))
    up = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return up, np.concatenate(lists).astype(np.int32)


def _pair_work(up, it):
    lens = np.diff(up)
    return np.bincount(it, weights=np.repeat(lens, lens).astype(np.float64), minlength=_M).astype(np.int64)


def _plan(W, freq, mid):
    """The planner's chunks of a whole row of W pairs (k_sp_plan, with the exact expected distinct keys where
    it interpolates a table): (tile 0 dense, chunks, dense tail tiles)."""
    n = float(freq.sum())
    hmax = 4096 if mid else 8192
    hfill = 0.45 * hmax
    chunks, cur, open_, dense = 0, 0.0, False, []
    for t in range(_T):
        f = freq[t * _TW:(t + 1) * _TW].astype(np.float64)
        d = float(np.sum(-np.expm1(-W * f[f > 0] / n)))
        if d > hfill or W * f.sum() / n > 2 * _TW:
            dense.append(t)
            chunks, open_ = chunks + 1, False
        else:
            if not open_ or cur + d > hfill:
                chunks, open_, cur = chunks + 1, True, 0.0
            cur += d
    return 0 in dense, chunks, [t for t in dense if t > 0]


@pytest.fixture(scope="module")
def walk_log():
    up, it = _walk_log()
    return up, it, _Brute(up, it, _M)


def test_walk_log_shapes(walk_log):
    """The log is what the GPU tests take it for (no GPU involved; kept here, beside them, so that a change of
    the log that loses an edge fails where it is made)."""
    up, it, brute = walk_log
    W = _pair_work(up, it)
    freq = np.bincount(it, minlength=_M)
    for x in _MID_G + _MID_S + _MID_D:
        assert 4096 < W[x] <= 65535, (x, W[x])
    for x in _BIG:
        assert W[x] > 65535 and W[x] < (1 << 23), (x, W[x])
    # the chunk plans, with room for the planner's table (linear in log2 W between half octaves: well within a
    # percent of the exact sum): W 8% lower and higher give the same classes
    for x in _MID_G:
        for s in (0.92, 1.0, 1.08):
            d0, chunks, dtail = _plan(s * W[x], freq, True)
            assert d0 and chunks >= 4 and not dtail, (x, s, d0, chunks, dtail)
    for x in _MID_S:
        for s in (0.92, 1.0, 1.08):
            d0, chunks, dtail = _plan(s * W[x], freq, True)
            assert d0 and chunks < 4, (x, s, d0, chunks)
    for x in _MID_D:
        for s in (0.92, 1.0, 1.08):
            d0, chunks, dtail = _plan(s * W[x], freq, True)
            assert d0 and chunks >= 4 and len(dtail) >= 4, (x, s, d0, chunks, dtail)
    for x in _BIG:
        for s in (0.92, 1.0, 1.08):
            d0, chunks, dtail = _plan(s * W[x], freq, False)
            assert d0 and chunks >= 4 and len(dtail) >= 4, (x, s, d0, chunks, dtail)
    # ragged ends: per list the tile-0 part's length (arena0, 8 ids per group) and the tail tiles' parts (arena1, 4)
    n_lists = len(up) - 1
    user = np.repeat(np.arange(n_lists), np.diff(up))
    tile = it.astype(np.int64) // _TW
    cnt = np.zeros((n_lists, _T), np.int64)
    np.add.at(cnt, (user, tile), 1)
    for targets in (_MID_G, _MID_S, _BIG):
        hold = np.unique(user[it == targets[1]])
        assert set(range(targets == _MID_S, 18)) <= set(cnt[hold, 0].tolist()), targets
        starts = np.cumsum(cnt[hold, 1:], axis=1) - cnt[hold, 1:]
        ends = starts + cnt[hold, 1:]
        ne = cnt[hold, 1:] > 0
        assert {(a, b) for a in range(4) for b in range(4)} <= set(zip((starts[ne] % 4).tolist(), (ends[ne] % 4).tolist()))
    assert cnt[-1, 0] % 8 == 3 and cnt[-1, 1:].sum() % 4 == 2 and it[up[-2]] == _MID_G[0]
    # the edge columns' counts in the target rows: distinct, a few hundred, zero beside nonzero in the mid rows
    for targets, edge in ((_MID_G, _EDGE_G1), (_MID_S, _EDGE_G2), (_BIG, _EDGE_G3)):
        c, n = brute.row(targets[1])
        got = {col: int(n[c == col].sum()) for col in _EDGE_COLS}
        assert got == edge, (targets, got)
        assert len({v for v in got.values() if v}) == len([v for v in got.values() if v])
    assert len(set(_EDGE_G3.values())) == 4 and min(_EDGE_G3.values()) >= 100


_SAMPLE = list(_MID_G + _MID_S + _MID_D + _BIG) + list(_EDGE_COLS) + [6000, 11999, 4000, 4001, 70_001, _TW, 2 * _TW + 5]


@pytest.mark.gpu
@pytest.mark.parametrize("mid", ["1", "0"])
def test_walk_edges_vs_brute(pkg, torch_cuda, monkeypatch, walk_log, mid):
    """The log with any_order off and on; mid = "0" (COOC_SP_MID=0): the mid rows again in the big shape (u32
    counters, batches of 512).  The target rows, the edge columns' own rows and rows of the background equal the
    rows summed from the lists bit for bit, and the two runs' host copies are equal entry by entry."""
    torch = torch_cuda
    up, it, brute = walk_log
    lens = np.diff(up)
    for k in ("COOC_SP_MID4", "COOC_SP_TBC", "COOC_SP_MID"):
        monkeypatch.delenv(k, raising=False)
    if mid == "0":
        monkeypatch.setenv("COOC_SP_MID", "0")
    dev = torch.device("cuda")
    up_d, it_d = torch.from_numpy(up).to(dev), torch.from_numpy(it).to(dev)
    first = None
    for any_order in (False, True):
        with pkg.CooccurrenceCore(n_items=_M, device=0, column_order=True, any_order=any_order) as core:
            res = core.count_device(up_d, it_d)
            torch.cuda.current_stream().synchronize()
            assert res.observed == int(np.sum(lens * (lens - 1)))
            assert core.last_sort_rows()[0] == 0, "a hash table overflowed: the row left k_sp_main"
            rows = _Rows(res, _M)
            assert int(rows.nnz.sum()) == res.nnz
            assert int(rows.rowsum.sum()) == res.observed
            _check_rows(rows, brute, _SAMPLE)
            got = core.copy_batch(res.nnz, res.observed)
        if first is None:
            first = got
            continue
        assert np.array_equal(got.row_ptr, first.row_ptr) and np.array_equal(got.cols, first.cols)
        assert np.array_equal(got.cnt, first.cnt) and np.array_equal(got.rowsum, first.rowsum)
