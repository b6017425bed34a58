"""The write sweeps of the dense compactions: sp_dense_compact (k_sp_main's dense tiles: u32 counters in the big
shape, packed u16 counters in the mid shapes) and the second pass of k_sp_split_finalize take a wave step's
columns interleaved over the lanes, one LDS word (or staging cell) per lane and sub-step, so that the active lanes
of a store write one contiguous run.  Rows against rows summed directly from the lists, bit for bit, and every
whole result (host copy, every row sorted by column) against the any_order=False run's, entry by entry.
Needs an MI355X.

The logs put non-zero counters where the lane mapping can go wrong: a tile with every counter non-zero (every
lane active in every sub-step), a tile whose only non-zero counter is its last column, counters on both sides
of the waves' range boundaries, a last tile of odd width that is no multiple of a wave step, u16 words with one
half or both halves set, the row's own column (zero after the self term), relabelled ids (the hot-column map),
and a split row whose finalize ends in a partial wave step.
"""
import numpy as np
import pytest

from tests.test_gpu_mid4 import _HEAD, _csr, _mid_log, _pair_work
from tests.test_gpu_sparse import _Brute, _check_rows, _Rows

pytestmark = pytest.mark.gpu

_TW = 16384          # k_sp_main's tile width
_SPLIT_W = 1 << 23   # rows above this pair work are split
# the planner's dense-tile rule (cooc_sparse_plan.hip): expected pairs in the tile W gmass[t] > 2 kTW, or expected
# distinct keys sum_b 1 - exp(-W f_b / N) above 0.45 x the shape's hash slots (8,192 big, 4,096 mid)
_DENSE_PAIRS, _DENSE_KEYS_BIG, _DENSE_KEYS_MID = 2.0 * _TW, 0.45 * 8192, 0.45 * 4096


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _count(pkg, torch, up, it, M, **kw):
    """A core with the flags kw and its count of the log on the device (the caller closes the core)."""
    dev = torch.device("cuda")
    core = pkg.CooccurrenceCore(n_items=M, device=0, **kw)
    res = core.count_device(torch.from_numpy(up).to(dev), torch.from_numpy(it).to(dev))
    torch.cuda.current_stream().synchronize()
    return core, res


def _same(got, first, where):
    assert np.array_equal(got.row_ptr, first.row_ptr) and np.array_equal(got.cols, first.cols), where
    assert np.array_equal(got.cnt, first.cnt) and np.array_equal(got.rowsum, first.rowsum), where


def _planned_dense(up, it, M, a, t, mid):
    """Row a's tile t (columns = ids) is dense by the planner's rule, with a quarter to spare."""
    f = np.bincount(it, minlength=M).astype(np.float64)
    N, W = float(len(it)), float(_pair_work(up, it, M)[a])
    ft = f[t * _TW:min(M, (t + 1) * _TW)]
    pairs, keys = W * ft.sum() / N, float(np.sum(1.0 - np.exp(-W * ft / N)))
    return pairs > 1.25 * _DENSE_PAIRS or keys > 1.25 * (_DENSE_KEYS_MID if mid else _DENSE_KEYS_BIG)


# ---- dense tiles of both shapes, a universe of three tiles just above the large-universe threshold --------------
_M = 2 * _TW + 8107  # 40,875 >= 40,320: the last tile is 8,107 columns wide (odd; no multiple of 256 or 512)
_FULL, _LAST, _EDGE = 100, 101, 102      # big rows (W > 65,535)
_MFULL, _MEDGE, _MSELF = 110, 111, 112   # mid rows (4,096 < W <= 65,535)
# both sides of the waves' range boundaries: 2,048 columns per wave in a full tile of the big shape (8 waves), 4,096
# in the mid shapes (4 waves); in the last tile 1,024 and 2,048, the last wave's range cut by the tile's end
_EDGE_COLS = np.array(
    [t * _TW + o for t in (0, 1) for o in (0, 2047, 2048, 4095, 4096, 8191, 8192, 12287, 12288, _TW - 1)] +
    [2 * _TW + o for o in (0, 1023, 1024, 2047, 2048, 6143, 6144, 7167, 7168, 8105, 8106)] +
    # u16 words with the low half, the high half and both halves set (their other columns stay zero)
    [1000, 1003, 1006, 1007, _TW + 1000, _TW + 1003, _TW + 1006, _TW + 1007])


def _edge_log(seed=41):
    """Lists [a] * r + columns, shuffled: row a holds r * (the columns' multiplicity) at each of them, and its pair
    work is r * the lists' summed lengths.
      _FULL / _MFULL: 160 lists over blocks of 256 consecutive ids, and one list with the five other rows named
      here: every column of every tile non-zero (but _MFULL's own: once per list).  That one list also puts those
      six columns of tile 0 into the rows below; their tiles 1 and 2 hold what is said here and nothing else.
      _LAST: the last columns of tiles 1 and 2.
      _EDGE / _MEDGE: the columns of _EDGE_COLS.
      _MSELF: once in each of 100 lists of 400 distinct other ids: its own column's counter is zero after the self
      term and must not be emitted.
    The other ids' rows are small and tiny rows (k_sp_small, k_sp_tiny)."""
    rng = np.random.default_rng(seed)
    named = np.array([_FULL, _LAST, _EDGE, _MFULL, _MEDGE, _MSELF])
    plain = np.setdiff1d(np.arange(_M), named)
    blocks = [plain[b:b + 256] for b in range(0, len(plain), 256)]
    lists = []
    for a, r in ((_FULL, 32), (_MFULL, 1)):
        lists += [np.concatenate([np.full(r, a), blk]) for blk in blocks + [named[named != a]]]
    lists += [np.concatenate([np.full(200, _LAST), [2 * _TW - 1, _M - 1]]) for _ in range(24)]
    lists += [np.concatenate([np.full(200, _EDGE), _EDGE_COLS]) for _ in range(24)]
    lists += [np.concatenate([np.full(30, _MEDGE), _EDGE_COLS]) for _ in range(24)]
    lists += [np.concatenate([[_MSELF], rng.choice(plain, 400, replace=False)]) for _ in range(100)]
    up, it = _csr([rng.permutation(x) for x in lists])
    return up, it, _M


@pytest.fixture(scope="module")
def edge_log():
    up, it, M = _edge_log()
    return up, it, M


@pytest.mark.parametrize("permute", [False, True])
def test_dense_tiles_both_shapes_vs_brute(pkg, torch_cuda, edge_log, permute):
    """permute=False: columns are ids (column_order: no relabel, asserted), so the tiles hold the patterns above.
    permute=True: the ids permuted and the default flags, so the hot-column map is taken (asserted through
    column_order()); tile 0 is then the 16,384 most frequent ids in ascending id order -- still every counter
    non-zero for the two full rows, and at least as much of the interactions as before, so still dense.
    Both with any_order off and on (the ranking and the any-order mid shape)."""
    torch = torch_cuda
    up, it, M = edge_log
    W = _pair_work(up, it, M)
    big, mid = (_FULL, _LAST, _EDGE), (_MFULL, _MEDGE, _MSELF)
    assert np.all(W[list(big)] > 65535) and np.all(W[list(big)] <= _SPLIT_W)
    assert np.all(W[list(mid)] > 4096) and np.all(W[list(mid)] <= 65535)
    for a in big + mid:
        for t in range(3):
            assert _planned_dense(up, it, M, a, t, a in mid), f"row {a} tile {t} is not planned dense"
    rng = np.random.default_rng(9)
    sample = np.concatenate([big, mid, rng.choice(np.setdiff1d(np.arange(M), big + mid), 12, replace=False)])
    if permute:
        perm = rng.permutation(M).astype(np.int32)
        it, sample = perm[it], perm[sample]
    brute = _Brute(up, it, M)
    if not permute:  # the patterns, from the lists
        named = np.array(big + mid)
        assert len(brute.row(_FULL)[0]) == M
        assert np.array_equal(brute.row(_MFULL)[0], np.setdiff1d(np.arange(M), [_MFULL]))
        assert np.array_equal(brute.row(_LAST)[0], np.union1d(named, [2 * _TW - 1, M - 1]))
        assert np.array_equal(brute.row(_MEDGE)[0], np.union1d(_EDGE_COLS, named))
        assert _MSELF not in brute.row(_MSELF)[0]
    first = None
    for any_order in (False, True):
        where = f"permute={permute} any_order={any_order}"
        core, res = _count(pkg, torch, up, it, M, column_order=not permute, any_order=any_order)
        with core:
            lens = np.diff(up)
            assert res.observed == int(np.sum(lens * (lens - 1))), where
            relabelled = not np.array_equal(core.column_order(), np.arange(M))
            assert relabelled == permute, where
            rows = _Rows(res, M)
            assert int(rows.nnz.sum()) == res.nnz, where
            _check_rows(rows, brute, sample)
            got = core.copy_batch(res.nnz, res.observed)
        if first is None:
            first = got
        else:
            _same(got, first, where)


# ---- mid rows: a dense u16 tile 0 beside hash chunks (the log of test_gpu_mid4) ---------------------------------
@pytest.mark.parametrize("column_order", [True, False])
def test_mid_rows_u16_words_vs_brute(pkg, torch_cuda, column_order):
    """The four head rows of most pair work of the mid-row log and two of its probe rows (dense tile 0: about 2,300
    of the 2,400 head columns non-zero in a head row, so words with the low half, the high half and both halves
    set -- asserted -- and the row's own column, zero after the self term), any_order off and on; with columns =
    ids, and with the default flags (the head ids are 2,400 of the 16,384 hottest: relabelled, asserted)."""
    torch = torch_cuda
    up, it, M = _mid_log()
    brute = _Brute(up, it, M)
    W = _pair_work(up, it, M)
    rng = np.random.default_rng(4)
    heads = _HEAD[np.argsort(-W[_HEAD], kind="stable")[:4]]
    dense = np.concatenate([heads, [3001, 3003]])
    assert np.all((W[dense] > 4096) & (W[dense] <= 65535))
    for a in dense:
        assert _planned_dense(up, it, M, int(a), 0, True), f"row {a}: tile 0 is not planned dense"
        assert int(a) not in brute.row(int(a))[0]
    for a in heads:
        c = brute.row(int(a))[0]
        nz = np.zeros(_TW, bool)
        nz[c[c < _TW]] = True
        lo, hi = nz[0::2], nz[1::2]
        assert np.any(lo & ~hi) and np.any(~lo & hi) and np.any(lo & hi)
    sample = np.concatenate([dense, rng.choice(np.unique(it[it >= _TW]), 4, replace=False)])
    first = None
    for any_order in (False, True):
        where = f"column_order={column_order} any_order={any_order}"
        core, res = _count(pkg, torch, up, it, M, column_order=column_order, any_order=any_order)
        with core:
            relabelled = not np.array_equal(core.column_order(), np.arange(M))
            assert relabelled == (not column_order), where
            rows = _Rows(res, M)
            assert int(rows.nnz.sum()) == res.nnz, where
            _check_rows(rows, brute, sample)
            got = core.copy_batch(res.nnz, res.observed)
        if first is None:
            first = got
        else:
            _same(got, first, where)


# ---- a split row: k_sp_split_finalize -------------------------------------------------------------------------
_MS = 50_001  # no multiple of 1,024 (nor is _MS + 16,384, the relabelled column space): the last wave step is partial
_SPLIT = 7


def _split_log(seed=43):
    """1,400 lists of item 7 x 64 and 40 uniform ids: every (u, 7) interaction is one contribution of 104 pairs,
    W_7 = 1,400 x 64 x 104 = 9.3e6 > 2^23 from 146,000 interactions; the other rows are tiny."""
    rng = np.random.default_rng(seed)
    lists = [rng.permutation(np.concatenate([np.full(64, _SPLIT), rng.integers(0, _MS, 40)])) for _ in range(1400)]
    up, it = _csr(lists)
    return up, it, _MS


def test_split_row_finalize_vs_brute(pkg, torch_cuda, monkeypatch):
    """The split row whole against the bincount of its lists, sampled other rows, and the whole result against
    the first run's: mirroring on (the default; one mirrored row, asserted) and off (COOC_SP_MIRROR=0, read when a
    core is created), relabelled ids (the default flags: uniform ids, asserted) and columns = ids, any_order on."""
    torch = torch_cuda
    up, it, M = _split_log()
    W = _pair_work(up, it, M)
    assert W[_SPLIT] > _SPLIT_W and np.count_nonzero(W > _SPLIT_W) == 1 and len(it) < 10_000_000
    brute = _Brute(up, it, M)
    rng = np.random.default_rng(6)
    sample = np.concatenate([[_SPLIT], rng.choice(np.unique(it), 20, replace=False)])
    runs = [(dict(), "1"), (dict(), "0"), (dict(column_order=True), "1"), (dict(column_order=True), "0"),
            (dict(any_order=True), "1")]
    first = None
    for kw, mirror in runs:
        where = f"{kw} COOC_SP_MIRROR={mirror}"
        monkeypatch.setenv("COOC_SP_MIRROR", mirror)
        core, res = _count(pkg, torch, up, it, M, **kw)
        with core:
            assert core.last_mirror_rows() == int(mirror), where
            relabelled = not np.array_equal(core.column_order(), np.arange(M))
            assert relabelled == (not kw.get("column_order", False)), where
            rows = _Rows(res, M)
            assert int(rows.nnz.sum()) == res.nnz and int(rows.rowsum.sum()) == res.observed, where
            _check_rows(rows, brute, sample)
            got = core.copy_batch(res.nnz, res.observed)
        if first is None:
            first = got
        else:
            _same(got, first, where)
