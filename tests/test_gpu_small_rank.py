"""The ranking primitive of the small rows' radix sort (wave_match, cooc_sparse.h) where it is used:
block_radix_sort under k_sp_small (rows of 257..4,096 pairs) and under k_srb_row (planner="sort": every whole
row).  The planner's k_rdx_scatter (cooc_radix.h) keeps its own ranking loop (wave_match measured slower there,
DESIGN.md §4); the radix cases at the end cover the lane patterns tests/test_gpu_radix.py lacks for whichever
ranking that kernel uses.

Every log is a handful of users over 65,536 items with the ids kept (column_order=True: no relabel), so tile 0 is
the ids below 16,384 and a key has 16 bits: two 7-bit passes and one of 2 bits.  65,536 and not the smallest large
universe (40,320) so that n_items - 1 has every bit set: the largest digit of every pass.  One case runs at 2^20
items, the largest universe (20 bits: digits 127, 127 and 63 for the last column).

A row fed by one list sees that list's tile-0 ids first, in list order, then its other ids: the patterns below are
aimed at lanes of the first pass's ranking steps that way (a step ranks 64 consecutive positions; steps start at
multiples of 64), but only results are asserted: every row of the log, entry by entry, against rows summed
directly from the lists (a dense count matrix over the ids that occur), the named rows also against
tests.test_gpu_sparse._Brute, and cooc_verify_batch clean.  That the named rows are k_sp_small's (pair work
257..4,096, computed on the host as test_gpu_region_grow.py does) is asserted on any machine
(test_named_rows_are_small_rows).
"""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_dense_stores import _count
from tests.test_gpu_mid4 import _csr
from tests.test_gpu_sparse import _Brute, _check_rows, _d2h, _Rows

_TW = 16384
_M = 65536
_A = 40_000  # a row above tile 0: in a list of tile-0 ids it is gathered last


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _pair_work(up, it, M):
    lens = np.diff(up)
    return np.bincount(it, weights=np.repeat(lens, lens).astype(np.float64), minlength=M).astype(np.int64)


def _distinct(rng, n, lo=0, hi=_TW, avoid=()):
    """n distinct ids of [lo, hi) in random order, none of avoid."""
    ids = np.setdiff1d(np.arange(lo, hi), np.asarray(avoid, np.int64))
    return rng.permutation(ids)[:n].astype(np.int64)


def _with_tails(keys):
    """The tile-0 pattern followed by its copy above tile 0 (id + 16,384 (1 + id % 3): equal ids stay equal), so
    half of the row's keys have non-zero digits in the last pass."""
    keys = np.asarray(keys, np.int64)
    return np.concatenate([keys, keys + _TW * (1 + keys % 3)])


# ---- the cases: name -> (lists, named rows, n_items) ---------------------------------------------------------------

def _size_case(W, tails):
    """A row of exactly W pairs: one list of W ids holding the row's id once.  Up to 576 the other ids are
    distinct; above, 512 ids eight times each, shuffled (their rows are mid rows)."""
    rng = np.random.default_rng(W + (1 << 20) * tails)
    n = W - 1
    if tails:
        # the row's own column among the tail keys: an id of tile 2, not one of the copies' (id % 3 == 1 there)
        half = n // 2
        base = _distinct(rng, half if W <= 576 else 256)
        p0 = base if W <= 576 else rng.permutation(np.repeat(base, -(-half // 256)))[:half]
        p1 = _with_tails(p0)[len(p0):]
        own = 2 * _TW + 2 + 3 * 100  # (id - 2 TW) % 3 == 2: no copy lands there
        extra = _distinct(rng, n - 2 * half, avoid=p0)
        lst = np.concatenate([p0, extra, p1[:len(p1) // 2], [own], p1[len(p1) // 2:]])
        a = own
    else:
        base = _distinct(rng, n if W <= 576 else 512)
        p0 = base if W <= 576 else rng.permutation(np.repeat(base, 8))[:n]
        lst, a = np.concatenate([p0, [_A]]), _A
    assert len(lst) == W
    return [lst], [a], _M


def _half_case(kind, shifted, tails):
    """Equal columns at chosen lanes of one ranking step, every other key distinct.  W = 616: P = 128, two steps
    per wave, the last wave's last step holds lanes 0..39.  shifted: the pattern sits in that step, else in the
    first step of wave 0."""
    rng = np.random.default_rng(sum(map(ord, kind)) + 1000 * shifted + 2000 * tails)
    n = 615 if not tails else 307  # + the row's id; with tails the pattern is half of the row
    W1 = n  # tile-0 keys
    step0 = 64 * ((W1 - 1) // 64) if shifted else 0
    last = min(63, W1 - 1 - step0)  # the step's last lane
    assert last >= 38
    lanes = {"31|32": [31, 32], "0|last": [0, last], "0|32|last": [0, 32, last], "high only": [33, 36, last],
             "whole step": list(range(last + 1))}[kind]
    keys = _distinct(rng, n)
    keys[[step0 + x for x in lanes]] = keys[step0 + lanes[0]]
    if tails:
        own = 2 * _TW + 2 + 3 * 100
        up = _with_tails(keys)[n:]
        lst, a = np.concatenate([keys, up[:150], [own], up[150:]]), own
    else:
        lst, a = np.concatenate([keys, [_A]]), _A
    return [lst], [a], _M


def _digit_case(kind):
    rng = np.random.default_rng(sum(map(ord, kind)))
    M = _M
    if kind.startswith("one column"):
        # 64 copies of one id: the row's 4,096 keys are its own column, one digit holds everything in every pass
        # and every wave's counter of it reaches 512 (rank 511 under digit 127 in one, two or three passes)
        M = 1 << 20 if kind.endswith("2^20 - 1") else _M
        c = {"one column 127": 127, "one column 16383": 16383, "one column n_items - 1": _M - 1,
             "one column 2^20 - 1": (1 << 20) - 1, "one column 5": 5}[kind]
        return [np.full(64, c)], [c], M
    if kind.startswith("two columns"):
        # 1,000 keys over exactly two columns that differ in one bit (the row's id is gathered last, apart)
        bit = int(kind.split()[-1])
        c = np.array([5, 5 | (1 << bit)])
        keys = c[rng.integers(0, 2, 999)]
        if bit == 15:
            # (the upper column lies above tile 0: its keys come after the tile-0 ones; the row is of tile 1)
            return [np.concatenate([keys, [_TW + 7]])], [_TW + 7], M
        return [np.concatenate([keys, [_A]])], [_A], M
    if kind == "ascending":  # 4,096 distinct tile-0 ids in order: every id's row is a small row of these keys
        return [np.sort(_distinct(rng, 4096))], [], M
    if kind == "descending":
        return [np.sort(_distinct(rng, 4096))[::-1]], [], M
    if kind == "alternating":
        # the first pass's digits alternate 0 and 127 lane by lane: 256 ids of low bits 0 or 127, 16 times each
        j = rng.integers(0, 128, 4095)
        keys = (j << 7) | np.where(np.arange(4095) % 2 == 0, 0, 127)
        return [np.concatenate([keys, [_A]])], [_A], M
    raise KeyError(kind)


_SIZES = [257, 511, 512, 513, 575, 576, 4032, 4095, 4096]
_HALVES = ["31|32", "0|last", "0|32|last", "whole step", "high only"]
_DIGITS = ["one column 5", "one column 127", "one column 16383", "one column n_items - 1", "one column 2^20 - 1",
           "two columns bit 6", "two columns bit 13", "two columns bit 15", "ascending", "descending", "alternating"]

_CASES = {}
for _w in _SIZES:
    for _t in (False, True):
        _CASES[f"size {_w}{' tails' if _t else ''}"] = (_size_case, (_w, _t))
for _k in _HALVES:
    for _s in (False, True):
        for _t in (False, True):
            _CASES[f"lanes {_k}{' shifted' if _s else ''}{' tails' if _t else ''}"] = (_half_case, (_k, _s, _t))
for _k in _DIGITS:
    _CASES[_k] = (_digit_case, (_k,))
# through k_srb_row (planner="sort"): the sizes and the half-mask patterns
_SRB = [n for n in _CASES if n.startswith(("size", "lanes")) and "tails" not in n] + ["size 4096 tails", "lanes 31|32 tails"]
# both emission orders
_ANY = ["size 513", "size 4096 tails", "lanes 0|32|last", "lanes 31|32 shifted tails", "one column 127",
        "two columns bit 13", "alternating"]

_BUILT = {}


def _case(name):
    """(up, it, M, named rows, pair work), built once."""
    if name not in _BUILT:
        fn, args = _CASES[name]
        lists, named, M = fn(*args)
        up, it = _csr([np.asarray(x, np.int64) for x in lists])
        W = _pair_work(up, it, M)
        if not named:  # every row of the log
            named = np.flatnonzero(W > 0).tolist()
        _BUILT[name] = (up, it, M, named, W)
    return _BUILT[name]


def _expected(up, it):
    """The whole count over the ids that occur: (ids ascending, C) with C = sum_u c_u c_u^T - diag(sum_u c_u)."""
    ids, inv = np.unique(it, return_inverse=True)
    D = len(ids)
    C = np.zeros((D, D), np.int64)
    tot = np.zeros(D, np.int64)
    for u in range(len(up) - 1):
        c = np.bincount(inv[up[u]:up[u + 1]], minlength=D).astype(np.int64)
        nz = np.flatnonzero(c)
        C[np.ix_(nz, nz)] += np.outer(c[nz], c[nz])
        tot += c
    C[np.arange(D), np.arange(D)] -= tot
    return ids, C


@pytest.mark.parametrize("name", list(_CASES))
def test_named_rows_are_small_rows(name):
    """No GPU: the rows each case is about have 257..4,096 pairs (k_sp_small's class), the size cases exactly W."""
    up, it, M, named, W = _case(name)
    assert len(named) >= 1 and int(it.max()) < M
    assert np.all((W[named] > 256) & (W[named] <= 4096)), W[named]
    if name.startswith("size"):
        assert W[named[0]] == int(name.split()[1])
    if name.startswith("one column"):
        assert W[named[0]] == 4096 and len(np.unique(it)) == 1


def _run(pkg, torch, name, **kw):
    up, it, M, named, W = _case(name)
    core, res = _count(pkg, torch, up, it, M, column_order=True, **kw)
    with core:
        lens = np.diff(up)
        assert res.observed == int(np.sum(lens * (lens - 1)))
        chk = core.verify_batch()
        assert chk["rows_bad_sum"] == 0 and chk["rows_bad_entries"] == 0
        assert chk["sum_counts"] == chk["sum_rowsums"] == res.observed
        rows = _Rows(res, M)
        got = core.copy_batch(res.nnz, res.observed)
        sort_rows = core.last_sort_rows()[0]
        # the named rows against the lists, through the device rows ...
        _check_rows(rows, _Brute(up, it, M), named[:8] + named[-8:])
        # ... which are in column order on the device whatever the flags (k_sp_small and k_srb_row write sorted runs)
        for a in named[:8]:
            col = _d2h(res.col, int(rows.nnz[a]), np.int32, int(rows.base[a]))
            assert np.all(np.diff(col) > 0), f"row {a} is not in column order on the device"
    # every row, entry by entry
    ids, C = _expected(up, it)
    r, c = np.nonzero(C)
    want_ptr = np.concatenate([[0], np.cumsum(np.bincount(ids[r], minlength=M))]).astype(np.int64)
    assert np.array_equal(got.row_ptr, want_ptr), "row sizes differ"
    g_cols, g_cnt = got.cols.astype(np.int64), got.cnt.astype(np.int64)
    if kw.get("any_order"):  # (rows of the hash chunks come in no order)
        o = np.lexsort((g_cols, np.repeat(np.arange(M), np.diff(got.row_ptr))))
        g_cols, g_cnt = g_cols[o], g_cnt[o]
    assert np.array_equal(g_cols, ids[c]), "columns differ"
    assert np.array_equal(g_cnt, C[r, c]), "counts differ"
    assert np.array_equal(got.rowsum[ids], C.sum(axis=1))
    return sort_rows, int(np.count_nonzero(W))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_CASES))
def test_small_rows_vs_lists(pkg, torch_cuda, name):
    _run(pkg, torch_cuda, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _ANY)
def test_small_rows_any_order(pkg, torch_cuda, name):
    """any_order=True against the same expectation as any_order=False (the sorted rows are in column order under
    both flags)."""
    _run(pkg, torch_cuda, name, any_order=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _SRB)
def test_sort_path_rows_vs_lists(pkg, torch_cuda, name):
    """COOC_FLAG_SORT_ROWS: every whole row through k_srb_row, whose bucket groups go through
    block_radix_sort<1024> (16 waves, four steps each)."""
    sort_rows, n_rows = _run(pkg, torch_cuda, name, planner="sort")
    assert sort_rows >= 1 and sort_rows <= n_rows


# ---- the planner's sort (k_rdx_scatter): what tests/test_gpu_radix.py lacks for the primitive ------------------------

def _radix(torch, keys, bit0, bit1):
    from flink_cooccurrence_amd import _lib

    lib = _lib.load()
    vals = np.arange(keys.size, dtype=np.uint32)
    kin = torch.from_numpy(keys).cuda()
    vin = torch.from_numpy(vals.view(np.int32)).cuda()
    kout, vout = torch.empty_like(kin), torch.empty_like(vin)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.cooc_selftest_radix(ctypes.c_void_p(kin.data_ptr()), ctypes.c_void_p(vin.data_ptr()),
                                 ctypes.c_void_p(kout.data_ptr()), ctypes.c_void_p(vout.data_ptr()), keys.size,
                                 keys.itemsize, bit0, bit1, 0, stream)
    assert rc == 0, lib.cooc_last_error(None)
    field = (keys.astype(np.uint64) >> np.uint64(bit0)) & np.uint64((1 << (bit1 - bit0)) - 1)
    perm = np.argsort(field, kind="stable")
    assert np.array_equal(kout.cpu().numpy(), keys[perm]), "keys differ"
    assert np.array_equal(vout.cpu().numpy().view(np.uint32), vals[perm]), "values differ (stability)"


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [(31, 32), (0, 63), (0, 32, 63), (33, 40, 63)])
@pytest.mark.parametrize("n", [4096 + 1024 + 64, 4096 + 1024 + 40])
def test_radix_equal_digits_across_the_mask_halves(pkg, torch_cuda, lanes, n):
    """32-bit keys, all distinct in every 8-bit digit of a ranking step (64 consecutive keys) but for equal keys at
    the given lanes of one step: the first of the tile, and the last of the input (partly filled at n = ...40: the
    lanes above its end are dropped)."""
    rng = np.random.default_rng(n + sum(lanes))
    keys = np.zeros(n, np.uint32)
    for s in range(0, n, 64):  # per step: 64 distinct bytes, the same in all four digits
        b = rng.permutation(256)[:min(64, n - s)].astype(np.uint32)
        keys[s:s + 64] = b | (b << 8) | (b << 16) | (b << 24)
    for s in (0, 64 * ((n - 1) // 64)):
        ln = [x for x in lanes if s + x < n]
        keys[[s + x for x in ln]] = keys[s + ln[0]]
    _radix(torch_cuda, keys, 0, 32)


@pytest.mark.gpu
def test_radix_tile_of_equal_keys(pkg, torch_cuda):
    """A whole 4,096-key tile of one key between two tiles of random ones: a wave's counter of the digit reaches
    1,024 in every pass."""
    rng = np.random.default_rng(4096)
    keys = rng.integers(0, 1 << 32, 3 * 4096, dtype=np.uint64).astype(np.uint32)
    keys[4096:8192] = 0xA5C3FF00
    _radix(torch_cuda, keys, 0, 32)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4096, 10_000])
def test_radix_four_bit_last_pass(pkg, torch_cuda, n):
    """20 bits: two 8-bit passes and a last one of 4 bits, whose high digit bits are zero in every lane; bits above
    the range are set and must not count."""
    rng = np.random.default_rng(n)
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    keys[: n // 2] |= np.uint32(0xF0000)  # half of the keys: the last pass's largest digit
    _radix(torch_cuda, keys, 0, 20)
    _radix(torch_cuda, keys, 16, 20)  # the 4-bit pass alone
