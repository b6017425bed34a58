"""The batch planner (k_batch_users .. k_batch_chunks) and k_acc_batch with its compactions at their edges: a
row's contributions around one and two descriptor batches, batches whose group totals sit at the walkers'
range and step boundaries, output rows with entries at the ends of every wave's compaction range, a row that is
exactly one chunk beside a row that is just two, partition blocks and fill loops at their thresholds, and
streaming windows whose descriptors mix old and new positions in one batch.

Every log is dictated, not drawn: tests/_batch_plan_model.py restates the plan from the formulas, the
test_*_log_shapes tests (no GPU) assert through it that each log still reaches the edge it is named for, and the
GPU tests assert that cooc_last_batch_plan reports the model's plan before they compare every row with the
closed form (streaming windows: with the oracle's operator).  The GPU tests need an MI355X and carry the gpu
mark one by one, so that the log-shape tests run wherever the suite runs without a GPU.
"""
import functools

import numpy as np
import pytest

from tests._batch_plan_model import (K_WALKERS, STEP_GROUPS, BatchPlan, batch_db, walker_ranges, walker_steps,
                                     wave_ranges)
from tests._helpers import INT64_MAX, assert_windows_equal

_N_CU = 256  # the CPU shape tests' device: an MI355X (the GPU tests take the count from the device)
_LAYOUTS = ("csr", "dense")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _n_cu(torch):
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def _csr(lists):
    up = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return up, np.concatenate([np.asarray(x, np.int64) for x in lists]).astype(np.int32)


_REFS = {}


def _ref(oracle, key, up, it, M):
    """The closed form of a log, computed once for the module."""
    if key not in _REFS:
        _REFS[key] = oracle.closed_form(up, it, M)
    return _REFS[key]


def _count_and_check(core, oracle, ref, up, it, M, layout, n_cu, where=""):
    """One run on `core`: the reported plan equals the model's, the result equals the closed form."""
    plan = BatchPlan(up, it, M, n_cu)
    got = core.count(up, it)
    assert core.last_batch_plan() == plan.expected(layout == "dense"), f"{where}: plan differs from the model"
    rp, cols, data, rowsums, observed = ref
    assert got.observed == observed, where
    if not np.array_equal(got.row_ptr, rp):
        bad = np.flatnonzero(np.diff(got.row_ptr) != np.diff(rp))
        raise AssertionError(f"{where}: row lengths differ in rows {bad[:8].tolist()}")
    assert np.array_equal(got.cols, cols), where
    if not np.array_equal(got.cnt.astype(np.int64), data):
        k = np.flatnonzero(got.cnt.astype(np.int64) != data)[:8]
        rows = np.searchsorted(rp, k, side="right") - 1
        bad = list(zip(rows.tolist(), cols[k].tolist(), got.cnt[k].tolist(), data[k].tolist()))
        raise AssertionError(f"{where}: counts differ at (row, col, got, want) {bad}")
    assert np.array_equal(got.cnt16, oracle.to_i16(data)), where
    if not np.array_equal(got.rowsum, rowsums):
        bad = np.flatnonzero(got.rowsum != rowsums)
        raise AssertionError(f"{where}: row sums differ in rows {bad[:8].tolist()}")
    assert np.array_equal(got.rowsum32, oracle.to_i32(rowsums)), where
    return plan


# ---- A. descriptor batches -----------------------------------------------------------------------------------
_A_M = (1003, 39000, 40319)
_A_DB = {1003: 1024, 39000: 524, 40319: 85}
_A_LENS = (1, 7, 8, 9, 15, 16, 17)


def _a_targets(M):
    return (0, 7, M // 2, M - 2, M - 1)


def _a_counts(M):
    db = batch_db(M)
    return (db - 1, db, db + 1, 2 * db, 2 * db + 1)


@functools.lru_cache(maxsize=None)
def _batch_log(M):
    """max(3 db + 64, 2000) lists of 1, 7, 8, 9, 15, 16, 17 ids (in turn).  Five target items get exactly db - 1, db,
    db + 1, 2 db and 2 db + 1 contributions: every list with room takes the targets still short of theirs (a list of
    one id takes one, the targets in turn), and each target's first holder holds it twice, two contributions of one
    list.  Everything else is uniform over the other ids, a few per row."""
    db = batch_db(M)
    targets, want = _a_targets(M), _a_counts(M)
    need = [c - 1 for c in want]  # holders: the first one gives two contributions
    first = [True] * 5
    rng = np.random.default_rng(M)
    lists = []
    for u in range(max(3 * db + 64, 2000)):
        l = _A_LENS[u % len(_A_LENS)]
        ids = []
        for k0 in range(5):
            k = (u + k0) % 5
            cost = 2 if first[k] else 1
            if need[k] == 0 or len(ids) + cost > l:
                continue
            ids += [targets[k]] * cost
            first[k] = False
            need[k] -= 1
        fill = rng.integers(8, M - 3, l - len(ids))
        fill += fill >= M // 2  # (not a target)
        lists.append(rng.permutation(np.concatenate([np.asarray(ids, np.int64), fill])))
    assert need == [0] * 5
    return _csr(lists)


@pytest.mark.parametrize("M", _A_M)
def test_batch_log_shapes(M):
    up, it = _batch_log(M)
    plan = BatchPlan(up, it, M, _N_CU)
    db = plan.db
    assert db == _A_DB[M]
    assert set(np.diff(up).tolist()) == set(_A_LENS)
    assert plan.n_split == 0 and plan.n_long == 0
    shapes = ([db - 1], [db], [db, 1], [db, db], [db, db, 1])
    user = np.repeat(np.arange(len(up) - 1), np.diff(up))
    for a, c, shape in zip(_a_targets(M), _a_counts(M), shapes):
        assert plan.c[a] == c
        (chunk,) = plan.batches(a)
        assert [nb for nb, _ in chunk] == shape
        assert sum(g for _, g in chunk) == int(plan.row_groups(a).sum())
        per_list = np.bincount(user[it == a])
        assert int(np.sum(per_list == 2)) == 1 and per_list.max() == 2  # one list holds it twice
        assert int(np.sum(per_list > 0)) == c - 1
    others = np.delete(plan.c, list(_a_targets(M)))
    assert others.max() < db - 1 and (M < 39000 or others.max() < 16)  # sparse beside the targets


@pytest.mark.gpu
@pytest.mark.parametrize("layout", _LAYOUTS)
@pytest.mark.parametrize("M", _A_M)
def test_batch_edges(pkg, oracle, torch_cuda, M, layout):
    """Rows of db - 1, db, db + 1, 2 db and 2 db + 1 contributions at db = 1024, 524 and 85: the descriptor prefetch
    of the next batch (b1 + tid < c.end) with nothing, one descriptor and a whole batch left."""
    up, it = _batch_log(M)
    with pkg.CooccurrenceCore(n_items=M, output=layout) as core:
        _count_and_check(core, oracle, _ref(oracle, ("A", M), up, it, M), up, it, M, layout, _n_cu(torch_cuda))


# ---- B. walker ranges ----------------------------------------------------------------------------------------
_B_M = 1003
_B_TOTALS = {lay: (1, kw - 1, kw, kw + 1, 4095, 4096, 4097, 4096 + kw) for lay, kw in K_WALKERS.items()}
_B_ALL = sorted(set(_B_TOTALS["dense"]) | set(_B_TOTALS["csr"]))
_B_ROW = {g: 10 + 3 * i for i, g in enumerate(_B_ALL)}  # the row whose one batch has g groups
_B_LONG = {"first": 100, "middle": 101, "last": 102}    # rows of 200 one-group lists and one list of 40 groups
_B_POOL = np.arange(200, 1000)
_B_LONG_GROUPS, _B_SHORTS = 40, 200


def _b_list(rng, target, n, edge_cols):
    """A list of n ids: the target once, columns 0 and M - 1 when asked, the rest distinct ids of the pool."""
    ids = [target] + ([0, _B_M - 1] if edge_cols else [])
    assert n >= len(ids)
    return rng.permutation(np.concatenate([ids, rng.choice(_B_POOL, n - len(ids), replace=False)]).astype(np.int64))


def _b_row_lists(rng, g):
    """min(g, 1024) lists with g groups in all: g // c groups each, the first g % c lists one more; a list of k
    groups has 8 k - (i mod 8) ids (k = 4: 25 to 32)."""
    a, c = _B_ROW[g], min(g, 1024)
    out = []
    for i in range(c):
        k = g // c + (1 if i < g % c else 0)
        out.append(_b_list(rng, a, 8 * k - i % 8, i == 0))
    return out


def _b_shorts(rng, a, count):
    """One-group lists of 8, 7, .., 1 ids in turn."""
    return [_b_list(rng, a, 8 - i % 8, False) for i in range(count)]


def _b_long(rng, a):
    return _b_list(rng, a, 8 * _B_LONG_GROUPS - 3, True)


@functools.lru_cache(maxsize=None)
def _walk_log():
    """Every target row is one batch (at most 1,024 lists, each holding the row's item once; the row's first list
    also holds columns 0 and M - 1).  The three long-list rows keep their long list first, in the middle and last
    among their descriptors: first and last by partition blocks (the long list lies a heavy row's lists away from
    the row's short ones, and the scatter orders a row's descriptors by block), the middle one by position."""
    rng = np.random.default_rng(41)
    kd, kc = K_WALKERS["dense"], K_WALKERS["csr"]
    lists = [_b_long(rng, _B_LONG["first"])]
    lists += _b_row_lists(rng, 4096 + kc)
    lists += _b_shorts(rng, _B_LONG["first"], _B_SHORTS)
    for g in (1, kd - 1, kd, kd + 1, kc - 1, kc, kc + 1):
        lists += _b_row_lists(rng, g)
    mid = _b_shorts(rng, _B_LONG["middle"], _B_SHORTS)
    lists += mid[:_B_SHORTS // 2] + [_b_long(rng, _B_LONG["middle"])] + mid[_B_SHORTS // 2:]
    for g in (4095, 4096, 4097):
        lists += _b_row_lists(rng, g)
    lists += _b_shorts(rng, _B_LONG["last"], _B_SHORTS)
    lists += _b_row_lists(rng, 4096 + kd)
    lists.append(_b_long(rng, _B_LONG["last"]))
    return _csr(lists)


def test_walk_log_shapes():
    up, it = _walk_log()
    M = _B_M
    plan = BatchPlan(up, it, M, _N_CU)
    lens = np.diff(up)
    user = np.repeat(np.arange(len(lens)), lens)
    assert plan.db == 1024 and plan.n_split == 0 and plan.B > 8

    def cols_of(a):
        return set(it[np.isin(user, user[it == a])].tolist())

    for lay in _LAYOUTS:
        kw, step = K_WALKERS[lay], STEP_GROUPS[lay]
        assert _B_TOTALS[lay] == (1, kw - 1, kw, kw + 1, 4095, 4096, 4097, 4096 + kw)
        for g in _B_TOTALS[lay]:
            a = _B_ROW[g]
            assert plan.batches(a) == [[(min(g, 1024), g)]], (lay, g)  # one chunk, one batch, g groups
            assert {0, M - 1, a} <= cols_of(a)
            assert int(np.bincount(user[it == a]).max()) == 1
        lo, hi = walker_ranges(kw - 1, lay)
        assert int(np.sum(hi == lo)) == 1 and walker_steps(kw - 1, lay) == 1  # an idle walker
        lo, hi = walker_ranges(1, lay)
        assert int(np.sum(hi > lo)) == 1  # one walker, one lane
        # 4,096 groups: every walker's range is exactly one step; one group more starts a second step
        assert 4096 // kw == step
        lo, hi = walker_ranges(4096, lay)
        assert set((hi - lo).tolist()) == {step} and walker_steps(4095, lay) == 1
        lo, hi = walker_ranges(4097, lay)
        assert sorted(set((hi - lo).tolist())) == [step, step + 1] and walker_steps(4097, lay) == 2
        lo, hi = walker_ranges(4096 + kw, lay)
        assert set((hi - lo).tolist()) == {step + 1}
    a = _B_ROW[4096]
    assert plan.c[a] == 1024 and set(lens[user[it == a]].tolist()) == set(range(25, 33))
    # the long-list rows: 1-group lists and one list over at least 3 walker ranges, at its place in the batch
    for where, a in _B_LONG.items():
        g = plan.row_groups(a)
        assert len(g) == _B_SHORTS + 1 and sorted(set(g.tolist())) == [1, _B_LONG_GROUPS]
        assert {0, M - 1, a} <= cols_of(a)
        k = int(np.flatnonzero(g == _B_LONG_GROUPS)[0])
        assert k == {"first": 0, "middle": _B_SHORTS // 2, "last": _B_SHORTS}[where]
        ex, total = int(g[:k].sum()), int(g.sum())
        for lay in _LAYOUTS:
            lo, _ = walker_ranges(total, lay)
            assert int(np.sum((lo >= ex) & (lo < ex + _B_LONG_GROUPS))) >= 3  # walkers starting inside the list
        blocks = plan.block_of(plan.row_positions(a))
        if where == "first":
            assert blocks[0] < blocks[1:].min()
        elif where == "last":
            assert blocks[-1] > blocks[:-1].max()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", _LAYOUTS)
def test_walker_edges(pkg, oracle, torch_cuda, layout):
    """Single-batch rows of 1, kW - 1, kW, kW + 1, 4095, 4096, 4097 and 4096 + kW groups for both walker counts
    (64 dense, 128 CSR), and rows whose batch holds one list that several walkers start in (s_qstart written by
    one segment for several walkers) as its first, a middle and its last descriptor."""
    up, it = _walk_log()
    with pkg.CooccurrenceCore(n_items=_B_M, output=layout) as core:
        _count_and_check(core, oracle, _ref(oracle, "B", up, it, _B_M), up, it, _B_M, layout, _n_cu(torch_cuda))


# ---- C. row output -------------------------------------------------------------------------------------------
_C_M = (61, 62, 255, 256, 257, 1003, 4096, 4097)  # (62: the only M % 4 == 2 among them)


def _c_edges(M):
    """lo, lo + 3, hi - 4 and hi - 1 of every wave's range, 256-aligned (compact_row_ranges4) and 64-aligned
    (k_pack_dense, compact_row_ranges), where they lie inside the range."""
    e = set()
    for align in (256, 64):
        for lo, hi in wave_ranges(M, align):
            e |= {b for b in (lo, lo + 3, hi - 4, hi - 1) if lo <= b < hi}
    return sorted(e)


def _c_rows(M):
    """(x, y, z): the rows with one entry at M - 1, with entries at M - 4 .. M - 1, and with the edge columns."""
    edges = set(_c_edges(M))
    return tuple([b for b in range(4, M - 4) if b not in edges][:3])


@functools.lru_cache(maxsize=None)
def _output_log(M, mirrored=False):
    """The count matrix is symmetric, so the full row is row M - 1 and every other row has column M - 1: a list
    {b, M - 1} per item b, {M - 1, M - 1} for the diagonal, {y, M - 1, .., M - 4}, and {z} with the edge columns
    (M - 1 among them).  mirrored: the same log with item b renamed M - 1 - b."""
    x, y, z = _c_rows(M)
    lists = [[b, M - 1] for b in range(M - 1) if b not in (y, z)]
    lists.append([M - 1, M - 1])
    lists.append([y, M - 1, M - 2, M - 3, M - 4])
    lists.append([z] + _c_edges(M))
    up, it = _csr(lists)
    return up, (M - 1 - it).astype(np.int32) if mirrored else it


@pytest.mark.parametrize("M", _C_M)
def test_output_log_shapes(oracle, M):
    assert {m % 4 for m in _C_M} == {0, 1, 2, 3}
    assert len(wave_ranges(61, 256)) == 1 and len(wave_ranges(256, 256)) == 1 and len(wave_ranges(257, 256)) == 2
    assert wave_ranges(257, 256)[1] == (256, 257) and wave_ranges(4097, 256)[-1] == (4096, 4097)  # a partial quad
    assert all((hi - lo) % 256 == 0 for lo, hi in wave_ranges(4096, 256))
    up, it = _output_log(M)
    x, y, z = _c_rows(M)
    edges = _c_edges(M)
    assert M - 1 in edges and 0 in edges and not {x, y, z} & (set(edges) | set(range(M - 4, M)))
    for align in (256, 64):
        for lo, hi in wave_ranges(M, align):
            assert {lo, hi - 1} <= set(edges) and (hi - lo < 4 or {lo + 3, hi - 4} <= set(edges))
    rp, cols, data, _, _ = _ref(oracle, ("C", M, False), up, it, M)

    def row(a):
        return cols[rp[a]:rp[a + 1]].tolist()

    assert row(M - 1) == list(range(M))           # every column
    assert row(x) == [M - 1]                      # the last column alone
    assert row(y) == [M - 4, M - 3, M - 2, M - 1]  # the last quad (M % 4 == 0) or across two
    assert row(z) == edges
    plan = BatchPlan(up, it, M, _N_CU)
    assert plan.n_split == 0 and plan.c[M - 1] == M + 1


@pytest.mark.gpu
@pytest.mark.parametrize("layout", _LAYOUTS)
@pytest.mark.parametrize("M", _C_M)
def test_output_edges(pkg, oracle, torch_cuda, M, layout):
    """A full row, a row with column M - 1 alone, a row with entries at the first and last quad of every wave's
    compaction range and a row with the last four columns, for M % 4 = 0 .. 3; then the mirrored log (row a as
    row M - 1 - a) on the same context: a counter or an output row left from the first run shows in the second."""
    n_cu = _n_cu(torch_cuda)
    with pkg.CooccurrenceCore(n_items=M, output=layout) as core:
        for mirrored in (False, True, False):
            up, it = _output_log(M, mirrored)
            _count_and_check(core, oracle, _ref(oracle, ("C", M, mirrored), up, it, M), up, it, M, layout, n_cu,
                             where=f"mirrored={mirrored}")


# ---- D. chunks -----------------------------------------------------------------------------------------------
_D_M, _D_LISTS = 1003, 131073


@functools.lru_cache(maxsize=None)
def _chunk_log():
    """131,073 lists of 25 to 32 distinct ids (pad8 = 32 for every list, so lbar = 32 exactly): item 0 in the first
    131,072, c lbar = 2^22, one chunk of 128 full batches; item 1 in all of them, two chunks."""
    u = np.arange(_D_LISTS, dtype=np.int64)
    lens = 25 + u % 8
    up = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    user = np.repeat(u, lens)
    k = np.arange(int(up[-1]), dtype=np.int64) - up[user]
    it = 2 + (user * 31 + k * 3) % 1001  # distinct inside a list: 3 and 1001 are coprime
    p0 = u % lens
    p1 = (p0 + 1 + (u // 8) % (lens - 1)) % lens  # another place
    it[up[:-2] + p0[:-1]] = 0
    it[up[:-1] + p1] = 1
    return up, it.astype(np.int32)


def test_chunk_log_shapes():
    up, it = _chunk_log()
    plan = BatchPlan(up, it, _D_M, _N_CU)
    lens = np.diff(up)
    assert lens.min() == 25 and lens.max() == 32
    assert plan.lbar == 32.0 and plan.sum_lpl == 32 * plan.n
    assert plan.c[0] == 131072 and plan.c[1] == 131073 and float(plan.c[0]) * plan.lbar == float(1 << 22)
    assert plan.nch[:2].tolist() == [1, 2] and plan.n_split == 1 and plan.n_chunks == int(np.sum(plan.c > 0)) + 1
    (chunk,) = plan.batches(0)
    assert chunk == [(1024, 4096)] * 128
    assert plan.chunks(1) == [(0, 65536), (65536, 131073)]
    assert [nb for nb, _ in plan.batches(1)[1]][-2:] == [1024, 1]  # the second chunk ends in a batch of one
    assert plan.B == _N_CU and plan.n // plan.B > 3 * 4096  # several 4,096-steps per block of hist / scatter


@pytest.mark.gpu
@pytest.mark.parametrize("layout", _LAYOUTS)
def test_chunk_edges(pkg, oracle, torch_cuda, layout):
    """c lbar = 2^22 exactly (one chunk) beside one contribution more (two chunks: global atomics and
    k_dense_split_check in the dense layout, a staging row and k_finalize_split in the CSR layout)."""
    up, it = _chunk_log()
    with pkg.CooccurrenceCore(n_items=_D_M, output=layout) as core:
        _count_and_check(core, oracle, _ref(oracle, "D", up, it, _D_M), up, it, _D_M, layout, _n_cu(torch_cuda))


# ---- E. planner passes ---------------------------------------------------------------------------------------
_E_M = 257
_E_LONG = {1500: 2047, 2500: 2048, 3500: 2049}  # list index -> length


@functools.lru_cache(maxsize=None)
def _planner_log():
    """12,000 lists of 1, 2, 3, 4, 5 ids in turn (starts at every offset mod 4 for every length) and, between
    them and past the first 4,097 interactions, lists of 2,047, 2,048 and 2,049 ids."""
    rng = np.random.default_rng(53)
    lens = [_E_LONG.get(j, 1 + j % 5) for j in range(12000)]
    up = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return up, rng.integers(0, _E_M, int(up[-1])).astype(np.int32)


def _truncate(up, it, n):
    up_t = np.concatenate([up[up < n], [n]]).astype(np.int64)
    return up_t, it[:n]


def _straddled(up_t, n, B):
    """Every inner block boundary n b // B lies strictly inside a list."""
    return all(n * b // B not in set(up_t.tolist()) for b in range(1, B))


@functools.lru_cache(maxsize=None)
def _planner_cases():
    """(n, B on a device of at least 9 CUs): 4095, 4096, 4097, and the first n of B = 7, 8 and 9 at which a list
    straddles every block boundary."""
    up, it = _planner_log()
    cases = [(4095, 1), (4096, 2), (4097, 2)]
    for B in (7, 8, 9):
        cases.append(next((n, B) for n in range((B - 1) * 4096 + 1, B * 4096)
                          if _straddled(_truncate(up, it, n)[0], n, B)))
    return tuple(cases)


def test_planner_log_shapes():
    up, it = _planner_log()
    lens = np.diff(up)
    assert {(int(s) % 4, int(l)) for s, l in zip(up[:-1], lens) if l <= 5} == {(s, l) for s in range(4)
                                                                               for l in range(1, 6)}
    for j, l in _E_LONG.items():
        assert lens[j] == l and lens[j - 1] <= 5 and lens[j + 1] <= 5 and up[j] > 4097
    cases = _planner_cases()
    assert [b for _, b in cases] == [1, 2, 2, 7, 8, 9] and [n for n, _ in cases[:3]] == [4095, 4096, 4097]
    for n, B in cases:
        up_t, it_t = _truncate(up, it, n)
        plan = BatchPlan(up_t, it_t, _E_M, _N_CU)
        assert plan.B == B and plan.n == n and _straddled(up_t, n, B)
        assert plan.n_long == (1 if B >= 7 else 0) and plan.max_len == (2049 if B >= 7 else 5)
        if B >= 7:  # all three long lists, whole
            assert {2047, 2048, 2049} <= set(np.diff(up_t).tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("layout", _LAYOUTS)
@pytest.mark.parametrize("case", range(6))
def test_planner_pass_edges(pkg, oracle, torch_cuda, case, layout):
    """B = 1 -> 2 at n = 4096 and B = 7, 8, 9 (k_batch_colscan's unroll by 8 and its tail), lists across every
    block boundary, k_batch_fill's head / 16-B / tail loops at every start offset, and lists of 2,047, 2,048 and
    2,049 ids (only the last goes to k_batch_fill_long)."""
    up, it = _planner_log()
    n, B = _planner_cases()[case]
    up_t, it_t = _truncate(up, it, n)
    with pkg.CooccurrenceCore(n_items=_E_M, output=layout) as core:
        plan = _count_and_check(core, oracle, _ref(oracle, ("E", n), up_t, it_t, _E_M), up_t, it_t, _E_M, layout,
                                _n_cu(torch_cuda))
    if plan.B != B:  # (the comparison above ran with the B this device forms)
        pytest.skip(f"a device of {plan.n_cu} CUs forms B = {plan.B}, not {B}")


# ---- F. streaming windows ------------------------------------------------------------------------------------
_F_M, _F_HOT, _F_BOTH, _F_TWICE = 1003, 777, 500, 600
_F_OLD, _F_NEW, _F_REPL = (0, 1, 7, 8, 9, 16), (1, 7, 8, 9, 17), 50


@functools.lru_cache(maxsize=None)
def _stream_log():
    """1,500 users, 50 per (old, new) in {0, 1, 7, 8, 9, 16} x {1, 7, 8, 9, 17}: window 0 brings a user's old part,
    window 1 its new part, window 2 a third part to every third user.  The hot item sits in the old part of the
    even users and in the new part of the odd ones, so its row has more than 1,024 contributions in window 1, old
    and new positions alternating.  One user has an item in both parts, one has an item twice in its new part.
    -> per window (users, items) in arrival order."""
    rng = np.random.default_rng(67)
    combos = [(o, nw) for o in _F_OLD for nw in _F_NEW]
    wins = [([], []), ([], []), ([], [])]
    for u in range(len(combos) * _F_REPL):
        o, nw = combos[u % len(combos)]
        parts = [rng.integers(2, _F_M - 1, o), rng.integers(2, _F_M - 1, nw),
                 rng.integers(2, _F_M - 1, 1 + u % 9 if u % 3 == 0 else 0)]
        for p in parts:
            p[p == _F_HOT] = _F_HOT + 1
        if u % 2 == 0 and o > 0:
            parts[0][u % o] = _F_HOT
        if u % 2 == 1:
            parts[1][u % nw] = _F_HOT
        if (o, nw) == (7, 7) and u < len(combos):
            parts[0][3] = parts[1][5] = _F_BOTH
        if (o, nw) == (8, 9) and u < len(combos):
            parts[1][2] = parts[1][7] = _F_TWICE
        for w, p in enumerate(parts):
            wins[w][0].append(np.full(len(p), u, np.int32))
            wins[w][1].append(p.astype(np.int32))
    return tuple((np.concatenate(us), np.concatenate(its)) for us, its in wins)


def _window_csr(wins, w):
    """Window w as the planner sees it: the active users' histories after the window and their lengths before."""
    hist = {}
    for k in range(w + 1):
        before = {u: len(h) for u, h in hist.items()}
        for u, i in zip(wins[k][0].tolist(), wins[k][1].tolist()):
            hist.setdefault(u, []).append(i)
    active = sorted(set(wins[w][0].tolist()))
    up, it = _csr([hist[u] for u in active])
    return up, it, np.array([before.get(u, 0) for u in active], np.int64)


def test_stream_log_shapes():
    wins = _stream_log()
    up, it, old = _window_csr(wins, 1)
    plan = BatchPlan(up, it, _F_M, _N_CU, old=old)
    assert {(int(o), int(l - o)) for o, l in zip(old, np.diff(up))} == {(o, nw) for o in _F_OLD for nw in _F_NEW}
    hot_old = plan.row_old(_F_HOT)
    assert len(hot_old) > plan.db == 1024 and plan.nch[_F_HOT] == 1
    first = hot_old[:plan.db]
    assert 400 < int(first.sum()) < 624 and int(np.sum(first[1:] != first[:-1])) > 500  # mixed in one batch
    user = np.repeat(np.arange(len(old)), np.diff(up))
    pos = np.arange(len(it)) - up[user]
    both = user[(it == _F_BOTH) & (pos < old[user])]
    assert len(set(both.tolist()) & set(user[(it == _F_BOTH) & (pos >= old[user])].tolist())) >= 1
    twice = np.bincount(user[(it == _F_TWICE) & (pos >= old[user])])
    assert twice.max() == 2
    up2, it2, old2 = _window_csr(wins, 2)
    assert len(old2) == 500 and old2.min() >= 1 and len(_window_csr(wins, 0)[2]) == 1250
    assert BatchPlan(up2, it2, _F_M, _N_CU, old=old2).sum_l2 > 0


@pytest.mark.gpu
def test_stream_window_edges(pkg, oracle, torch_cuda):
    """Three windows through run_window (planner="auto"): every window's plan equals the model's over the active
    users' (old, new) parts, and its delta rows, row sums, observed and top-k equal the oracle operator's; then the
    global rows and row sums."""
    wins = _stream_log()
    n_cu = _n_cu(torch_cuda)
    op = pkg.NonSampledUserInteractionCounterOneInputStreamOperator(1, "SECONDS", n_items=_F_M, top_k=5,
                                                                    planner="auto")
    ref = oracle.OracleStream(1000, topk=5)
    for w, (users, items) in enumerate(wins):
        ts = np.full(len(users), 1000 * w + 500, np.int64)
        op.process_elements(users, items, ts)
        ref.process_elements(users, items, ts)
        wm = 1000 * (w + 1) - 1 if w < 2 else INT64_MAX
        got, want = op.process_watermark(wm), ref.process_watermark(wm)
        assert len(got) == len(want) == 1
        up, it, old = _window_csr(wins, w)
        assert op.core.last_batch_plan() == BatchPlan(up, it, _F_M, n_cu, old=old).expected(False), f"window {w}"
        assert_windows_equal(got[0], want[0])
    assert op.accumulators() == ref.counters()
    rows, rp, cols, exact, v16 = ref.global_rows()
    for r, a in enumerate(rows):
        c, n, n16 = op.core.global_row(int(a))
        assert np.array_equal(c, cols[rp[r]:rp[r + 1]])
        assert np.array_equal(n.astype(np.int64), exact[rp[r]:rp[r + 1]])
        assert np.array_equal(n16, v16[rp[r]:rp[r + 1]])
    gi, gv32, gex = ref.global_rowsums()
    ex, v32 = op.core.global_rowsums()
    assert np.array_equal(ex[gi], gex) and np.array_equal(v32[gi], gv32)
    op.close()


# ---- G. the row order's sort: equal contribution counts ------------------------------------------------------
_G_M = 4097  # one row more than a radix tile holds
_G_HOT = 300


@functools.lru_cache(maxsize=None)
def _ties_log():
    """Item a < 4,096 holds 1 + a mod 4 contributions, every 64th of them none, item 4,096 holds 300: the multiset,
    shuffled, in lists of 8 ids."""
    a = np.arange(_G_M - 1, dtype=np.int64)
    ids = np.concatenate([np.repeat(a, np.where(a % 64 == 0, 0, 1 + a % 4)), np.full(_G_HOT, _G_M - 1, np.int64)])
    ids = np.random.default_rng(4097).permutation(ids)
    return _csr([ids[k:k + 8] for k in range(0, len(ids), 8)])


def test_ties_log_shapes():
    up, it = _ties_log()
    plan = BatchPlan(up, it, _G_M, _N_CU)
    assert plan.M == 4097 > 4096 and plan.n < 1 << 14  # the sort: two tiles of rows, keys of at most 14 bits
    values, rows = np.unique(plan.c, return_counts=True)
    assert values.tolist() == [0, 1, 2, 3, 4, _G_HOT] and rows.tolist() == [64, 960, 1024, 1024, 1024, 1]
    assert plan.c[_G_M - 1] == _G_HOT and plan.c[0] == 0  # the heaviest row is the last, an empty one the first
    assert plan.n_chunks == _G_M - 64 and plan.n_split == 0


@pytest.mark.gpu
@pytest.mark.parametrize("layout", _LAYOUTS)
def test_row_order_with_ties(pkg, oracle, torch_cuda, layout):
    """4,097 rows of which about a thousand each share a contribution count of 1, 2, 3 and 4, 64 empty rows among
    them and the heaviest row last: the chunk plan's descending sort over two tiles.  cooc_last_batch_plan reports
    the plan's totals and not the order of its chunks, so what shows here is that the order is a permutation of the
    rows (the chunk count, every row against the closed form); that equal keys keep their input order, ascending
    row id, is pinned for this shape in tests/test_gpu_radix.py."""
    up, it = _ties_log()
    with pkg.CooccurrenceCore(n_items=_G_M, output=layout) as core:
        _count_and_check(core, oracle, _ref(oracle, "G", up, it, _G_M), up, it, _G_M, layout, _n_cu(torch_cuda))


# ---- the accessor itself -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_last_batch_plan_zero_states(pkg, torch_cuda):
    """Zeros before any run of the batch planner and after a large-universe run (here: the large-universe planner
    chosen for a small universe)."""
    up, it = _batch_log(1003)
    with pkg.CooccurrenceCore(n_items=1003, output="csr") as core:
        assert core.last_batch_plan() == (0,) * 8
        core.count(up, it)
        assert core.last_batch_plan() == BatchPlan(up, it, 1003, _n_cu(torch_cuda)).expected(False)
    with pkg.CooccurrenceCore(n_items=1003, planner="large") as core:
        core.count(up, it)
        assert core.last_batch_plan() == (0,) * 8
