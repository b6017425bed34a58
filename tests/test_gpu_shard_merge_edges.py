"""The owner's merge of partial rows (cooc_shard.hip: k_merge_rows in both forms, and k_merge_keys, the radix sort
and sum by key of cooc_radix.h, k_merge_rows_from_keys) and the partition pack, at their edges: the dense merge's
wave ranges and the largest LDS row, a workgroup's second and later rows, the sorted merge around row counts and
columns of a power of two and around the tiles of its sum by key, both merges on one input, uint32 overflow, signed
nets on both sides of their own threshold, and the pack round trip on real counts with parts that own nothing.

Every input of groups A to F and H is dictated (tests/_shard_cases.py) and goes straight into merge_partitions as device
tensors, in a context of the n_items under test that has counted nothing; tests/test_shard_model_cpu.py asserts
without a GPU that each input still reaches the edge it is named for.  Every comparison is exact: the row lengths,
columns, counts and row sums of every owned row equal tests/_shard_model.py's.  The tests need an MI355X and carry
the gpu mark one by one.
"""
import ctypes

import numpy as np
import pytest

from tests import _shard_cases as cases
from tests import _shard_model as model


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _d2h(ptr, n, dtype):
    out = np.zeros(n, dtype)
    if n:
        hip = ctypes.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), ctypes.c_size_t(out.nbytes),
                             ctypes.c_int(2)) == 0
    return out


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda")


def _merge(core, torch, c, M=None, rowsum="true", entries="tensor"):
    """The case through merge_partitions -> the result as a model.Merged.  rowsum: "true" (the case's sums as
    rowsum_global), None (unchecked) or an int64 [M] array; entries="none" passes no entries buffer."""
    M = c.M if M is None else M
    assert core.n_items == M
    nnz = _dev(torch, c.recv_nnz)
    ent = None if entries == "none" or len(c.entries) == 0 else _dev(torch, c.entries)
    rs = None if rowsum is None else _dev(torch, cases.rowsum_global(c, M) if isinstance(rowsum, str) else rowsum)
    m = core.merge_partitions(c.n, c.part, nnz, ent, rs, signed_nets=c.signed)
    R = c.R
    assert m.n_items == R
    base = _d2h(m.row_base, R, np.int64)
    lens = _d2h(m.row_nnz, R, np.int32).astype(np.int64)
    # (read nothing past the output capacity, whatever the lengths say)
    cap = int(np.minimum(cases.row_totals(c), M).sum())
    hi = int((base + lens).max()) if R else 0
    assert np.all(lens >= 0) and np.all(base >= 0) and hi <= cap, "row_base / row_nnz outside the output"
    col, cnt = _d2h(m.col, hi, np.int32), _d2h(m.cnt, hi, np.uint32)
    idx = np.repeat(base, lens) + model._ramp(lens)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return model.Merged(row_ptr, col[idx], cnt[idx], _d2h(m.rowsum, R, np.int64))


def _assert_equal(got, want, where):
    if not np.array_equal(got.row_ptr, want.row_ptr):
        bad = np.flatnonzero(np.diff(got.row_ptr) != np.diff(want.row_ptr))
        pairs = [(int(r), int(np.diff(got.row_ptr)[r]), int(np.diff(want.row_ptr)[r])) for r in bad[:8]]
        raise AssertionError(f"{where}: {len(bad)} row lengths differ, (row, got, want) {pairs}")
    if not (np.array_equal(got.cols, want.cols) and np.array_equal(got.cnt, want.cnt)):
        k = np.flatnonzero((got.cols != want.cols) | (got.cnt != want.cnt))
        rows = np.searchsorted(want.row_ptr, k[:8], side="right") - 1
        bad = list(zip(rows.tolist(), got.cols[k[:8]].tolist(), want.cols[k[:8]].tolist(), got.cnt[k[:8]].tolist(),
                       want.cnt[k[:8]].tolist()))
        raise AssertionError(f"{where}: {len(k)} entries differ, (row, col, want col, cnt, want cnt) {bad}")
    if not np.array_equal(got.rowsum, want.rowsum):
        bad = np.flatnonzero(got.rowsum != want.rowsum)
        pairs = [(int(r), int(got.rowsum[r]), int(want.rowsum[r])) for r in bad[:8]]
        raise AssertionError(f"{where}: {len(bad)} row sums differ, (row, got, want) {pairs}")


def _want(c):
    return model.merge(c.M, c.n, c.part, c.recv_nnz, c.entries, c.signed)


# ---- A. dense, unsigned, compaction edges --------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M", cases.A_M)
def test_dense_compaction_edges(pkg, torch_cuda, M):
    """Rows that are empty, hold column 0 or M - 1 alone, the columns at both ends of every wave's range, every
    column from every source, one column from every source, or entries of the last source only; one key that sums
    to 2^32 - 1; M around one and sixteen waves' widths and at the largest LDS row (162,816 B).  At M = 1 parts 1
    and 2 own nothing."""
    with pkg.CooccurrenceCore(n_items=M) as core:
        for part in range(cases.A_N):
            c = cases.case_a(M, part)
            got = _merge(core, torch_cuda, c)
            _assert_equal(got, _want(c), f"part {part}")
            if M == 1:
                assert len(got.rowsum) == (1 if part == 0 else 0)


# ---- B. LDS row reuse ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("variant", cases.B_VARIANTS)
def test_lds_row_reuse(pkg, torch_cuda, variant):
    """2,000 rows on one part, about eight per workgroup: after a full row of counts >= 2^31 a row of three small
    counts (and, third_empty, an empty row) shows every counter its workgroup left behind."""
    c = cases.case_b(variant)
    with pkg.CooccurrenceCore(n_items=cases.B_M) as core:
        _assert_equal(_merge(core, torch_cuda, c), _want(c), variant)


# ---- C. sorted path, unsigned --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,n", cases.C_SHAPES)
def test_sorted_merge_edges(pkg, torch_cuda, M, n):
    """The first n_items past the LDS row and 10^6: rows around every power of two (10,000 parts: 5 and 4 owned
    rows, 35 and 34 key bits), columns 0, 65,535, 65,536 and M - 1, a key from every source, sources with disjoint
    columns; then the first, last and middle row empty; then no entry at all and no entries buffer."""
    with pkg.CooccurrenceCore(n_items=M) as core:
        for part in cases.c_parts(M, n):
            for variant in cases.C_VARIANTS:
                c = cases.case_c(M, n, part, variant)
                got = _merge(core, torch_cuda, c, entries="none" if variant == "none" else "tensor")
                _assert_equal(got, _want(c), f"part {part}, {variant}")
                if variant == "none":
                    assert got.row_ptr.tolist() == [0] * (c.R + 1) and not got.rowsum.any()


# ---- H. sorted path, the sum by key at tile edges ------------------------------------------------------------
@pytest.mark.gpu
def test_sum_by_key_tile_edges(pkg, torch_cuda):
    """At 40,705 items and 70 sources: 4,095, 4,096, 4,097 and 8,193 received entries (a scan tile and a radix tile
    hold 4,096), a run of equal keys over the sorted positions 4,094 to 4,098, the last element a run of its own, one
    key from all 70 sources, 5,000 keys that all differ, one key and nothing else."""
    with pkg.CooccurrenceCore(n_items=cases.H_M) as core:
        for variant in cases.H_VARIANTS:
            c = cases.case_h(variant)
            _assert_equal(_merge(core, torch_cuda, c), _want(c), variant)


# ---- D. both paths, one input --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("part", cases.D_PARTS)
def test_dense_and_sorted_agree(pkg, torch_cuda, part):
    """One random input of 13,568 owned rows merged in a context of 40,704 items (dense) and in one of 40,705
    (sorted): both equal the model, so each other."""
    c = cases.case_d(part)
    want = _want(c)
    got = []
    for M in cases.D_M:
        with pkg.CooccurrenceCore(n_items=M) as core:
            got.append(_merge(core, torch_cuda, c, M=M))
            _assert_equal(got[-1], want, f"{model.merge_path(M, False)} merge at {M} items")
    _assert_equal(got[0], got[1], "dense against sorted")


# ---- E. uint32 overflow --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M", cases.E_M)
def test_overflow_is_reported(pkg, torch_cuda, M):
    """Two sources send 2^31 for one key: with the true row sums the merge fails with status 5 on both paths;
    with 2^31 - 1 from each the same input merges clean.  (What an unchecked merge does with the wrapped key is
    not asserted: the dense merge drops it, the sorted one keeps it with count 0.)"""
    with pkg.CooccurrenceCore(n_items=M) as core:
        with pytest.raises(pkg.CoocError) as e:
            _merge(core, torch_cuda, cases.case_e(M, 1 << 31))
        assert e.value.status == 5
        ok = cases.case_e(M, (1 << 31) - 1)
        _assert_equal(_merge(core, torch_cuda, ok), _want(ok), "control")


# ---- F. signed nets ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", cases.F_N)
@pytest.mark.parametrize("M", cases.F_M)
def test_signed_nets(pkg, torch_cuda, M, n):
    """signed_nets on both sides of its threshold (39,470 dense, 39,471 sorted): keys whose nets cancel stay with
    count 0, negative nets, a row whose every key cancels, a negative row sum, columns at the touched bitmap's word
    edges.  Clean with the signed row sums; status 5 with one row's sum off by one."""
    with pkg.CooccurrenceCore(n_items=M) as core:
        for part in range(n):
            c = cases.case_f(M, n, part)
            _assert_equal(_merge(core, torch_cuda, c), _want(c), f"part {part}")
        wrong = cases.rowsum_global(c)
        wrong[c.part + (c.R // 2) * c.n] += 1
        with pytest.raises(pkg.CoocError) as e:
            _merge(core, torch_cuda, c, rowsum=wrong)
        assert e.value.status == 5


# ---- G. pack round trip on real counts -----------------------------------------------------------------------
def _pack_round_trip(pkg, oracle, torch, M, n_parts, output):
    up, it = cases.g_log(M)
    packs = []
    with pkg.CooccurrenceCore(n_items=M, output=output) as core:
        for s, (sup, sit) in enumerate(cases.g_shards(up, it, n_parts)):
            core.count_device(_dev(torch, sup), _dev(torch, sit))
            counts = core.partition_plan(n_parts)
            row_nnz = torch.empty(M, dtype=torch.int32, device="cuda")
            entries = torch.empty(int(counts.sum()), dtype=torch.int64, device="cuda")
            core.partition_pack(n_parts, row_nnz, entries)
            torch.cuda.synchronize()
            got = (row_nnz.cpu().numpy(), counts, entries.cpu().numpy().view(np.uint64))
            rp, cols, data, _, _ = oracle.closed_form(sup, sit, M)
            want = model.pack(rp, cols, data, M, n_parts)
            assert np.array_equal(got[0], want.row_nnz), f"shard {s}: packed row lengths"
            assert np.array_equal(got[1], want.part_entries), f"shard {s}: entries per owner"
            assert np.array_equal(got[2], want.entries), f"shard {s}: packed entries"
            packs.append(got)
        rp, cols, data, rowsums, _ = oracle.closed_form(up, it, M)
        for part in range(n_parts):
            nnz, ent = cases.slice_for_owner(packs, M, n_parts, part)
            c = cases.Case(M, n_parts, part, model.rows_owned(M, n_parts, part), nnz, ent, None, False, {})
            own = np.arange(part, M, n_parts)
            got = _merge(core, torch, c, rowsum=rowsums.astype(np.int64))
            lens = np.diff(rp)[own]
            idx = np.repeat(rp[own], lens) + model._ramp(lens)
            want = model.Merged(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), cols[idx].astype(np.int32),
                                data[idx].astype(np.uint32), rowsums[own].astype(np.int64))
            _assert_equal(got, want, f"owner {part}")


@pytest.mark.gpu
@pytest.mark.parametrize("n_parts", cases.G_SMALL_PARTS)
@pytest.mark.parametrize("output", ["csr", "dense"])
def test_pack_round_trip(pkg, oracle, torch_cuda, output, n_parts):
    """300 users in n_parts shards at 130 items, each counted, planned and packed (k_permute_nnz, k_pack_entries,
    k_pack_entries_dense): the packed buffers equal the model's pack of the shard's closed form, and every owner's
    merge of the slices equals the closed form of the whole log.  133 parts: parts 130 to 132 own nothing."""
    _pack_round_trip(pkg, oracle, torch_cuda, cases.G_SMALL_M, n_parts, output)


@pytest.mark.gpu
@pytest.mark.parametrize("n_parts", cases.G_LARGE_PARTS)
def test_pack_round_trip_large_universe(pkg, oracle, torch_cuda, n_parts):
    """The same at 41,000 items: the large-universe planner's padded CSR through k_pack_entries and the sorted
    merge."""
    _pack_round_trip(pkg, oracle, torch_cuda, cases.G_LARGE_M, n_parts, "csr")
