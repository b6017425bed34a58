"""tests/_verify_model.py (the numpy restatement of cooc_verify_batch's contract that the corrupted-result tests
of tests/test_gpu_verify_negative.py compare the device checker with) on hand-written 4-row results: every total
below is counted by hand from the arrays, the fingerprints with a splitmix64 on Python ints."""
import numpy as np

from tests import _verify_model as vm

_MASK = (1 << 64) - 1


def _splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _MASK
    return x ^ (x >> 31)


def _fingerprint(entries) -> int:
    return sum(_splitmix64(((c & 0xFFFFFFFF) << 32) ^ v) for c, v in entries) & _MASK


def _padded(rows, pad=-7):
    """rows: per row a list of (col, count) -> (row_base, col, cnt) with two words of padding after every row."""
    base, col, cnt = [], [], []
    for r in rows:
        base.append(len(col))
        col += [c for c, _ in r] + [pad, pad]
        cnt += [v for _, v in r] + [9, 9]
    return np.array(base, np.int64), np.array(col, np.int32), np.array(cnt, np.uint32)


def test_key_hash_known_answers():
    # the first output of splitmix64 seeded with 0 (the published test vector): the hash of key 0, count 0
    assert int(vm.key_hash([0], [0])[0]) == 0xE220A8397B1DCDAF == _splitmix64(0)
    cols, counts = [0, 1, 299, 33000, -1, 40000], [1, 7, 65536, 0xFFFFFFFF, 3, 2]
    got = vm.key_hash(cols, counts)
    assert got.dtype == np.uint64
    assert [int(x) for x in got] == [_fingerprint([(c, v)]) for c, v in zip(cols, counts)]


# C = [[0 2 1 0] [2 4 0 1] [1 0 0 0] [0 1 0 0]]: symmetric, one diagonal key, 7 keys, counts sum to 12
_CLEAN = [[(1, 2), (2, 1)], [(0, 2), (1, 4), (3, 1)], [(0, 1)], [(1, 1)]]


def test_clean_csr_identity_and_relabelled_order():
    base, col, cnt = _padded(_CLEAN)
    nnz, rowsum = np.array([2, 3, 1, 1], np.int32), np.array([3, 7, 1, 1], np.int64)
    rep, cs = vm.verify_csr(base, nnz, col, cnt, rowsum, np.arange(4), ordered=True, symmetry=True)
    assert rep == {"sum_counts": 12, "sum_rowsums": 12, "entries": 7, "rows_bad_sum": 0, "rows_bad_entries": 0,
                   "asymmetric_entries": 0}
    assert [int(x) for x in cs] == [_fingerprint(r) for r in _CLEAN]
    # column order 1, 3, 0, 2 (order[col] = the column's position): row 1 = [0, 1, 3] is out of order there
    order = np.array([2, 0, 3, 1])
    rep, cs2 = vm.verify_csr(base, nnz, col, cnt, rowsum, order, ordered=True, symmetry=False)
    assert rep["rows_bad_entries"] == 1 and rep["rows_bad_sum"] == 0 and rep["asymmetric_entries"] is None
    assert np.array_equal(cs, cs2)
    # ... and in order as [1, 3, 0], which ascending ids call unsorted; the fingerprints do not see the order
    rows = [_CLEAN[0], [(1, 4), (3, 1), (0, 2)], _CLEAN[2], _CLEAN[3]]
    base, col, cnt = _padded(rows)
    rep, cs3 = vm.verify_csr(base, nnz, col, cnt, rowsum, order, ordered=True, symmetry=True)
    assert rep["rows_bad_entries"] == 0 and rep["asymmetric_entries"] == 0
    assert np.array_equal(cs, cs3)
    assert vm.verify_csr(base, nnz, col, cnt, rowsum, np.arange(4))[0]["rows_bad_entries"] == 1
    assert vm.verify_csr(base, nnz, col, cnt, rowsum, np.arange(4), ordered=False)[0]["rows_bad_entries"] == 0


def test_corrupted_csr_totals_by_hand():
    """Row 0: a count of 0 (bad row; 2 != 3: bad sum).  Row 1: clean.  Row 2: row_nnz = -1 (bad row without
    entries; 0 != 1: bad sum).  Row 3: a column 4 = n_items (bad row; 1 + 1 == 2).
    [5]: (0, 2, 0) finds no key in the entry-less row 2, (3, 4, 1) is out of range; the other five entries
    (0,1,2) (1,1,4) (1,3,1) (1,0,2) (3,1,1) find their partner."""
    rows = [[(1, 2), (2, 0)], [(1, 4), (3, 1), (0, 2)], [(0, 1)], [(4, 1), (1, 1)]]
    base, col, cnt = _padded(rows)
    nnz, rowsum = np.array([2, 3, -1, 2], np.int32), np.array([3, 7, 1, 2], np.int64)
    order = np.array([2, 0, 3, 1])
    rep, cs = vm.verify_csr(base, nnz, col, cnt, rowsum, order, ordered=True, symmetry=True)
    assert rep == {"sum_counts": 11, "sum_rowsums": 13, "entries": 7, "rows_bad_sum": 2, "rows_bad_entries": 3,
                   "asymmetric_entries": 2}
    assert [int(x) for x in cs] == [_fingerprint(rows[0]), _fingerprint(rows[1]), 0, _fingerprint(rows[3])]
    rep_u, cs_u = vm.verify_csr(base, nnz, col, cnt, rowsum, order, ordered=False, symmetry=True)
    assert rep_u == dict(rep, asymmetric_entries=None) and np.array_equal(cs, cs_u)
    # ascending ids: row 1 = [1, 3, 0] is out of order as well
    assert vm.verify_csr(base, nnz, col, cnt, rowsum, np.arange(4))[0]["rows_bad_entries"] == 4


def test_equal_neighbours_are_not_ascending():
    rows = [[(2, 1), (2, 1)], [], [], []]
    base, col, cnt = _padded(rows)
    nnz, rowsum = np.array([2, 0, 0, 0], np.int32), np.array([2, 0, 0, 0], np.int64)
    rep, cs = vm.verify_csr(base, nnz, col, cnt, rowsum, np.arange(4), ordered=True, symmetry=True)
    # (0, 2, 1) twice, row 2 is empty: both asymmetric
    assert rep == {"sum_counts": 2, "sum_rowsums": 2, "entries": 2, "rows_bad_sum": 0, "rows_bad_entries": 1,
                   "asymmetric_entries": 2}
    assert int(cs[0]) == (2 * _splitmix64((2 << 32) ^ 1)) & _MASK and not cs[1:].any()
    assert vm.verify_csr(base, nnz, col, cnt, rowsum, np.arange(4), ordered=False)[0]["rows_bad_entries"] == 0


def test_dense_totals_by_hand():
    dense = np.array([[0, 2, 1, 0], [2, 4, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0]], np.uint32)
    nnz, rowsum = np.array([2, 3, 1, 1], np.int32), np.array([3, 7, 1, 1], np.int64)
    rep, cs = vm.verify_dense(dense, nnz, rowsum)
    assert rep == {"sum_counts": 12, "sum_rowsums": 12, "entries": 7, "rows_bad_sum": 0, "rows_bad_entries": 0,
                   "asymmetric_entries": None}
    assert [int(x) for x in cs] == [_fingerprint(r) for r in _CLEAN]
    # a zero cell := 5 in row 2 (6 != 1: bad sum; 2 cells != 1: bad row) and row_nnz[0] = 3 (2 cells: bad row)
    dense[2, 3] = 5
    nnz[0] = 3
    rep, cs = vm.verify_dense(dense, nnz, rowsum)
    assert rep == {"sum_counts": 17, "sum_rowsums": 12, "entries": 8, "rows_bad_sum": 1, "rows_bad_entries": 2,
                   "asymmetric_entries": None}
    assert int(cs[2]) == _fingerprint([(0, 1), (3, 5)]) and int(cs[0]) == _fingerprint(_CLEAN[0])
