"""A plain numpy restatement of cooc_verify_batch's contract (include/cooc.h, "invariant checks of a batch
result"), written from that text: what the six totals and the per-row fingerprints of ANY result arrays are,
correct or corrupted.  tests/test_gpu_verify_negative.py runs the device checker and this model on the same
mutated arrays; tests/test_verify_model_cpu.py pins the model itself on hand-written matrices.

    [0] sum of all counts                       [1] sum of the row sums
    [2] entries                                 [3] ROWS whose counts do not sum to their row sum
    [4] ROWS with a bad entry                   [5] ENTRIES with C[a, b] != C[b, a]

A row of the padded CSR holds the entries [row_base[a], row_base[a] + row_nnz[a]); a row with row_nnz < 0 is a
bad row without entries.  [4], padded CSR: a column outside [0, n_items), a count of 0, or -- unless the result is
an any-order one -- two neighbours that are not strictly ascending in order[col] (order: the result's column
order, core.column_order()).  [4], dense: row_nnz[a] != the row's non-zero cells.  [5], per entry (a, b, v): b out
of range, row b without a key a, or with another count than v; only when asked for, on an ordered padded CSR
(else None, as core.verify_batch reports the -1).

fingerprint[a] = sum over the row's keys of splitmix64((col << 32) ^ count) mod 2^64 (col as its 32-bit
pattern), with splitmix64(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;
x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31.
"""
import numpy as np

KEYS = ("sum_counts", "sum_rowsums", "entries", "rows_bad_sum", "rows_bad_entries", "asymmetric_entries")


def key_hash(cols, counts) -> np.ndarray:
    """splitmix64((col << 32) ^ count) per entry, uint64 (wrapping)."""
    with np.errstate(over="ignore"):
        c = np.asarray(cols, np.int32).view(np.uint32).astype(np.uint64)
        x = (c << np.uint64(32)) ^ np.asarray(counts, np.uint32).astype(np.uint64)
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def _as_i64(total: int) -> int:
    """A uint64 total as the int64 the C-ABI reports."""
    total &= (1 << 64) - 1
    return total - (1 << 64) if total >> 63 else total


def _row_sums(rows, values, M):
    """Per-row wrapping uint64 sums of values (one per entry; rows: the entry's row)."""
    out = np.zeros(M, np.uint64)
    with np.errstate(over="ignore"):
        np.add.at(out, rows, values)
    return out


def verify_csr(row_base, row_nnz, col, cnt, rowsum, order, ordered=True, symmetry=False):
    """-> (report dict with KEYS, fingerprints uint64 [n_items]) of a padded CSR."""
    row_nnz = np.asarray(row_nnz, np.int64)
    row_base = np.asarray(row_base, np.int64)
    M = len(row_nnz)
    n = np.maximum(row_nnz, 0)
    rows = np.repeat(np.arange(M), n)
    first = np.cumsum(n) - n  # a row's first entry among the gathered ones
    pos = row_base[rows] + (np.arange(len(rows)) - first[rows])
    c = np.asarray(col, np.int32)[pos].astype(np.int64)
    v = np.asarray(cnt, np.uint32)[pos].astype(np.uint64)

    fingerprints = _row_sums(rows, key_hash(c, v), M)
    sums = _row_sums(rows, v, M)
    bad_sum = sums != np.asarray(rowsum, np.int64).astype(np.uint64)

    in_range = (c >= 0) & (c < M)
    bad_entry = ~in_range | (v == 0)
    if ordered and len(rows) > 1:
        pair = (rows[1:] == rows[:-1]) & in_range[1:] & in_range[:-1]  # (an out-of-range column is bad already)
        rank = np.asarray(order, np.int64)[np.where(in_range, c, 0)]
        bad_entry[:-1] |= pair & (rank[1:] <= rank[:-1])
    bad_row = row_nnz < 0
    bad_row[rows[bad_entry]] = True

    asym = None
    if symmetry and ordered:
        cl, vl = c.tolist(), v.tolist()
        lo, hi = first.tolist(), (first + n).tolist()
        filled = np.flatnonzero(n).tolist()
        keys = {a: dict(zip(cl[lo[a]:hi[a]], vl[lo[a]:hi[a]])) for a in filled}
        none = {}
        asym = 0
        for a in filled:
            for b, x in zip(cl[lo[a]:hi[a]], vl[lo[a]:hi[a]]):
                asym += not (0 <= b < M and keys.get(b, none).get(a) == x)

    report = {"sum_counts": _as_i64(sum(v.tolist())),
              "sum_rowsums": _as_i64(sum(np.asarray(rowsum, np.int64).tolist())),
              "entries": int(n.sum()),
              "rows_bad_sum": int(bad_sum.sum()),
              "rows_bad_entries": int(bad_row.sum()),
              "asymmetric_entries": asym}
    return report, fingerprints


def verify_dense(dense, row_nnz, rowsum):
    """-> (report, fingerprints) of a dense [n_items x n_items] result: a cell is a key iff it is non-zero."""
    d = np.asarray(dense, np.uint32)
    M = d.shape[0]
    rows, c = np.nonzero(d)
    v = d[rows, c].astype(np.uint64)
    fingerprints = _row_sums(rows, key_hash(c, v), M)
    sums = _row_sums(rows, v, M)
    cells = np.bincount(rows, minlength=M)
    report = {"sum_counts": _as_i64(sum(v.tolist())),
              "sum_rowsums": _as_i64(sum(np.asarray(rowsum, np.int64).tolist())),
              "entries": int(len(rows)),
              "rows_bad_sum": int((sums != np.asarray(rowsum, np.int64).astype(np.uint64)).sum()),
              "rows_bad_entries": int((cells != np.asarray(row_nnz, np.int64)).sum()),
              "asymmetric_entries": None}
    return report, fingerprints
