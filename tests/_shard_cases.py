"""The dictated inputs of tests/test_gpu_shard_merge_edges.py (groups A to F and H; G counts real logs): what one owner
receives from its sources, built on the CPU.  tests/test_shard_model_cpu.py asserts each input's shape claims without
a GPU; the GPU tests feed the same inputs to the library.

A Case is what cooc_merge_partitions takes for owner `part` of `n` parts in a context of M items: recv_nnz int32
[n * R] and entries uint64 (col << 32 | cnt), both source-major, a (source, owned row) segment in column order.
rowsum holds the true int64 sum of every owned row's sent counts (signed nets: sign-extended), which is what the
all-reduced row sums of a real exchange hold; rowsum_global() scatters it to the items.  Every column is < M.  Every
row receives at most M entries, the full rows of group A apart, which every source sends whole (n M entries for M
keys: the output capacity is the M it is cut to).
"""
import functools
from collections import namedtuple

import numpy as np

from tests._shard_model import rows_owned, wave_ranges

Case = namedtuple("Case", "M n part R recv_nnz entries rowsum signed tags")

U32 = (1 << 32) - 1


class _Triples:
    """(source, owned row, column, count) quadruples of one case, collected pattern by pattern."""

    def __init__(self, M, n, part):
        self.M, self.n, self.part, self.R = M, n, part, rows_owned(M, n, part)
        self.parts = []

    def add(self, src, r, col, cnt):
        src, r, col, cnt = np.broadcast_arrays(np.asarray(src, np.int64), np.asarray(r, np.int64),
                                               np.asarray(col, np.int64), np.asarray(cnt, np.int64))
        self.parts.append(np.stack([src.ravel(), r.ravel(), col.ravel(), cnt.ravel()]))

    def case(self, signed=False, tags=None, force=None):
        """force: {(owned row, column): total}: the senders of that key get counts that sum to exactly total."""
        M, n, R = self.M, self.n, self.R
        q = np.concatenate(self.parts, axis=1) if self.parts else np.zeros((4, 0), np.int64)
        src, r, col, cnt = q
        assert np.all((0 <= src) & (src < n)) and np.all((0 <= r) & (r < R)) and np.all((0 <= col) & (col < M))
        order = np.lexsort((col, r, src))
        src, r, col, cnt = src[order], r[order], col[order], cnt[order]
        seg = src * R + r
        same = (seg[1:] == seg[:-1]) & (col[1:] == col[:-1])
        assert not same.any(), "a source sends a key twice"
        for (fr, fc), total in (force or {}).items():
            k = np.flatnonzero((r == fr) & (col == fc))
            assert len(k) >= 1
            cnt[k] = 1
            cnt[k[0]] = total - (len(k) - 1)
        assert np.all((-(1 << 31) <= cnt) & (cnt <= U32)) and (signed or np.all(cnt >= 1))
        recv_nnz = np.bincount(seg, minlength=n * R).astype(np.int32)
        entries = (col.astype(np.uint64) << np.uint64(32)) | (cnt.astype(np.uint64) & np.uint64(U32))
        rowsum = np.zeros(R, np.int64)
        np.add.at(rowsum, r, cnt)
        return Case(M, n, self.part, R, recv_nnz, entries, rowsum, signed, tags or {})


def rowsum_global(case, M=None):
    """int64 [M]: the owned rows' true sums at their items, zeros elsewhere."""
    out = np.zeros(case.M if M is None else M, np.int64)
    out[case.part + np.arange(case.R, dtype=np.int64) * case.n] = case.rowsum
    return out


def row_totals(case):
    """Entries every owned row receives (what k_merge_plan sums before it cuts to M)."""
    return case.recv_nnz.astype(np.int64).reshape(case.n, case.R).sum(axis=0) if case.R else np.zeros(0, np.int64)


# ---- A. dense, unsigned, compaction edges --------------------------------------------------------------------
A_M = (1, 63, 64, 65, 1023, 1024, 1025, 40704)
A_N = 3
A_PATTERNS = ("col0", "empty", "last_col", "wave_edges", "full", "one_col_all", "last_source")
A_FULL_ROWS_BIG = 2  # full rows per part at M = 40,704


def wave_edge_cols(M):
    """w per - 1, w per and min(M, (w + 1) per) - 1 of every wave w whose range is non-empty."""
    cols = set()
    for lo, hi in wave_ranges(M):
        if hi > lo:
            cols |= {lo - 1, lo, hi - 1}
    return np.array(sorted(c for c in cols if 0 <= c < M), np.int64)


def a_pattern_of(M, part):
    """Pattern index of every owned row: item a takes pattern a mod 7; at M = 40,704 only the first two full rows of
    a part stay full, the others send column 0 alone."""
    a = part + np.arange(rows_owned(M, A_N, part), dtype=np.int64) * A_N
    pat = a % len(A_PATTERNS)
    if M == 40704:
        full = np.flatnonzero(pat == A_PATTERNS.index("full"))
        pat[full[A_FULL_ROWS_BIG:]] = A_PATTERNS.index("col0")
    return a, pat


@functools.lru_cache(maxsize=None)
def case_a(M, part):
    n = A_N
    t = _Triples(M, n, part)
    rng = np.random.default_rng(1000 * M + part)
    a, pat = a_pattern_of(M, part)

    def rows(name):
        return np.flatnonzero(pat == A_PATTERNS.index(name))

    def counts(*shape):
        return rng.integers(1, (1 << 20) + 1, shape)

    r = rows("col0")
    t.add(a[r] % n, r, 0, counts(len(r)))
    r = rows("last_col")
    t.add((a[r] // 7) % n, r, M - 1, counts(len(r)))
    edges = wave_edge_cols(M)
    for r in rows("wave_edges"):  # edge i from source i mod n, the even ones from the next source as well
        i = np.arange(len(edges))
        t.add(i % n, r, edges, counts(len(edges)))
        t.add((i[::2] + 1) % n, r, edges[::2], counts(len(edges[::2])))
    for r in rows("full"):
        t.add(np.arange(n)[:, None], r, np.arange(M)[None, :], counts(n, M))
    r = rows("one_col_all")
    t.add(np.arange(n)[:, None], r[None, :], ((a[r] * 37) % M)[None, :], counts(n, len(r)))
    k = min(5, M)
    for r in rows("last_source"):
        t.add(n - 1, r, rng.choice(M, k, replace=False), counts(k))
    # one key of the case sums to exactly 2^32 - 1: a column all sources send, else the case's only key
    r = rows("one_col_all")
    key = (int(r[0]), int((a[r[0]] * 37) % M)) if len(r) else ((0, 0) if t.R else None)
    return t.case(tags={"max_key": key}, force={key: U32} if key else None)


# ---- B. LDS row reuse ----------------------------------------------------------------------------------------
B_M = 2000
B_VARIANTS = ("alternate", "third_empty")


@functools.lru_cache(maxsize=None)
def case_b(variant):
    """One part owns all 2,000 rows (a workgroup takes about eight of them): full rows with counts of 2^31 and more
    alternate with rows of three columns; third_empty: every third row is empty, the others alternate."""
    M = B_M
    t = _Triples(M, 1, 0)
    rng = np.random.default_rng(7)
    r = np.arange(M, dtype=np.int64)
    live = r if variant == "alternate" else r[r % 3 != 2]
    full, three = live[0::2], live[1::2]
    t.add(0, full[:, None], np.arange(M)[None, :], rng.integers(1 << 31, U32 + 1, (len(full), M)))
    cols = np.stack([three % 997, 997 + three % 1000, np.full(len(three), M - 1)], axis=1)
    t.add(0, three[:, None], cols, rng.integers(1, 1 << 20, cols.shape))
    return t.case(tags={"full": full, "three": three})


# ---- C. sorted path, unsigned --------------------------------------------------------------------------------
C_SHAPES = ((40705, 2), (40705, 3), (1000000, 2), (1000000, 3), (40705, 10000))
C_VARIANTS = ("every_row", "holes", "none")
C_EDGE_COLS = (0, 65535, 65536)  # and M - 1


def c_parts(M, n):
    return (0, 704, 705, 9999) if n == 10000 else tuple(range(n))


def c_rows(R, variant):
    """The owned rows that receive anything: every row up to 4,096 rows, else the first and last 1,500, 100 in the
    middle and the rows around every power of two; holes: without the first, the last and the middle row."""
    if variant == "none":
        return np.zeros(0, np.int64)
    if R <= 4096:
        rows = set(range(R))
    else:
        rows = set(range(1500)) | set(range(R - 1500, R)) | set(range(R // 2 - 50, R // 2 + 50))
        k = 1
        while k < R:
            rows |= {k - 1, k, k + 1} & set(range(R))
            k *= 2
    if variant == "holes":
        rows -= {0, R - 1, R // 2}
    return np.array(sorted(rows), np.int64)


@functools.lru_cache(maxsize=None)
def case_c(M, n, part, variant):
    """Row r takes pattern r mod 3: (0) the edge columns {0, 65,535, 65,536, M - 1} below M, in turn from the
    sources, and a key from every source; (1) a key from every source and two more keys; (2) every source sends d
    columns of its own (d = 3, at 10,000 sources 2), the sources' columns interleaved."""
    t = _Triples(M, n, part)
    rng = np.random.default_rng(M + 31 * n + part)
    rows = c_rows(t.R, variant)
    edges = np.array(sorted({c for c in C_EDGE_COLS + (M - 1,) if c < M}), np.int64)
    d = 2 if n == 10000 else 3
    assert 7 + d * n <= M
    s = np.arange(n, dtype=np.int64)

    def counts(*shape):  # (n of them stay below 2^32)
        return rng.integers(1, min(1 << 20, U32 // n) + 1, shape)

    r = rows[rows % 3 == 0]
    i = np.arange(len(edges))
    t.add((r[:, None] + i[None, :]) % n, r[:, None], edges[None, :], counts(len(r), len(edges)))
    t.add(s[:, None], r[None, :], (1 + (r * 13) % 1000)[None, :], counts(n, len(r)))
    r = rows[rows % 3 == 1]
    t.add(s[:, None], r[None, :], (40000 + r % 700)[None, :], counts(n, len(r)))
    t.add(r % n, r, 5 + r % 11, counts(len(r)))
    t.add((r + 1) % n, r, M - 2 - r % 3, counts(len(r)))
    r = rows[rows % 3 == 2]
    for j in range(d):
        t.add(s[:, None], r[None, :], 7 + s[:, None] + j * n, counts(n, len(r)))
    return t.case(tags={"rows": rows})


# ---- H. sorted path, the sum by key at tile edges ------------------------------------------------------------
H_M, H_N, H_PART = 40705, 70, 0  # the first n_items past the LDS row; 70 sources: a run of more than 64 equal keys
H_TILE = 4096  # elements of one scan tile and of one radix tile
H_SIZES = {"n4095": 4095, "n4096": 4096, "n4097": 4097, "n8193": 8193}
H_VARIANTS = tuple(H_SIZES) + ("straddle", "last_alone", "long_run", "distinct", "one_key")
H_STRADDLE = (H_TILE - 2, H_TILE + 2)  # the sorted positions of the straddling run's first and last element
H_LONG_KEY, H_ONE_KEY, H_ONE_SOURCES = (3, 1000), (291, 12345), 66


def _h_fill(t, rng, total, rows, mult=(1, 2, 3)):
    """total entries in the owned rows [rows[0], rows[1]): distinct key j (row rows[0] + j mod width, column
    11 (j div width) + j mod 7) from mult[j mod len(mult)] sources in a row, from source j on; the last key is cut
    to fit."""
    width = rows[1] - rows[0]
    j = np.arange(total, dtype=np.int64)
    m = np.asarray(mult, np.int64)[j % len(mult)]
    m = np.minimum(m, np.maximum(total - (np.cumsum(m) - m), 0))
    key, i = np.repeat(j, m), _ramp(m)
    t.add((key + i) % t.n, rows[0] + key % width, 11 * (key // width) + key % 7, rng.integers(1, (1 << 20) + 1, total))


def _ramp(lens):
    return np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)


@functools.lru_cache(maxsize=None)
def case_h(variant):
    """n4095 .. n8193: that many received entries, runs of one, two and three equal keys in turn; straddle: 4,094
    entries of rows below 100, then one key of row 100 from five sources (sorted positions 4,094 to 4,098), then
    300 entries of later rows; last_alone: the largest key (R - 1, M - 1) from one source after runs of two and
    three; long_run: one key from all 70 sources between runs of one to three; distinct: 5,000 keys, each from one
    source; one_key: one key from 66 sources and nothing else."""
    t = _Triples(H_M, H_N, H_PART)
    rng = np.random.default_rng(4096 + H_VARIANTS.index(variant))
    R, s = t.R, np.arange(H_N, dtype=np.int64)

    def counts(k):
        return rng.integers(1, (1 << 20) + 1, k)

    if variant in H_SIZES:
        _h_fill(t, rng, H_SIZES[variant], (0, R))
    elif variant == "straddle":
        _h_fill(t, rng, H_STRADDLE[0], (0, 100))
        t.add(s[:5], 100, 5, counts(5))
        _h_fill(t, rng, 300, (101, R))
    elif variant == "last_alone":
        _h_fill(t, rng, 200, (0, R - 1), mult=(2, 3))
        t.add(7, R - 1, H_M - 1, counts(1))
    elif variant == "long_run":
        _h_fill(t, rng, 100, (0, H_LONG_KEY[0]))
        t.add(s, H_LONG_KEY[0], H_LONG_KEY[1], counts(H_N))
        _h_fill(t, rng, 100, (H_LONG_KEY[0] + 1, R))
    elif variant == "distinct":
        _h_fill(t, rng, 5000, (0, R), mult=(1,))
    else:
        t.add(s[:H_ONE_SOURCES], H_ONE_KEY[0], H_ONE_KEY[1], counts(H_ONE_SOURCES))
    return t.case()


# ---- D. both paths, one input --------------------------------------------------------------------------------
D_M = (40704, 40705)
D_N, D_PARTS, D_R, D_ENTRIES = 3, (1, 2), 13568, 200000


@functools.lru_cache(maxsize=None)
def case_d(part):
    """About 2 10^5 random (source, row, column) keys with every column < 40,704, as a case of 40,704 items; the GPU
    test merges it in a context of 40,704 items and in one of 40,705 (the same rows are owned at both)."""
    M = D_M[0]
    t = _Triples(M, D_N, part)
    rng = np.random.default_rng(90 + part)
    k = np.unique(rng.integers(0, D_N * D_R * M, D_ENTRIES))
    t.add(k // (D_R * M), (k // M) % D_R, k % M, rng.integers(1, (1 << 20) + 1, len(k)))
    return t.case()


# ---- E. uint32 overflow --------------------------------------------------------------------------------------
E_M = (700, 40705)
E_KEY = (4, 17)  # (owned row, column) that two sources send 2^31 (control: 2^31 - 1) for


@functools.lru_cache(maxsize=None)
def case_e(M, big):
    t = _Triples(M, 2, 0)
    rng = np.random.default_rng(M)
    r = np.arange(10, dtype=np.int64)
    for s in range(2):
        t.add(s, r[:, None], np.array([3 + s, 100, M - 1 - s])[None, :] + 0 * r[:, None],
              rng.integers(1, (1 << 20) + 1, (len(r), 3)))
    t.add(np.arange(2), E_KEY[0], E_KEY[1], big)
    return t.case()


# ---- F. signed nets ------------------------------------------------------------------------------------------
F_M = (65, 1025, 39470, 39471, 40705)
F_N = (2, 3)
F_PATTERNS = ("cancel", "negative", "all_cancel", "negative_sum", "word_edges", "empty")
F_WORD_COLS = (31, 32, 63, 64)  # and M - 1


@functools.lru_cache(maxsize=None)
def case_f(M, n, part):
    """Row r takes pattern r mod 6.  cancel: + 3 and - 3 for one key from two sources, + 7 for another key;
    negative: three keys of negative nets, one of them from two sources; all_cancel: four keys, the sources' nets
    of each sum to 0; negative_sum: + 5, - 100 and a key of + 2 and - 9; word_edges: the columns {31, 32, 63, 64,
    M - 1} with + 4 and - 4 in turn, column 32 cancelling as well; empty."""
    t = _Triples(M, n, part)
    rng = np.random.default_rng(M * 10 + n * 3 + part)
    rr = np.arange(t.R, dtype=np.int64)

    def rows(name):
        return rr[rr % len(F_PATTERNS) == F_PATTERNS.index(name)]

    r = rows("cancel")
    c = (r * 5) % (M - 1)
    t.add(0, r, c, 3)
    t.add(1, r, c, -3)
    t.add(n - 1, r, c + 1, 7)
    r = rows("negative")
    c = (r * 11) % (M - 40)
    t.add(r % n, r, c, -rng.integers(1, 1 << 20, len(r)))
    t.add((r + 1) % n, r, c + 9, -rng.integers(1, 1 << 20, len(r)))
    t.add(0, r, c + 33, -1)
    t.add(n - 1, r, c + 33, -(1 << 20))
    r = rows("all_cancel")
    for j in range(4):
        c = (r * 3 + 16 * j) % M
        v = rng.integers(3, 1 << 20, len(r))
        t.add(0, r, c, v)
        if n == 2:
            t.add(1, r, c, -v)
        else:
            t.add(1, r, c, -(v - 2))
            t.add(2, r, c, -2)
    r = rows("negative_sum")
    t.add(r % n, r, 2, 5)
    t.add((r + 1) % n, r, M - 2, -100)
    t.add(0, r, 40, 2)
    t.add(n - 1, r, 40, -9)
    r = rows("word_edges")
    cols = np.array(sorted(set(F_WORD_COLS + (M - 1,))), np.int64)
    i = np.arange(len(cols))
    t.add((r[:, None] + i[None, :]) % n, r[:, None], cols[None, :], np.where(i % 2 == 0, 4, -4)[None, :])
    other = (r[:, None] + i[None, :] + 1) % n  # column 32: the next source cancels it
    t.add(other[:, 1], r, 32, 4)
    return t.case(signed=True, tags={"rows": rows})


# ---- G. pack round trip on real counts -----------------------------------------------------------------------
G_SMALL_M, G_LARGE_M, G_USERS = 130, 41000, 300
G_SMALL_PARTS = (1, 2, 3, 7, 130, 133)
G_LARGE_PARTS = (2, 3)


@functools.lru_cache(maxsize=None)
def g_log(M):
    """300 users of about six interactions over M items (the package's seeded small log)."""
    from __graft_entry__ import load_package

    load_package()
    from flink_cooccurrence_amd import datagen

    return datagen.small_log(17 + M, G_USERS, M, 6.0)


def g_shards(up, it, n_parts):
    """The log's users in n_parts contiguous shards, each a CSR of its own."""
    U = len(up) - 1
    for s in range(n_parts):
        lo, hi = s * U // n_parts, (s + 1) * U // n_parts
        yield up[lo:hi + 1] - up[lo], it[up[lo]:up[hi]]


def slice_for_owner(packs, M, n_parts, part):
    """What an all-to-all delivers to owner `part` from every source's (row_nnz, part_entries, entries): the
    source-major row lengths and entries of the owner's rows."""
    R = rows_owned(M, n_parts, part)
    r0 = sum(rows_owned(M, n_parts, o) for o in range(part))
    nnz = np.concatenate([np.asarray(pk[0][r0:r0 + R], np.int32) for pk in packs])
    ent = [np.asarray(pk[2]).view(np.uint64)[int(np.sum(pk[1][:part])):int(np.sum(pk[1][:part + 1]))] for pk in packs]
    return nnz, np.concatenate(ent)
