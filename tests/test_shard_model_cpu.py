"""tests/_shard_model.py against a brute-force accumulation, and the shape claims of the dictated inputs of
tests/test_gpu_shard_merge_edges.py (tests/_shard_cases.py): which merge a case takes, its owned rows, the key bits
its sort needs, the edges its rows reach.  No GPU: one shape test per GPU test of that module."""
import numpy as np
import pytest

from tests import _shard_cases as cases
from tests import _shard_model as model

U32 = (1 << 32) - 1


# ---- the model -----------------------------------------------------------------------------------------------
def _brute_merge(M, n, part, recv_nnz, entries, signed):
    """Dicts, one Python int at a time: per owned row {col: sum mod 2^32}, presence, row sum."""
    R = len([a for a in range(M) if a % n == part])
    rows = [dict() for _ in range(R)]
    pos = 0
    for s in range(n):
        for r in range(R):
            for _ in range(int(recv_nnz[s * R + r])):
                e = int(entries[pos])
                pos += 1
                rows[r][e >> 32] = (rows[r].get(e >> 32, 0) + (e & U32)) & U32
    out = []
    for d in rows:
        keys = sorted(c for c, v in d.items() if signed or v != 0)
        vals = [d[c] for c in keys]
        total = sum(v - (1 << 32) if signed and v >= 1 << 31 else v for v in vals)
        out.append((keys, vals, total))
    return out


def _random_input(rng, signed):
    M = int(rng.integers(1, 40))
    n = int(rng.integers(1, 6))
    part = int(rng.integers(0, n))
    R = model.rows_owned(M, n, part)
    nnz = rng.integers(0, min(M, 6) + 1, n * R).astype(np.int32)
    ents = []
    for k in nnz:
        cols = np.sort(rng.choice(M, int(k), replace=False)).astype(np.uint64)
        if signed:
            cnt = rng.choice(np.array([-3, 3, -1, 1, -(1 << 31), (1 << 31) - 1, 0], np.int64), int(k))
        else:
            cnt = rng.choice(np.array([1, 2, 1 << 31, U32, (1 << 31) + 5], np.int64), int(k))
        ents.append((cols << np.uint64(32)) | (cnt.astype(np.uint64) & np.uint64(U32)))
    entries = np.concatenate(ents) if ents else np.zeros(0, np.uint64)
    return M, n, part, nnz, entries


@pytest.mark.parametrize("signed", [False, True])
def test_merge_equals_brute_force(signed):
    """300 small random inputs, with counts that wrap and nets that cancel."""
    rng = np.random.default_rng(11 + signed)
    seen_wrap = seen_zero = 0
    for _ in range(300):
        M, n, part, nnz, entries = _random_input(rng, signed)
        got = model.merge(M, n, part, nnz, entries, signed)
        want = _brute_merge(M, n, part, nnz, entries, signed)
        assert len(got.row_ptr) == len(want) + 1 and len(got.rowsum) == len(want)
        for r, (keys, vals, total) in enumerate(want):
            s, e = got.row_ptr[r], got.row_ptr[r + 1]
            assert got.cols[s:e].tolist() == keys and got.cnt[s:e].tolist() == vals
            assert int(got.rowsum[r]) == total
            seen_zero += vals.count(0)
        sent = model.merge(M, n, part, nnz, entries, True)  # (every key a source sent)
        seen_wrap += len(sent.cols) - len(model.merge(M, n, part, nnz, entries, False).cols)
    assert seen_wrap > 0 and (seen_zero > 0) == signed  # keys of sum 0: dropped when unsigned, kept when signed
    assert got.cols.dtype == np.int32 and got.cnt.dtype == np.uint32 and got.rowsum.dtype == np.int64


def test_merge_of_nothing():
    m = model.merge(1, 3, 1, np.zeros(0, np.int32), None, False)
    assert m.row_ptr.tolist() == [0] and len(m.cols) == len(m.cnt) == len(m.rowsum) == 0
    m = model.merge(5, 2, 0, np.zeros(6, np.int32), None, True)
    assert m.row_ptr.tolist() == [0, 0, 0, 0] and m.rowsum.tolist() == [0, 0, 0]


def test_rows_owned_equals_the_package(pkg):
    from flink_cooccurrence_amd import sharding

    for M in (1, 2, 7, 130, 700, 40704, 40705):
        for n in (1, 2, 3, 7, M, M + 3, 10000):
            owned = [model.rows_owned(M, n, p) for p in range(n)]
            assert owned == [sharding.rows_owned(M, n, p) for p in range(n)]
            assert sum(owned) == M


@pytest.mark.parametrize("M", [1, 2, 7, 130, 700])
def test_perm_index_is_a_bijection(M):
    for n in (1, 2, 3, 7, M, M + 3):
        p = model.perm_index(np.arange(M), M, n)
        assert sorted(p.tolist()) == list(range(M))
        inv = np.empty(M, np.int64)
        inv[p] = np.arange(M)
        assert inv.tolist() == [a for o in range(n) for a in range(o, M, n)]  # owner-major, then ascending row


def test_pack_equals_brute_force():
    rng = np.random.default_rng(5)
    for _ in range(200):
        M = int(rng.integers(1, 30))
        n = int(rng.integers(1, M + 4))
        nnz = rng.integers(0, min(M, 5) + 1, M)
        rp = np.concatenate([[0], np.cumsum(nnz)]).astype(np.int64)
        cols = np.concatenate([np.sort(rng.choice(M, int(k), replace=False)) for k in nnz] + [np.zeros(0, np.int64)])
        cnt = rng.integers(1, U32 + 1, len(cols))
        got = model.pack(rp, cols, cnt, M, n)
        order = [a for o in range(n) for a in range(o, M, n)]
        assert got.row_nnz.tolist() == [int(nnz[a]) for a in order]
        assert got.part_entries.tolist() == [int(sum(nnz[a] for a in range(o, M, n))) for o in range(n)]
        want = [(int(cols[i]) << 32) | int(cnt[i]) for a in order for i in range(rp[a], rp[a + 1])]
        assert got.entries.tolist() == want
        assert np.array_equal(got.row_nnz[model.perm_index(np.arange(M), M, n)], nnz)


def test_paths_and_key_bits():
    assert model.merge_path(40704, False) == "dense" and 4 * 40704 == model.DENSE_MAX_BYTES
    assert model.merge_path(40705, False) == "sorted"
    assert model.merge_path(39470, True) == "dense" and 4 * 39470 + 4 * ((39470 + 31) // 32) == model.DENSE_MAX_BYTES
    assert model.merge_path(39471, True) == "sorted"
    assert [model.sort_key_bits(R) for R in (1, 2, 3, 4, 5, 8, 9, 13568, 500000)] == [33, 33, 34, 34, 35, 35, 36, 46,
                                                                                      51]


# ---- the dictated inputs -------------------------------------------------------------------------------------
def _check_case(c, path, full_rows=()):
    """What holds for every case: the buffers' shapes, columns < M, a row's total <= M (the named full rows
    apart, whose capacity M still holds their M keys), the true row sums equal to the model's unless a key wraps."""
    assert c.R == model.rows_owned(c.M, c.n, c.part) and len(c.recv_nnz) == c.n * c.R
    assert c.recv_nnz.dtype == np.int32 and c.entries.dtype == np.uint64 and len(c.entries) == int(c.recv_nnz.sum())
    assert model.merge_path(c.M, c.signed) == path
    if len(c.entries):
        assert int((c.entries >> np.uint64(32)).max()) < c.M
    tot = cases.row_totals(c)
    over = np.flatnonzero(tot > c.M)
    assert sorted(over.tolist()) == sorted(int(r) for r in full_rows)
    m = model.merge(c.M, c.n, c.part, c.recv_nnz, c.entries, c.signed)
    assert np.all(np.diff(m.row_ptr) <= np.minimum(tot, c.M))  # the output capacity holds every row
    return m, tot


def _row(m, r):
    s, e = m.row_ptr[r], m.row_ptr[r + 1]
    return m.cols[s:e], m.cnt[s:e]


@pytest.mark.parametrize("M", cases.A_M)
def test_dense_edge_shapes(M):
    per = (-(-M // 16) + 63) // 64 * 64
    widths = [hi - lo for lo, hi in model.wave_ranges(M) if hi > lo]
    assert widths == [per] * ((M - 1) // per) + [M - (M - 1) // per * per]
    edges = cases.wave_edge_cols(M)
    for lo, hi in model.wave_ranges(M):
        if hi > lo:
            assert {lo, hi - 1} <= set(edges.tolist()) and (lo == 0 or lo - 1 in edges)
    owned = 0
    for part in range(cases.A_N):
        c = cases.case_a(M, part)
        a, pat = cases.a_pattern_of(M, part)
        full = np.flatnonzero(pat == cases.A_PATTERNS.index("full"))
        m, tot = _check_case(c, "dense", full_rows=full)
        assert np.array_equal(m.rowsum, c.rowsum)  # nothing wraps
        owned += c.R
        if M == 1:
            assert c.R == (1 if part == 0 else 0)
        if M >= 65:
            assert set(pat.tolist()) == set(range(len(cases.A_PATTERNS)))  # every part sees every pattern
        if M == 40704:
            assert c.R == 13568 and len(full) == cases.A_FULL_ROWS_BIG
        for k, name in enumerate(cases.A_PATTERNS):
            for r in np.flatnonzero(pat == k)[:3]:
                cols, cnt = _row(m, r)
                want = {"col0": [0], "empty": [], "last_col": [M - 1], "wave_edges": edges.tolist(),
                        "full": list(range(M)), "one_col_all": [int(a[r] * 37 % M)]}.get(name)
                if want is not None:
                    assert cols.tolist() == want, (name, r)
                if name == "full":
                    assert tot[r] == c.n * M
                if name == "one_col_all":
                    assert tot[r] == c.n
                if name == "last_source":
                    assert len(cols) == min(5, M) and c.recv_nnz.reshape(c.n, c.R)[:-1, r].sum() == 0
        if c.R:
            r, col = c.tags["max_key"]
            cols, cnt = _row(m, r)
            assert int(cnt[cols.tolist().index(col)]) == U32 and int(m.cnt.max()) == U32
            assert int(np.sum(m.cnt == U32)) == 1
    assert owned == M


@pytest.mark.parametrize("variant", cases.B_VARIANTS)
def test_row_reuse_shapes(variant):
    c = cases.case_b(variant)
    m, tot = _check_case(c, "dense")
    assert c.R == cases.B_M == 2000 and c.n == 1 and c.R / 256 > 7  # about eight rows per workgroup of 256
    nnz = np.diff(m.row_ptr)
    if variant == "alternate":
        assert nnz.tolist() == [2000, 3] * 1000
    else:
        assert nnz[2::3].tolist() == [0] * 666 and sorted(set(nnz.tolist())) == [0, 3, 2000]
        assert nnz[:6].tolist() == [2000, 3, 0, 2000, 3, 0]
        live = nnz[nnz > 0]
        assert live.tolist() == [2000, 3] * (len(live) // 2) + [2000] * (len(live) % 2)
    assert int(m.cnt[:2000].min()) >= 1 << 31  # a full row's counters: all above what a three-column row adds
    assert np.array_equal(m.rowsum, c.rowsum)


@pytest.mark.parametrize("M,n", cases.C_SHAPES)
def test_sorted_edge_shapes(M, n):
    want_R = {(40705, 10000): {0: 5, 704: 5, 705: 4, 9999: 4}}.get((M, n))
    for part in cases.c_parts(M, n):
        for variant in cases.C_VARIANTS:
            c = cases.case_c(M, n, part, variant)
            m, tot = _check_case(c, "sorted")
            assert np.array_equal(m.rowsum, c.rowsum)
            R = c.R
            if want_R:
                assert R == want_R[part] and model.sort_key_bits(R) == {5: 35, 4: 34}[R]
            nnz = np.diff(m.row_ptr)
            if variant == "none":
                assert len(c.entries) == 0 and not c.recv_nnz.any()
                continue
            if variant == "holes":
                assert nnz[0] == nnz[R - 1] == nnz[R // 2] == 0
            else:
                assert nnz[0] > 0 and nnz[R - 1] > 0 and nnz[R // 2] > 0
                k = 1
                while k < R:  # rows on both sides of every power of two
                    assert nnz[k - 1] > 0 and nnz[k] > 0
                    k *= 2
            rows = c.tags["rows"]
            if variant == "every_row":
                assert {int(r) % 3 for r in rows} == {0, 1, 2}
            edge_cols = [x for x in (0, 65535, 65536, M - 1) if x < M]
            assert len(edge_cols) == (4 if M == 1000000 else 2)
            for r in rows[rows % 3 == 0][:3]:
                cols, _ = _row(m, r)
                assert set(edge_cols) < set(cols.tolist()) and len(cols) == len(edge_cols) + 1
                assert tot[r] == len(edge_cols) + n  # the one key more comes from every source
            for r in rows[rows % 3 == 2][:3]:
                assert nnz[r] == tot[r] == (2 if n == 10000 else 3) * n  # disjoint columns
                assert np.all(c.recv_nnz.reshape(n, R)[:, r] == (2 if n == 10000 else 3))


@pytest.mark.parametrize("variant", cases.H_VARIANTS)
def test_sum_by_key_edge_shapes(variant):
    """Group H in sorted order: the received entries around one and two tiles of 4,096, the run that straddles the
    first tile's end, the last element alone, a run of more than 64, no two keys equal, one key only."""
    c = cases.case_h(variant)
    m, tot = _check_case(c, "sorted")
    assert np.array_equal(m.rowsum, c.rowsum)  # nothing wraps
    assert (c.M, c.n, c.R) == (40705, 70, 582) and cases.H_TILE == 4096
    assert c.M - 1 == 40704 and model.merge_path(c.M - 1, False) == "dense"  # the first n_items past the LDS row
    key, _ = model.sorted_keys(c.M, c.n, c.part, c.recv_nnz, c.entries)
    n_recv = len(key)
    first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    runs = np.diff(np.concatenate([first, [n_recv]]))
    assert len(m.cols) == len(runs)  # every run is one merged key
    if variant in cases.H_SIZES:
        assert n_recv == cases.H_SIZES[variant] == int(variant[1:]) and variant[1:] in ("4095", "4096", "4097", "8193")
        assert set(runs.tolist()) == {1, 2, 3} and min(np.bincount(runs)[1:]) > n_recv // 8  # many of each length
    elif variant == "straddle":
        lo, hi = cases.H_STRADDLE
        assert (lo, hi) == (4094, 4098) and n_recv > hi + 1
        k = np.flatnonzero(first == lo)
        assert len(k) == 1 and runs[k[0]] == hi - lo + 1 == 5  # sorted positions 4,094 .. 4,098 hold one key
        assert key[lo - 1] != key[lo] and key[hi + 1] != key[hi] and np.all(key[lo:hi + 1] == key[lo])
    elif variant == "last_alone":
        assert runs[-1] == 1 and first[-1] == n_recv - 1 and runs[-2] > 1
        assert int(key[-1]) == ((c.R - 1) << 32) | (c.M - 1)
    elif variant == "long_run":
        k = np.flatnonzero(runs > 64)
        assert len(k) == 1 and runs[k[0]] == 70 == c.n and 0 < k[0] < len(runs) - 1
        assert int(key[first[k[0]]]) == (cases.H_LONG_KEY[0] << 32) | cases.H_LONG_KEY[1]
    elif variant == "distinct":
        assert n_recv == 5000 > cases.H_TILE and np.all(runs == 1)
    else:
        assert variant == "one_key" and runs.tolist() == [66] and n_recv == 66 > 64


@pytest.mark.parametrize("part", cases.D_PARTS)
def test_both_paths_shapes(part):
    c = cases.case_d(part)
    _check_case(c, "dense")
    assert c.M == 40704 and 190000 < len(c.entries) <= cases.D_ENTRIES
    for M in cases.D_M:
        assert model.rows_owned(M, cases.D_N, part) == cases.D_R == c.R
    assert model.merge_path(cases.D_M[1], False) == "sorted"
    a = model.merge(cases.D_M[0], c.n, part, c.recv_nnz, c.entries, False)
    b = model.merge(cases.D_M[1], c.n, part, c.recv_nnz, c.entries, False)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert len(a.cols) < len(c.entries)  # some keys come from several sources


@pytest.mark.parametrize("M", cases.E_M)
def test_overflow_shapes(M):
    path = "dense" if M == 700 else "sorted"
    r, col = cases.E_KEY
    c = cases.case_e(M, 1 << 31)
    m, _ = _check_case(c, path)
    assert col not in _row(m, r)[0]  # the model's unsigned merge: the wrapped key sums to 0
    assert int(c.rowsum[r]) - int(m.rowsum[r]) == 1 << 32 and np.array_equal(np.delete(c.rowsum, r),
                                                                             np.delete(m.rowsum, r))
    ok = cases.case_e(M, (1 << 31) - 1)
    m, _ = _check_case(ok, path)
    cols, cnt = _row(m, r)
    assert int(cnt[cols.tolist().index(col)]) == U32 - 1 and np.array_equal(m.rowsum, ok.rowsum)
    assert np.array_equal(ok.recv_nnz, c.recv_nnz)  # the same input but for the two counts


@pytest.mark.parametrize("M", cases.F_M)
def test_signed_shapes(M):
    for n in cases.F_N:
        for part in range(n):
            c = cases.case_f(M, n, part)
            m, tot = _check_case(c, "dense" if M <= 39470 else "sorted")
            assert c.signed and np.array_equal(m.rowsum, c.rowsum)
            assert c.R >= 2 * len(cases.F_PATTERNS)
            rows = c.tags["rows"]
            unsigned = model.merge(M, n, part, c.recv_nnz, c.entries, False)
            for r in rows("cancel")[:3]:
                cols, cnt = _row(m, r)
                assert cnt.tolist() == [0, 7] and len(_row(unsigned, r)[0]) == 1  # kept at net 0 only when signed
            for r in rows("negative")[:3]:
                assert np.all(_row(m, r)[1].view(np.int32) < 0) and m.rowsum[r] < 0
            for r in rows("all_cancel")[:3]:
                assert _row(m, r)[1].tolist() == [0] * 4 and m.rowsum[r] == 0 and tot[r] == 4 * n
            for r in rows("negative_sum")[:3]:
                assert m.rowsum[r] == -102 and sorted(_row(m, r)[1].view(np.int32).tolist()) == [-100, -7, 5]
            for r in rows("word_edges")[:3]:
                cols, cnt = _row(m, r)
                assert cols.tolist() == sorted({31, 32, 63, 64, M - 1})
                assert cnt[1] == 0 and set(np.delete(cnt.view(np.int32), 1).tolist()) == {4, -4}
            assert all(tot[r] == 0 for r in rows("empty")[:3])
            # a sum read without sign extension would differ in every row with a negative net
            wrong = np.zeros(c.R, np.int64)
            np.add.at(wrong, np.repeat(np.arange(c.R), np.diff(m.row_ptr)), m.cnt.astype(np.int64))
            assert np.sum(wrong != m.rowsum) >= c.R // 3


@pytest.mark.parametrize("M,n_parts", [(130, 1), (130, 2), (130, 3), (130, 7), (130, 130), (130, 133), (41000, 2),
                                       (41000, 3)])
def test_pack_round_trip_shapes(oracle, pkg, M, n_parts):
    """The round trip of the GPU test in the model alone: the shards' closed forms packed, sliced as an all-to-all
    would and merged equal the closed form of the whole log."""
    up, it = cases.g_log(M)
    assert len(up) - 1 == 300
    assert model.merge_path(M, False) == ("dense" if M == 130 else "sorted")
    packs = []
    for sup, sit in cases.g_shards(up, it, n_parts):
        assert len(sup) >= 2
        rp, cols, data, _, _ = oracle.closed_form(sup, sit, M)
        packs.append(model.pack(rp, cols, data, M, n_parts))
    rp, cols, data, rowsums, _ = oracle.closed_form(up, it, M)
    for part in range(n_parts):
        nnz, ent = cases.slice_for_owner(packs, M, n_parts, part)
        m = model.merge(M, n_parts, part, nnz, ent, False)
        own = np.arange(part, M, n_parts)
        assert len(own) == model.rows_owned(M, n_parts, part) and (part < 130 or len(own) == 0)
        assert np.array_equal(np.diff(m.row_ptr), np.diff(rp)[own])
        idx = np.repeat(rp[own], np.diff(rp)[own]) + model._ramp(np.diff(rp)[own])
        assert np.array_equal(m.cols, cols[idx]) and np.array_equal(m.cnt.astype(np.int64), data[idx])
        assert np.array_equal(m.rowsum, rowsums[own])
