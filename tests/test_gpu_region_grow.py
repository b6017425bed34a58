"""The large-universe path's output region, grown and the attempt repeated (Counter::run_sparse, cooc_sparse.hip).

The region is sized from the planner's estimate of the distinct keys (est_nnz * 1.25 + slab slack), not from the
exact bound.  A batch far more diverse than its item frequencies predict exhausts it: a kernel sets error bit 4,
the host grows the region to the exact bound and repeats the whole attempt -- staging rows re-zeroed, bump pointer,
queue counters and n_deferred reset, every row_base / row_nnz of the failed attempt overwritten.  The logs here
reach that through the public API alone: users that hold thousands of ids which occur nowhere else (rows of ~2,500
distinct partners where the global frequencies predict ~100), beside a mass of interactions on a few columns.

Every log has a precondition, asserted on any machine (test_logs_force_the_grow, no GPU): its true entry count,
known from its construction, is at least 1.5 x the first region as modelled on the CPU (est_model, slack_model:
restatements of k_sp_est / est_distinct / k_sp_plan's est_sum and of sparse_sizes' R.slack at its largest).  The
1.5 covers what the model leaves out: float rounding in the estimate table, and occupancy results below the 2 and
4 workgroups per CU assumed (fewer workgroups only shrink the slack).

Scenarios (bit-exact; the GPU ones need an MI355X):
  A  small rows only (k_sp_small), the smallest log that exhausts the region; both emission orders.
  B  a split row mirrored from the small rows: the staging rows take mirrored stores in both attempts.
  C  B plus a mid row whose hash table overflows: grow, then the repeat without mirroring on a rebuilt queue,
     then the sort path; three attempts, both emission orders.
  D  A's log over 2 owned parts: every part grows; the parts' rows are disjoint and equal the whole count's.
  E  one context: a six-interaction log, A, the small log again, A again.
"""
import time

import numpy as np
import pytest

from tests.test_gpu_sparse import _Brute, _check_rows, _Rows

_TW = 16384  # k_sp_main's tile width
_M = 300_000
_MARGIN = 1.5  # true entries >= _MARGIN x the modelled first region


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


# ---- the CPU model of the first region ------------------------------------------------------------------------

def est_model(W, freq, n_total):
    """Sum over the rows (pair works W, all > 0) of the planner's expected distinct keys: the table
    E[k] = sum_b 1 - exp(-2^(k/2) f_b / N), k < 84 (k_sp_est, summed over the tiles), interpolated linearly in
    x = 2 log2(W) between E[floor(x)] and E[floor(x) + 1] (est_distinct), truncated, + 1 (k_sp_plan's est_sum)."""
    f, mult = np.unique(freq[freq > 0], return_counts=True)
    k = np.arange(84, dtype=np.float64)
    E = (-np.expm1(-np.exp2(0.5 * k)[:, None] * f[None, :] / float(n_total)) * mult[None, :]).sum(axis=1)
    uW, n_rows = np.unique(np.asarray(W, np.int64), return_counts=True)
    x = 2.0 * np.log2(uW.astype(np.float32)).astype(np.float64)
    kk = np.minimum(x.astype(np.int64), 83)
    frac = np.where(kk < 83, x - kk, 0.0)
    e = E[kk] + frac * (E[np.minimum(kk + 1, 83)] - E[kk])
    return int(np.sum((e.astype(np.int64) + 1) * n_rows))


def slack_model(W, est, M, n_cu):
    """sparse_sizes' R.slack at its largest: the rows classified by pair work at 256 (tiny), 4,096 (small) and
    65,535 (mid); the big launch's items are the other whole rows plus the split rows' shares (rows above 2^23
    pairs; at most max(ceil(W / 2^24), ceil(W / (3 * 2^21))) shares each, the tail bounded by the whole row);
    two big and four mid workgroups per CU."""
    W = np.asarray(W, np.int64)
    n_tiny = int(np.sum(W <= 256))
    n_small = int(np.sum((W > 256) & (W <= 4096)))
    n_mid = int(np.sum((W > 4096) & (W <= 65535)))
    split = W[W > 2 ** 23]
    shares = np.maximum(-(-split // 2 ** 24), -(-split // (3 * 2 ** 21)))
    n_big = int(np.sum((W > 65535) & (W <= 2 ** 23))) + int(shares.sum())
    small_slab, tiny_slab, tiny_waves = 16384, 4096, 4
    grid = min(max(n_big, 1), 2 * n_cu)
    grid_mid = min(max(n_mid, 1), 4 * n_cu)
    slab = max(2 ** 16, min(2 ** 22, est // (8 * grid)))
    grid_small = min(n_small, 4 * n_cu)
    grid_tiny = min(-(-n_tiny // tiny_waves), 8 * n_cu)
    return (2 * grid * slab + (2 * grid_mid * slab if n_mid else 0) + M
            + (grid_tiny * tiny_waves * tiny_slab if n_tiny else 0) + (grid_small * small_slab if n_small else 0)
            + 2 * n_cu * small_slab)


def first_region_model(log, n_cu, rows=None):
    """(estimate, slack, first region = 1.25 estimate + slack) of a count of the log's rows (rows: a mask, the
    rows of an owned part; the frequencies stay the whole log's)."""
    W = log.W if rows is None else np.where(rows, log.W, 0)
    W = W[W > 0]
    est = est_model(W, log.freq, len(log.it))
    slack = slack_model(W, est, log.M, n_cu)
    return est, slack, est + est // 4 + slack


# ---- the logs ------------------------------------------------------------------------------------------------

class _Log:
    """A log of bulk lists (a U x k id matrix over a few hot ids) followed by extra lists, each a hot part and a
    private part: ids that occur once in the whole log.  From that construction every row's true entry count:
    the hot-hot cells from the lists' hot-id count matrices, + a list's private ids on every hot row the list
    holds; a private id's row holds its list's other private ids and distinct hot ids."""

    def __init__(self, M, bulk, extras, extra_lists):
        self.M = M
        lists = [bulk.reshape(-1)] + extra_lists
        self.it = np.ascontiguousarray(np.concatenate(lists), np.int32)
        U, k = bulk.shape
        self.up = np.concatenate([np.arange(U + 1, dtype=np.int64) * k,
                                  U * k + np.cumsum([len(x) for x in extra_lists], dtype=np.int64)])
        self.lens = np.diff(self.up)
        self.observed = int(np.sum(self.lens * (self.lens - 1)))
        self.freq = np.bincount(self.it, minlength=M).astype(np.int64)
        self.W = np.bincount(self.it, weights=np.repeat(self.lens, self.lens).astype(np.float64),
                             minlength=M).astype(np.int64)  # (sums below 2^53: exact)
        hot = np.unique(np.concatenate([bulk.reshape(-1)] + [h for h, _ in extras]))
        H = len(hot)
        cnt = np.bincount(np.repeat(np.arange(U, dtype=np.int64), k) * H + np.searchsorted(hot, bulk.reshape(-1)),
                          minlength=U * H).reshape(U, H).astype(np.float64)
        G = cnt.T @ cnt - np.diag(cnt.sum(axis=0))  # (integers below 2^53: exact)
        nnz = np.zeros(M, np.int64)
        for (h, p), lst in zip(extras, extra_lists):
            assert sorted(lst.tolist()) == sorted(np.concatenate([h, p]).tolist())
            assert np.all(self.freq[p] == 1), "a private id occurs elsewhere"
            c = np.bincount(np.searchsorted(hot, h), minlength=H).astype(np.float64)
            G += np.outer(c, c) - np.diag(c)
            nnz[hot[c > 0]] += len(p)
            nnz[p] = int(np.count_nonzero(c)) + len(p) - 1
        nnz[hot] += np.count_nonzero(G > 0, axis=1)
        self.row_nnz = nnz
        self.entries = int(nnz.sum())
        self._brute = None

    @property
    def brute(self):
        if self._brute is None:
            self._brute = _Brute(self.up, self.it, self.M)
        return self._brute


def _log_a():
    """A: 200,000 users of two ids from the ten columns 8192..8201 (the global mass), 12 users of 2,500 private
    ids each.  A private id's row: 2,500 pairs (k_sp_small), 2,499 partners, ~190 expected."""
    rng = np.random.default_rng(51)
    bulk = rng.integers(8192, 8202, (200_000, 2)).astype(np.int32)
    priv = rng.permutation(np.arange(20_000, _M, dtype=np.int32))[:12 * 2500].reshape(12, 2500)
    none = np.zeros(0, np.int32)
    log = _Log(_M, bulk, [(none, priv[u]) for u in range(12)], [priv[u] for u in range(12)])
    empty = np.flatnonzero(log.freq == 0)[:1]
    log.sample = np.concatenate([np.arange(8192, 8202), priv[0, :4], priv[5, 100:108], priv[11, -8:], empty])
    return log


def _logs_bc():
    """B: 290,000 users of 31 ids -- item 0, 15 of the ids [1, 33), 15 of [16384, 16416) (no mid rows: 64 big rows
    and the split row 0) -- and 16 users of item 0 plus 2,500 private ids >= 20,000 each: small rows above tile 0,
    mirror sources of row 0 with kept ids.  C: B plus three lists [ovf, 2,500 own ids, 0, 7, 7]: the mid row ovf
    overflows its hash table."""
    rng = np.random.default_rng(53)
    U, ovf = 290_000, 250_000
    lo = 1 + np.argsort(rng.random((U, 32)), axis=1)[:, :15]
    hi = _TW + np.argsort(rng.random((U, 32)), axis=1)[:, :15]
    bulk = rng.permuted(np.concatenate([np.zeros((U, 1), np.int64), lo, hi], axis=1), axis=1).astype(np.int32)
    priv = rng.permutation(np.arange(20_000, 100_000, dtype=np.int32))[:16 * 2500].reshape(16, 2500)
    own = rng.permutation(np.arange(100_000, 100_000 + _TW, dtype=np.int32))[:7500].reshape(3, 2500)
    zero = np.zeros(1, np.int32)
    ex_b = [(zero, priv[u]) for u in range(16)]
    ls_b = [np.concatenate([zero, priv[u]]) for u in range(16)]
    hot_c = np.array([ovf, 0, 7, 7], np.int32)
    ex_c = ex_b + [(hot_c, own[k]) for k in range(3)]
    ls_c = ls_b + [np.concatenate([[ovf], own[k], [0, 7, 7]]).astype(np.int32) for k in range(3)]
    b, c = _Log(_M, bulk, ex_b, ls_b), _Log(_M, bulk, ex_c, ls_c)
    b.sample = np.concatenate([[0, 1, 2, 17, 32, _TW, _TW + 1, _TW + 16, _TW + 31],
                               priv[0, :5], priv[7, 1000:1010], priv[15, -5:]])
    c.sample = np.concatenate([b.sample, [ovf, 7], own[0, :3], own[2, 17:20]])
    c.ovf = ovf
    return b, c


_LOGS = {}


def _log(name):
    if not _LOGS:
        _LOGS["A"] = _log_a()
        _LOGS["B"], _LOGS["C"] = _logs_bc()
    return _LOGS[name]


def _owner_a(log):
    """D's owner map: alternating over the ids that occur."""
    occ = np.flatnonzero(log.freq > 0)
    owner = np.zeros(log.M, np.int32)
    owner[occ] = np.arange(len(occ), dtype=np.int32) % 2
    return owner


def _assert_precondition(log, n_cu, name):
    est, slack, first = first_region_model(log, n_cu)
    print(f"{name}: n_cu {n_cu}: modelled estimate {est}, slack {slack}, first region {first}; true entries "
          f"{log.entries}; ratio {log.entries / first:.3f}")
    assert log.entries >= _MARGIN * first, f"log {name} no longer forces the region to grow"
    return first


def test_logs_force_the_grow():
    """Every scenario's log (D and E use A's), with 256 CUs: true entries >= 1.5 x (1.25 est_model + slack_model).
    A: estimate ~5.7e6, first region <= 3.4e7 against 7.5e7 entries; B, C: first region <= 4.1e7 against 1.0e8.
    The classes the scenarios are built around are asserted with it.  D's parts each hold half of A's private rows
    under the whole slack (the owner map and the part count are the scenario's): their entries exceed the
    modelled first region by 1.2, not 1.5 -- still above a region whose slack is modelled at its largest."""
    a, b, c = _log("A"), _log("B"), _log("C")
    for name, log in (("A", a), ("B", b), ("C", c)):
        _assert_precondition(log, 256, name)
    Wa = a.W[a.W > 0]
    assert int(np.sum((Wa > 256) & (Wa <= 4096))) == 30_000 and int(np.sum(Wa > 65535)) == 10 and len(Wa) == 30_010
    assert np.all(a.row_nnz[a.W == 2500] == 2499) and a.entries >= 12 * 2500 * 2499
    for log in (b, c):
        W = log.W
        assert np.flatnonzero(W > 2 ** 23).tolist() == [0]  # one split row, in tile 0
        assert int(np.sum((W > 65535) & (W <= 2 ** 23))) == 64
        assert int(np.sum((W > 4096) & (W <= 65535))) == (1 if log is c else 0)
        assert log.entries >= 16 * 2501 * 2500
    assert 4096 < c.W[c.ovf] <= 65535 and c.row_nnz[c.ovf] == 7502
    owner = _owner_a(a)
    for part in range(2):
        mine = (owner == part) & (a.freq > 0)
        first = first_region_model(a, 256, mine)[2]
        entries = int(a.row_nnz[mine].sum())
        print(f"D part {part}: modelled first region {first}, true entries {entries}, ratio {entries / first:.3f}")
        assert entries > first


# ---- the GPU scenarios ---------------------------------------------------------------------------------------

def _n_cu(torch):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _check_regions(rows, region_entries):
    """The rows' regions [row_base, row_base + row_nnz), row_nnz > 0: pairwise disjoint, inside the region (a
    row_base left over from the failed attempt points into another row's entries, or past a smaller region)."""
    live = np.flatnonzero(rows.nnz > 0)
    o = live[np.argsort(rows.base[live], kind="stable")]
    b, e = rows.base[o], rows.base[o] + rows.nnz[o]
    assert len(o) > 0 and b[0] >= 0 and e[-1] <= region_entries
    assert np.all(e[:-1] <= b[1:]), "two rows' regions overlap"


def _count_whole(core, torch, log, name, want_attempts):
    """One count of the whole log on core, with every whole-log check; returns (res, rows)."""
    dev = torch.device("cuda")
    t0 = time.perf_counter()
    res = core.count_device(torch.from_numpy(log.up).to(dev), torch.from_numpy(log.it).to(dev))
    torch.cuda.current_stream().synchronize()
    attempts, region = core.last_attempts()
    print(f"{name}: attempts {attempts}, region entries {region}, entries {res.nnz}, mirror rows "
          f"{core.last_mirror_rows()}, sort rows {core.last_sort_rows()[0]}, count {time.perf_counter() - t0:.2f} s")
    assert attempts == want_attempts
    assert region >= log.entries
    assert res.observed == log.observed
    rows = _Rows(res, log.M)
    assert int(rows.rowsum.sum()) == res.observed
    assert int(rows.nnz.sum()) == res.nnz == log.entries
    assert np.array_equal(rows.nnz, log.row_nnz)
    chk = core.verify_batch()
    assert chk["rows_bad_sum"] == 0 and chk["rows_bad_entries"] == 0
    assert chk["sum_counts"] == chk["sum_rowsums"] == res.observed
    _check_regions(rows, region)
    _check_rows(rows, log.brute, log.sample)
    return res, rows


@pytest.mark.gpu
@pytest.mark.parametrize("any_order", [False, True])
def test_small_rows_exhaust_the_region(pkg, torch_cuda, any_order):
    """A: two attempts, the second into a region of at least the true entry count."""
    log = _log("A")
    _assert_precondition(log, _n_cu(torch_cuda), "A")
    with pkg.CooccurrenceCore(n_items=log.M, device=0, any_order=any_order) as core:
        _count_whole(core, torch_cuda, log, f"A any_order={any_order}", 2)
        assert core.last_mirror_rows() == 0 and core.last_sort_rows()[0] == 0


@pytest.mark.gpu
def test_grow_with_split_row_mirrored(pkg, torch_cuda):
    """B: the repeated attempt is still mirrored, so row 0's staging row took mirrored stores in both attempts
    (it is re-zeroed between them); row 0, heavy rows on both sides of column 16384 and private rows exact."""
    log = _log("B")
    _assert_precondition(log, _n_cu(torch_cuda), "B")
    with pkg.CooccurrenceCore(n_items=log.M, device=0, column_order=True) as core:
        _count_whole(core, torch_cuda, log, "B", 2)
        assert core.last_mirror_rows() >= 1
        assert core.last_sort_rows()[0] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("any_order", [False, True])
def test_grow_then_mirror_repeat_then_sort_path(pkg, torch_cuda, any_order):
    """C: the first attempt exhausts the region; the second, mirrored, defers the overflowing mid row; the third
    runs without mirroring on a rebuilt queue (its est fields come from the row_nnz the earlier attempts wrote),
    then the sort path takes the deferred row."""
    log = _log("C")
    _assert_precondition(log, _n_cu(torch_cuda), "C")
    with pkg.CooccurrenceCore(n_items=log.M, device=0, any_order=any_order, column_order=True) as core:
        _count_whole(core, torch_cuda, log, f"C any_order={any_order}", 3)
        assert core.last_mirror_rows() == 0
        assert core.last_sort_rows()[0] >= 1, "the overflowing row was not deferred"


@pytest.mark.gpu
def test_owned_parts_each_grow_and_equal_the_whole(pkg, torch_cuda):
    """D: A's log over 2 owned parts (owner alternating over the ids that occur, item_counts the log's own):
    every part takes two attempts, counts exactly its own rows, and equals the whole count on the sample."""
    torch = torch_cuda
    log = _log("A")
    owner = _owner_a(log)
    dev = torch.device("cuda")
    up_d, it_d = torch.from_numpy(log.up).to(dev), torch.from_numpy(log.it).to(dev)
    freq_d, owner_d = torch.from_numpy(log.freq).to(dev), torch.from_numpy(owner).to(dev)
    with pkg.CooccurrenceCore(n_items=log.M, device=0) as core:
        _, w = _count_whole(core, torch, log, "D whole", 2)
        want = {int(a): w.row(int(a)) for a in log.sample}
        w_rowsum = w.rowsum.copy()
    for part in range(2):
        mine = owner == part
        with pkg.CooccurrenceCore(n_items=log.M, device=0) as core:
            res = core.count_device_owned(up_d, it_d, owner_d, part, freq_d, int(len(log.it)))
            torch.cuda.current_stream().synchronize()
            attempts, region = core.last_attempts()
            entries = int(log.row_nnz[mine].sum())
            print(f"D part {part}: attempts {attempts}, region entries {region}, entries {res.nnz}")
            assert attempts == 2 and region >= entries
            r = _Rows(res, log.M)
            assert res.nnz == entries == int(r.nnz.sum())
            assert np.array_equal(r.nnz[mine], log.row_nnz[mine]) and np.all(r.nnz[~mine] == 0)
            assert np.array_equal(r.rowsum[mine], w_rowsum[mine])
            assert res.observed == int(w_rowsum[mine].sum())
            chk = core.verify_batch()
            assert chk["rows_bad_sum"] == 0 and chk["rows_bad_entries"] == 0
            assert chk["sum_counts"] == chk["sum_rowsums"] == res.observed
            _check_regions(r, region)
            n_mine = 0
            for a, (wc, wn) in want.items():
                if mine[a]:
                    gc, gn = r.row(a)
                    assert np.array_equal(gc, wc) and np.array_equal(gn, wn)
                    n_mine += len(wc) > 0
            assert n_mine >= 5


@pytest.mark.gpu
def test_context_reuse_around_a_grow(pkg, oracle, torch_cuda):
    """E: one context counts a six-interaction ragged log, A, the ragged log again, A again.  The ragged results
    are the closed form's both times; both A runs take two attempts (the region is sized from the estimate,
    however large the buffers already are) and give the same rows."""
    torch = torch_cuda
    log = _log("A")
    lens = [0, 2, 0, 3, 1, 0]
    rng = np.random.default_rng(len(lens))
    up = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    it = rng.choice([0, 1, 7, 40_000, log.M - 1], int(up[-1])).astype(np.int32)
    rp, cols, data, rowsums, observed = oracle.closed_form(up, it, log.M)
    dev = torch.device("cuda")

    def ragged(core):
        res = core.count_device(torch.from_numpy(up).to(dev), torch.from_numpy(it).to(dev))
        torch.cuda.current_stream().synchronize()
        assert core.last_attempts()[0] == 1
        got = core.copy_batch(res.nnz, res.observed)
        assert got.observed == observed and res.nnz == len(cols)
        assert np.array_equal(got.row_ptr, rp) and np.array_equal(got.cols, cols)
        assert np.array_equal(got.cnt.astype(np.int64), data) and np.array_equal(got.rowsum, rowsums)
        return got

    with pkg.CooccurrenceCore(n_items=log.M, device=0) as core:
        g0 = ragged(core)
        _, r1 = _count_whole(core, torch, log, "E first A", 2)
        a1 = {int(a): r1.row(int(a)) for a in log.sample}
        nnz1, rowsum1 = r1.nnz.copy(), r1.rowsum.copy()
        g1 = ragged(core)
        for x, y in ((g0.row_ptr, g1.row_ptr), (g0.cols, g1.cols), (g0.cnt, g1.cnt), (g0.rowsum, g1.rowsum)):
            assert np.array_equal(x, y)
        _, r2 = _count_whole(core, torch, log, "E second A", 2)
        assert np.array_equal(r2.nnz, nnz1) and np.array_equal(r2.rowsum, rowsum1)
        for a, (c1, n1) in a1.items():
            c2, n2 = r2.row(a)
            assert np.array_equal(c1, c2) and np.array_equal(n1, n2)
