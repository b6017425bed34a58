"""cooc_verify_batch (k_verify_csr, k_verify_dense, k_verify_symmetry: csrc/cooc_verify.hip) on CORRUPTED results,
one defect at a time.  Needs an MI355X.

The benchmark's gate, the C3-sized exactness tests and the "columns strictly ascending in the device's own order"
contract of the sparse tests all rest on that checker, and every other call of it in the suite is on a correct
result.  Here a small log is counted, single words of the result are overwritten in device memory, and the whole
report and every row's fingerprint must equal (a) tests/_verify_model.py, a numpy restatement of the contract
text of include/cooc.h, run on the same mutated host copy, and (b) the numbers stated by hand at each case
(counters [3] and [4] count rows, [5] counts entries).  Then the words go back and the report must be the clean
one again (the totals buffer is zeroed by every call).

Layouts: D dense (k_verify_dense); C padded CSR of the batch planner (ascending ids, no column-order table); R the
large-universe planner with its column relabel (rows ascending in column_order(), not in id); U as R with
any_order (no order check, no symmetry search); G a 33,001-item universe, whose rows from 32,768 on are a wave's
second trip through its row loop (the grid is capped at 32,768 waves).  Positions in a row are 0, 63, 64, 127,
128, n - 1 for single entries and 0, 62, 63, 64, n - 2 for neighbours (63: the pair whose second element belongs
to the next 64-entry step of the wave).

What the tests write stays inside mapped memory: words inside [row_base[a], row_base[a] + row_nnz[a]) of col /
cnt, single words of row_nnz / rowsum, cells of the dense matrix; a CSR row_nnz never grows; the only
out-of-range columns are n_items and (layout C, which has no column-order table to index) -1.
"""
import ctypes
import os

import numpy as np
import pytest

from tests import _verify_model as vm

pytestmark = pytest.mark.gpu

SINGLE = (0, 63, 64, 127, 128, -1)  # (-1: the row's last entry)
PAIRS = (0, 62, 63, 64, -2)
MIN_ROW = 130  # entries a row needs for every position above


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_HIP = None


def _memcpy(dst, src, nbytes, kind):
    global _HIP
    if _HIP is None:
        _HIP = ctypes.CDLL("libamdhip64.so")
    assert _HIP.hipMemcpy(ctypes.c_void_p(dst), ctypes.c_void_p(src), ctypes.c_size_t(nbytes), ctypes.c_int(kind)) == 0


def _d2h(ptr, n, dtype, offset=0):
    out = np.zeros(n, dtype)
    if n:
        _memcpy(out.ctypes.data, ptr + offset * out.itemsize, out.nbytes, 2)
    return out


# ---- the logs -------------------------------------------------------------------------------------------------
def _log_a():
    """10,040 records over 300 items: rows of 28 to 300 entries."""
    from flink_cooccurrence_amd import datagen

    up, it = datagen.small_log(7, 250, 300, 40.0)
    assert len(it) == 10_040
    return up, it.astype(np.int32), 300


R_ITEMS = 40_000


def _log_r():
    """Log A with its ids sent through a fixed permutation of a 40,000-item universe (its three most frequent items
    to 0, M - 1 and M / 2), plus 16,384 filler items of two interactions each, in users of their own.  The column
    relabel needs more than 16,384 columns, and it is the identity on the columns a row holds unless the log uses more
    than 16,384 items: the filler items push log A's two single-interaction items (keys of every full row) out of
    the 16,384 most frequent ones, so those keys sort behind every hot column whatever their id."""
    up, it, _ = _log_a()
    M = R_ITEMS
    perm = np.random.default_rng(5).permutation(M)
    for src, dst in ((0, 0), (1, M - 1), (2, M // 2)):
        j = int(np.flatnonzero(perm == dst)[0])
        perm[src], perm[j] = perm[j], perm[src]
    pairs = perm[300:300 + 16_384].reshape(-1, 2)
    filler = np.concatenate([pairs, pairs]).reshape(-1)  # every pair of filler items as two users
    up_r = np.concatenate([up, up[-1] + 2 * np.arange(1, len(filler) // 2 + 1)]).astype(np.int64)
    it_r = np.concatenate([perm[it], filler]).astype(np.int32)
    assert len(np.unique(it_r)) == 300 + 16_384
    return up_r, it_r, M


def _log_b():
    """9,036 records over S = ids 0..99 and 32,700..33,000: 60 users of 150 distinct ids, every fifth repeating
    its first three (diagonal keys)."""
    S = np.concatenate([np.arange(100), np.arange(32_700, 33_001)])
    rng = np.random.default_rng(11)
    lists = []
    for u in range(60):
        x = rng.choice(S, 150, replace=False)
        lists.append(np.concatenate([x, x[:3]]) if u % 5 == 0 else x)
    up = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    it = np.concatenate(lists).astype(np.int32)
    assert len(it) == 9_036
    return up, it, 33_001


LAYOUTS = {
    "D": (_log_a, dict(output="dense")),
    "C": (_log_a, dict(output="csr")),
    "R": (_log_r, dict(output="csr", planner="large")),
    "U": (_log_r, dict(output="csr", planner="large", any_order=True)),
    "G": (_log_b, dict(output="csr")),
}


# ---- a counted result: device views, a host copy that every write goes through, the checker and the model ------
class _Result:
    def __init__(self, pkg, torch, name):
        log, opts = LAYOUTS[name]
        self.name, self.torch = name, torch
        self.up, self.it, self.M = log()
        self.ordered = not opts.get("any_order", False)
        dev = torch.device("cuda", 0)
        self.up_d, self.it_d = torch.from_numpy(self.up).to(dev), torch.from_numpy(self.it).to(dev)
        self.core = pkg.CooccurrenceCore(n_items=self.M, device=0, **opts)
        self.cs = torch.zeros(self.M, dtype=torch.int64, device=dev)
        self.count()

    def count(self):
        M = self.M
        self.res = res = self.core.count_device(self.up_d, self.it_d)
        self.torch.cuda.synchronize()
        self.dense = bool(res.dense)
        self.ptr = {"row_nnz": res.row_nnz, "rowsum": res.rowsum}
        self.host = {"row_nnz": _d2h(res.row_nnz, M, np.int32), "rowsum": _d2h(res.rowsum, M, np.int64)}
        if self.dense:
            self.ptr["dense"] = res.dense
            self.host["dense"] = _d2h(res.dense, M * M, np.uint32)
        else:
            self.base = _d2h(res.row_base, M, np.int64)
            nnz = self.host["row_nnz"].astype(np.int64)
            extent = int(np.max(np.where(nnz > 0, self.base + nnz, 0)))
            self.ptr.update(col=res.col, cnt=res.cnt)
            self.host.update(col=_d2h(res.col, extent, np.int32), cnt=_d2h(res.cnt, extent, np.uint32))
        self.nnz0 = self.host["row_nnz"].copy()
        self.order = self.core.column_order()
        self.undo = []

    def close(self):
        self.core.close()

    # -- reads of the host copy
    def row(self, a):
        s = slice(int(self.base[a]), int(self.base[a]) + int(self.nnz0[a]))
        return self.host["col"][s], self.host["cnt"][s]

    def pos(self, a, p):
        n = int(self.nnz0[a])
        return p if p >= 0 else n + p

    def find(self, a, key):
        """Position of column `key` in row a, or None."""
        hit = np.flatnonzero(self.row(a)[0] == key)
        return int(hit[0]) if len(hit) else None

    # -- single-word writes: host copy and device memory together
    def _write(self, name, index, value):
        h = self.host[name]
        h[index] = value
        _memcpy(self.ptr[name] + index * h.itemsize, h[index:index + 1].ctypes.data, h.itemsize, 1)

    def _poke(self, name, index, value):
        self.undo.append((name, index, self.host[name][index].copy()))
        self._write(name, index, value)

    def poke_entry(self, a, p, col=None, cnt=None):
        assert not self.dense and 0 <= p < int(self.nnz0[a]), "writes stay inside the row"
        i = int(self.base[a]) + p
        if col is not None:
            assert 0 <= col <= self.M or (col == -1 and self.name == "C"), "no far out-of-range column"
            self._poke("col", i, col)
        if cnt is not None:
            self._poke("cnt", i, cnt)

    def poke_nnz(self, a, value):
        assert self.dense or value <= int(self.nnz0[a]), "a CSR row never grows"
        self._poke("row_nnz", a, value)

    def poke_rowsum(self, a, value):
        self._poke("rowsum", a, value)

    def poke_cell(self, a, c, value):
        assert self.dense and 0 <= a < self.M and 0 <= c < self.M
        self._poke("dense", a * self.M + c, value)

    def restore(self):
        for name, index, old in reversed(self.undo):
            self._write(name, index, old)
        self.undo = []

    # -- the device checker and the model, on the same words
    def verify(self, symmetry=True):
        self.cs.fill_(-1)  # (every row's fingerprint is written by every call)
        rep = self.core.verify_batch(symmetry=symmetry, row_checksum=self.cs)
        return rep, self.cs.cpu().numpy().view(np.uint64).copy()

    def model(self, symmetry=True):
        h = self.host
        if self.dense:
            return vm.verify_dense(h["dense"].reshape(self.M, self.M), h["row_nnz"], h["rowsum"])
        return vm.verify_csr(self.base, h["row_nnz"], h["col"], h["cnt"], h["rowsum"], self.order,
                             ordered=self.ordered, symmetry=symmetry)


def _exp(counts=0, rowsums=0, entries=0, bad_sum=None, bad_rows=None, asym="model", changed=()):
    """The numbers stated by hand for a case: the three sums relative to the clean report, [3] and [4] (None: left
    to the model), [5] (a number; "model"; "some": at least 1 and no less than the model, the search may miss more
    keys of a row that holds an out-of-range column; "skip": not compared, the search presumes sorted rows of
    distinct keys), and the rows whose fingerprint changes (every other row's must not)."""
    return dict(counts=counts, rowsums=rowsums, entries=entries, bad_sum=bad_sum, bad_rows=bad_rows, asym=asym,
                changed=tuple(changed))


class _Cases:
    """Runs cases on one result, collects every failure (so that one run names all the cases a defect trips)."""

    def __init__(self, L):
        self.L, self.fails, self.ran = L, [], 0
        self.clean, self.clean_cs = L.verify()

    def _compare(self, label, exp):
        L, clean = self.L, self.clean
        sym_checked = L.ordered and not L.dense
        rep, cs = L.verify()
        want, want_cs = L.model()
        bad = []
        for k in vm.KEYS[:5]:
            if rep[k] != want[k]:
                bad.append(f"{k} {rep[k]}, model {want[k]}")
        hand = {"sum_counts": clean["sum_counts"] + exp["counts"], "sum_rowsums": clean["sum_rowsums"] + exp["rowsums"],
                "entries": clean["entries"] + exp["entries"], "rows_bad_sum": exp["bad_sum"],
                "rows_bad_entries": exp["bad_rows"]}
        for k, v in hand.items():
            if v is not None and rep[k] != v:
                bad.append(f"{k} {rep[k]}, stated {v}")
        got, a = rep["asymmetric_entries"], exp["asym"]
        if not sym_checked:
            if got is not None or want["asymmetric_entries"] is not None:
                bad.append(f"asymmetric_entries {got} (model {want['asymmetric_entries']}), must be None")
        elif a == "some":
            if got is None or got < 1 or got < want["asymmetric_entries"]:
                bad.append(f"asymmetric_entries {got}, must be >= 1 and >= the model's {want['asymmetric_entries']}")
        elif a != "skip":
            if got != want["asymmetric_entries"]:
                bad.append(f"asymmetric_entries {got}, model {want['asymmetric_entries']}")
            if a != "model" and got != a:
                bad.append(f"asymmetric_entries {got}, stated {a}")
        diff = np.flatnonzero(cs != want_cs)
        if len(diff):
            bad.append(f"{len(diff)} fingerprints differ from the model's, rows {diff[:5].tolist()}")
        moved = set(np.flatnonzero(cs != self.clean_cs).tolist())
        if moved != set(exp["changed"]):
            bad.append(f"fingerprints changed in rows {sorted(moved)[:8]}, stated {sorted(exp['changed'])}")
        if bad:
            self.fails.append(f"{L.name} {label}: " + "; ".join(bad))

    def run(self, label, mutate, exp):
        L = self.L
        self.ran += 1
        try:
            mutate()
            self._compare(label, exp)
        finally:
            L.restore()
        rep, cs = L.verify()
        if rep != self.clean or not np.array_equal(cs, self.clean_cs):
            self.fails.append(f"{L.name} {label}: after the words went back the report is {rep}, clean {self.clean}")

    def finish(self):
        print(f"layout {self.L.name}: {self.ran} cases, {len(self.fails)} failed")
        assert not self.fails, f"{len(self.fails)} of {self.ran} cases:\n" + "\n".join(self.fails)


def _threads():
    return max(1, min(8, os.cpu_count() or 1))


def _check_clean(L, cases, oracle):
    """The clean report: all-zero defects, equal to the model, fingerprints equal to the closed form's."""
    rep, cs = cases.clean, cases.clean_cs
    lens = np.diff(L.up)
    P = int(np.sum(lens * (lens - 1)))
    want = oracle.row_checksums(L.up, L.it, L.M, _threads())
    assert L.res.observed == P == want.pairs
    assert rep == {"sum_counts": P, "sum_rowsums": P, "entries": want.distinct, "rows_bad_sum": 0, "rows_bad_entries": 0,
                   "asymmetric_entries": 0 if L.ordered and not L.dense else None}
    model, model_cs = L.model()
    assert rep == model
    assert np.array_equal(cs, model_cs) and np.array_equal(cs, want.checksum)
    assert np.array_equal(L.nnz0.astype(np.int64), want.nnz)
    # without the symmetry pass: the same five totals, [5] not reported
    rep0, cs0 = L.verify(symmetry=False)
    assert rep0 == dict(rep, asymmetric_entries=None) and np.array_equal(cs0, cs)


def _csr_rows(L):
    """(the rows that take every position, further rows that take the positions they have)."""
    M, nnz = L.M, L.nnz0
    if L.name == "G":
        return [32_767, 32_768, 33_000], []
    if L.name == "C":
        # log A's row M - 1 is its rarest item's (29 entries): it takes the positions it has, and the last row of
        # 130 entries takes them all
        mid = M // 2 + int(np.flatnonzero(nnz[M // 2:] >= MIN_ROW)[0])
        last = int(np.flatnonzero(nnz >= MIN_ROW)[-1])
        assert 0 < mid < last < M - 1
        return [0, mid, last], [M - 1]
    return [0, M // 2, M - 1], []  # (log R puts full rows there)


def _csr_cases(L, cases):
    M = L.M
    big, small = _csr_rows(L)
    for a in big:
        assert L.nnz0[a] >= MIN_ROW, f"row {a} holds {L.nnz0[a]} entries"
    for a in small:
        assert 2 <= L.nnz0[a] < MIN_ROW
    one = 1 if L.ordered else 0
    diag_rows = [a for a in big if L.find(a, a) is not None]
    if not diag_rows:  # the highest row of every position that holds its diagonal key
        diag_rows = [int(max(a for a in np.flatnonzero(L.nnz0 >= MIN_ROW).tolist() if L.find(a, a) is not None))]
    assert diag_rows, "a diagonal entry for the diagonal cases"
    n_off = n_pairs = 0
    for a in big + small:
        n = int(L.nnz0[a])
        col, cnt = (x.copy() for x in L.row(a))
        for p in sorted({L.pos(a, p) for p in SINGLE if L.pos(a, p) < n}):
            b, v = int(col[p]), int(cnt[p])
            both = 0 if b == a else 2  # C[a, b] and C[b, a] disagree, seen from both rows (one key on the diagonal)
            n_off += b != a
            cases.run(f"row {a} cnt[{p}] += 1", lambda: L.poke_entry(a, p, cnt=v + 1),
                      _exp(counts=1, bad_sum=1, bad_rows=0, asym=both, changed=[a]))
            cases.run(f"row {a} cnt[{p}] = 0", lambda: L.poke_entry(a, p, cnt=0),
                      _exp(counts=-v, bad_sum=1, bad_rows=1, asym=both, changed=[a]))
            cases.run(f"row {a} col[{p}] = n_items", lambda: L.poke_entry(a, p, col=M),
                      _exp(bad_sum=0, bad_rows=1, asym="some", changed=[a]))
            if L.name == "C":
                cases.run(f"row {a} col[{p}] = -1", lambda: L.poke_entry(a, p, col=-1),
                          _exp(bad_sum=0, bad_rows=1, asym="some", changed=[a]))
            if b != a:
                q = L.find(b, a)
                assert q is not None, "the clean result is symmetric"
                w = int(L.row(b)[1][q])
                assert w == v

                def both_sides():
                    L.poke_entry(a, p, cnt=v + 1)
                    L.poke_entry(b, q, cnt=w + 1)
                cases.run(f"row {a} cnt[{p}] += 1 and row {b} cnt[{q}] += 1", both_sides,
                          _exp(counts=2, bad_sum=2, bad_rows=0, asym=0, changed=[a, b]))
        for p in sorted({L.pos(a, p) for p in PAIRS if 0 <= L.pos(a, p) and L.pos(a, p) + 1 < n}):
            n_pairs += 1

            def swap():
                L.poke_entry(a, p, col=int(col[p + 1]), cnt=int(cnt[p + 1]))
                L.poke_entry(a, p + 1, col=int(col[p]), cnt=int(cnt[p]))
            cases.run(f"row {a} swap entries {p}, {p + 1}", swap,
                      _exp(bad_sum=0, bad_rows=one, asym="skip", changed=[]))
            cases.run(f"row {a} col[{p + 1}] = col[{p}]", lambda: L.poke_entry(a, p + 1, col=int(col[p])),
                      _exp(bad_sum=0, bad_rows=one, asym="skip", changed=[a]))
        cases.run(f"rowsum[{a}] += 1", lambda: L.poke_rowsum(a, int(L.host["rowsum"][a]) + 1),
                  _exp(rowsums=1, bad_sum=1, bad_rows=0, asym=0, changed=[]))
        cases.run(f"row_nnz[{a}] -= 1", lambda: L.poke_nnz(a, n - 1),
                  _exp(counts=-int(cnt[n - 1]), entries=-1, bad_sum=1, bad_rows=0,
                       asym=0 if int(col[n - 1]) == a else 1, changed=[a]))
        gone = _exp(counts=-int(cnt.astype(np.int64).sum()), entries=-n, bad_sum=1, bad_rows=0, changed=[a])
        cases.run(f"row_nnz[{a}] = 0", lambda: L.poke_nnz(a, 0), gone)
        cases.run(f"row_nnz[{a}] = -1", lambda: L.poke_nnz(a, -1), dict(gone, bad_rows=1))
    assert n_off >= 6 and n_pairs >= 15
    for a in diag_rows:
        p = L.find(a, a)
        v = int(L.row(a)[1][p])
        cases.run(f"row {a} diagonal cnt[{p}] += 1", lambda: L.poke_entry(a, p, cnt=v + 1),
                  _exp(counts=1, bad_sum=1, bad_rows=0, asym=0, changed=[a]))
        cases.run(f"row {a} diagonal cnt[{p}] = 0", lambda: L.poke_entry(a, p, cnt=0),
                  _exp(counts=-v, bad_sum=1, bad_rows=1, asym=0, changed=[a]))
    # rows, not entries: two bad entries of one row count once, one in each of two rows twice
    a0, a1, a2 = big
    v0 = int(L.row(a0)[1][0])

    def two_in_one():
        L.poke_entry(a0, 0, cnt=0)
        L.poke_entry(a0, L.pos(a0, -1), col=M)
    cases.run(f"row {a0}: cnt[0] = 0 and col[n - 1] = n_items", two_in_one,
              _exp(counts=-v0, bad_sum=1, bad_rows=1, asym="some", changed=[a0]))
    for x, y in ((a0, a1), (a1, a2)):
        vx, vy = int(L.row(x)[1][64]), int(L.row(y)[1][0])

        def one_each():
            L.poke_entry(x, 64, cnt=0)
            L.poke_entry(y, 0, cnt=0)
        if int(L.row(x)[0][64]) == y and int(L.row(y)[0][0]) == x:
            continue  # (the two halves of one pair: [5] is then 2, not 4; no chosen rows do this)
        cases.run(f"rows {x}, {y}: cnt[64] = 0 and cnt[0] = 0", one_each,
                  _exp(counts=-vx - vy, bad_sum=2, bad_rows=2, changed=[x, y]))


def _dense_cases(L, cases):
    M = L.M
    d = L.host["dense"].reshape(M, M)
    classes = {"below 64": range(63, -1, -1), "64 and above": range(64, M - 1), "last": [M - 1]}
    ran = set()
    for a in (0, M // 2, M - 1):
        for cname, cols in classes.items():
            zero = next((c for c in cols if d[a, c] == 0), None)
            key = next((c for c in cols if d[a, c] != 0), None)
            if zero is not None:
                ran.add(("zero", cname))
                cases.run(f"cell ({a}, {zero}) 0 := 5", lambda: L.poke_cell(a, zero, 5),
                          _exp(counts=5, entries=1, bad_sum=1, bad_rows=1, changed=[a]))
            if key is not None:
                ran.add(("key", cname))
                v = int(d[a, key])
                cases.run(f"cell ({a}, {key}) += 1", lambda: L.poke_cell(a, key, v + 1),
                          _exp(counts=1, bad_sum=1, bad_rows=0, changed=[a]))
                cases.run(f"cell ({a}, {key}) := 0", lambda: L.poke_cell(a, key, 0),
                          _exp(counts=-v, entries=-1, bad_sum=1, bad_rows=1, changed=[a]))
        cases.run(f"row_nnz[{a}] += 1", lambda: L.poke_nnz(a, int(L.nnz0[a]) + 1),
                  _exp(bad_sum=0, bad_rows=1, changed=[]))
    # a zero cell and a key in every column class (log A's row 0 is full, its row M - 1 nearly empty)
    assert ran == {(k, c) for k in ("zero", "key") for c in classes}, ran


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_corrupted_result_one_defect_at_a_time(pkg, oracle, torch_cuda, layout):
    L = _Result(pkg, torch_cuda, layout)
    try:
        assert L.dense == (layout == "D"), "the layout under test"
        identity = np.array_equal(L.order, np.arange(L.M))
        if layout in ("R", "U"):
            assert not identity, "the large-universe planner relabelled the columns"
        else:
            assert identity
        if layout == "R":
            for a in (0, L.M // 2, L.M - 1):  # ascending in the device's order is not ascending by id
                assert np.any(np.diff(L.row(a)[0]) < 0) and np.all(np.diff(L.order[L.row(a)[0]]) > 0)
        cases = _Cases(L)
        _check_clean(L, cases, oracle)
        if L.dense:
            _dense_cases(L, cases)
        else:
            _csr_cases(L, cases)
        cases.finish()
    finally:
        L.close()


def test_interface_edges(pkg, torch_cuda):
    """No result yet: the state error.  An unknown flag through the raw entry point: COOC_ERR_ARG.  Symmetry asked of
    an any-order result: not reported.  After each the context still counts and verifies clean."""
    from flink_cooccurrence_amd import _lib

    torch = torch_cuda
    up, it, M = _log_r()
    dev = torch.device("cuda", 0)
    up_d, it_d = torch.from_numpy(up).to(dev), torch.from_numpy(it).to(dev)
    lens = np.diff(up)
    P = int(np.sum(lens * (lens - 1)))

    def counts_clean(core, symmetry):
        res = core.count_device(up_d, it_d)
        torch.cuda.synchronize()
        rep = core.verify_batch(symmetry=symmetry)
        assert res.observed == P
        assert (rep["sum_counts"], rep["sum_rowsums"], rep["entries"]) == (P, P, res.nnz)
        assert rep["rows_bad_sum"] == 0 and rep["rows_bad_entries"] == 0
        return rep

    with pkg.CooccurrenceCore(n_items=M, device=0, output="csr", planner="large", any_order=True) as core:
        with pytest.raises(pkg.IllegalStateException) as e:
            core.verify_batch()
        assert e.value.status == _lib.COOC_ERR_STATE
        assert counts_clean(core, False)["asymmetric_entries"] is None
        out = np.full(8, 77, np.int64)
        st = _lib.load().cooc_verify_batch(core._h, 2, None, out.ctypes.data_as(_lib.i64p), None)
        assert st == _lib.COOC_ERR_ARG and np.all(out == 77)
        assert counts_clean(core, False)["asymmetric_entries"] is None
        assert core.verify_batch(symmetry=True)["asymmetric_entries"] is None
        assert counts_clean(core, True)["asymmetric_entries"] is None
    with pkg.CooccurrenceCore(n_items=M, device=0, output="csr", planner="large") as core:
        with pytest.raises(pkg.IllegalStateException):
            core.verify_batch(symmetry=True)
        assert counts_clean(core, True)["asymmetric_entries"] == 0
