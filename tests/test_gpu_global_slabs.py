"""The sparse global rows of the streaming state (n_items >= 40,320), branch by branch: the slab merge
(launch_gs_merge: k_gs_flags, k_gs_alloc, k_gs_move_all, k_gs_insert, k_gs_commit) and the arena compaction
(compact_global / k_gs_compact) of cooc_stream.hip.

Every log is dictated, not drawn: windows of two-item users (so a row's columns are exactly the partners named),
a few returning users (the old / new position path of the window count), at n_items = 40,320, the smallest
universe with slabs; cases A and D repeat at 1,000,000 with the same ids spread over the whole range.  Each log
is built so that the branch its case names is certain.  That certainty is asserted twice: on any machine from a
CPU model of the arena (_SlabModel, read off launch_gs_merge / compact_global and fed with the oracle's delta
rows; test_logs_reach_their_branches), and on the GPU from cooc_global_slab_stats, which must equal the model's
(cap, bump, live, compactions) after every window of every case.

Two references, agreeing on the CPU before the GPU is consulted (_reference): oracle.OracleStream record by
record, and oracle.closed_form (A^T A - diag(colsum A)) over all records up to each window.  After every window
the GPU's delta rows, row sums, observed and top-k equal the oracle's (top-k values and scores with ==: the
device's log is the oracle's), the global row sums (exact and int32 view) and global_observed equal
it, and every global row equals it: all rows' ids, columns and exact counts in bulk through the snapshot blob,
and global_row (columns, counts, and the cnt16 view that call derives on the host) for the rows the window
touched and a stride over the others; after the last window global_row for every row.

  A  chunk boundaries: a hub row of L = 2,047 / 2,048 / 2,049 / 4,096 / 4,097 columns moves (kGsChunk = 2,048
     per block) with new columns before, after and on both sides of each boundary, and repeated old partners;
     then a window that leaves it in place.
  B  3,000 one-chunk rows move in one window: more chunks than k_gs_move_all's 2,048 blocks (the stride loop).
  C  windows in which every touched row is in place: bump and live unchanged, counts grown.
  D  one window with moved, in-place, created and untouched rows, rows 0 and M-1 touched (existing, or created
     from length 0), column M-1, 400 untouched rows between two touched ones.
  E  a window without pairs, a window of one user repeating one item, ordinary windows around them.
  F  a 3,000-column row that gains a column per window: four compactions after the first; 300 bystander rows
     identical at the end.
  G  counts of 90,000 in one window and in-place adds across 32,768 and 65,536 (the cnt16 view wraps).
  H  F's state restored from a blob taken at a compacting window, then moving and in-place windows.
"""
import functools

import numpy as np
import pytest

from tests._helpers import assert_windows_equal
from tests.test_gpu_snapshot import ROW_CNTS, ROW_COLS, ROW_IDS, ROW_PTR, ROW_SUMS, _sections

_M0 = 40_320
_BIG = 1_000_000
_TOPK = 10
_CHUNK = 2048   # kGsChunk
_GRID = 2048    # k_gs_move_all's blocks


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


# ---- the CPU model of the arena ---------------------------------------------------------------------------------

class _SlabModel:
    """(cap, bump, live, compactions) as launch_gs_merge / compact_global keep them.  Before a window of nnz delta
    entries: if bump + live + nnz > cap, compact (cap = max(2 (2 live + nnz), 4096), bump = live).  Every touched
    row with new columns takes a new slab of old length + new columns behind bump; live grows by the new columns.
    A restore leaves cap = max(2 live, 4096), bump = live and no compaction counted (cooc_snapshot_restore.hip)."""

    def __init__(self, M):
        self.M = M
        self.len = np.zeros(M, np.int64)
        self.keys = np.zeros(0, np.int64)  # row * M + col of every global entry, ascending
        self.cap = self.bump = self.live = self.compactions = 0

    def stats(self):
        return self.cap, self.bump, self.live, self.compactions

    def restore(self):
        self.cap = max(2 * self.live, 4096)
        self.bump = self.live
        self.compactions = 0

    def window(self, w):
        """One window's delta rows (an oracle.WindowOutput) -> what the merge does with them."""
        rows = w.rows.astype(np.int64)
        ridx = np.repeat(np.arange(len(rows)), np.diff(w.row_ptr))
        keys = rows[ridx] * self.M + w.cols
        nnz = len(keys)
        new = ~np.isin(keys, self.keys)
        added = np.bincount(ridx[new], minlength=len(rows)).astype(np.int64)
        old = self.len[rows]
        compacted = self.bump + self.live + nnz > self.cap
        if compacted:
            self.cap = max(2 * (2 * self.live + nnz), 4096)
            self.bump = self.live
            self.compactions += 1
        moved = added > 0
        self.bump += int((old[moved] + added[moved]).sum())
        self.live += int(added.sum())
        self.len[rows] += added
        self.keys = np.union1d(self.keys, keys[new])
        return dict(nnz=nnz, compacted=bool(compacted), rows=rows, old=old, added=added, new=new, ridx=ridx,
                    chunks=int(((old[moved] + _CHUNK - 1) // _CHUNK).sum()), stats=self.stats())


# ---- the logs: a list of windows, each a list of (user id, items) ---------------------------------------------

def _ids(M):
    """Ids of the 40,320 universe spread over [0, M): the lower half from 0 up, the upper half from M - 1 down."""
    s = (M - 1) // (_M0 - 1)
    return lambda x: x * s if x <= _M0 // 2 else M - 1 - (_M0 - 1 - x) * s


class _Users:
    def __init__(self):
        self.next = 1

    def new(self, items):
        self.next += 1
        return self.next - 1, list(items)


_HUB = 30_001


def _partner(i):
    return 12 + 4 * i


def _log_a(L, M):
    I, U = _ids(M), _Users()
    h = I(_HUB)
    x = [I(_partner(i)) for i in range(L)]
    w1 = [U.new([h, p]) for p in x]
    spaced = list(range(5, L, max(1, L // 20)))
    new = {I(3), I(_partner(0) - 1), I(_partner(L - 1) + 1), I(_partner(L - 1) + 3), M - 1}
    for b in (_CHUNK, 2 * _CHUNK):
        new |= {I(_partner(j) + 1) for j in (b - 2, b - 1, b) if 0 <= j < L}
    new |= {I(_partner(j) + 2) for j in spaced}
    rep = {0, L - 1} | {j for b in (_CHUNK, 2 * _CHUNK) for j in (b - 1, b) if j < L} | set(spaced)
    w2 = [U.new([h, n]) for n in sorted(new)] + [U.new([h, x[j]]) for j in sorted(rep)]
    w2 += [U.new([h, x[0]]), U.new([h, x[L - 1]])]
    w2 += [(w1[0][0], [I(20_011)]), (w1[1][0], [x[2]])]  # returning users: a new item, another partner
    w3 = [U.new([h, x[j]]) for j in sorted(rep)] + [U.new([h, I(_partner(0) - 1)])]
    return [w1, w2, w3]


_B_ROWS = 3000


def _log_b(M):
    I, U = _ids(M), _Users()
    w1 = [U.new([I(3 * i), I(3 * i + 1)]) for i in range(_B_ROWS)]
    w2 = [U.new([I(3 * i), I(3 * i + 2)]) for i in range(_B_ROWS)]
    w2 += [(w1[i][0], [I(39_000 + i)]) for i in range(5)]
    w3 = [U.new([I(3 * i), I(3 * i + 2)]) for i in range(0, _B_ROWS, 7)]
    return [w1, w2, w3]


def _log_c(M):
    I, U = _ids(M), _Users()
    lists = [[I(14 * i), I(14 * i + 1)] for i in range(200)] + [[I(x) for x in range(25_000, 25_030)], [0, M - 1]]
    w1 = [U.new(l) for l in lists]
    w2 = [U.new(l) for l in lists]
    w3 = [U.new(l) for l in lists[::3]] + [U.new([0, M - 1])]
    return [w1, w2, w3]


def _log_d(edge_rows_new, M):
    I, U = _ids(M), _Users()
    w1 = [] if edge_rows_new else [U.new([0, I(5)]), U.new([M - 1, I(40_317)])]
    w1 += [U.new([I(1000), I(1001)]), U.new([I(1002), I(1003)]), U.new([I(x) for x in range(2000, 2041)])]
    w1 += [U.new([I(5000 + 2 * k), I(5001 + 2 * k)]) for k in range(200)]
    back = U.new([I(30_000), I(30_001)])
    w1.append(back)
    w2 = [U.new([0, M - 1]), U.new([I(1000), I(1001)]), U.new([I(1002), I(1004)]), U.new([I(2000), I(2005)]),
          U.new([I(2000), I(1)]), U.new([I(2000), I(2001)]), U.new([I(2000), I(2040)]), U.new([I(4999), I(5400)]),
          U.new([I(20_000), I(20_001)]), U.new([I(2040), I(39_999)]), (back[0], [I(30_000)])]
    w3 = [U.new([0, I(5)]), U.new([M - 1, I(40_318)]), U.new([I(1), I(2)]), U.new([I(5100), I(5101)]),
          U.new([I(5102), I(5105)]), U.new([0, M - 1])]
    return [w1, w2, w3]


def _log_e(M):
    I, U = _ids(M), _Users()
    w1 = [U.new([I(10), I(11)]), U.new([I(10), I(12)]), U.new([I(500), I(501)]), U.new([I(20), I(21), I(22)])]
    w2 = [U.new([I(10)]), U.new([I(777)]), U.new([M - 1]), U.new([0])]
    w3 = [U.new([I(900)] * 5)]
    w4 = [U.new([I(10), I(11)]), U.new([I(900), I(901)]), (w2[1][0], [I(778)])]
    w5 = [U.new([I(10)] * 3)]
    return [w1, w2, w3, w4, w5]


_F_LEN, _F_MOVING, _F_BYSTANDERS = 3000, 19, 300


def _log_f(M):
    I, U = _ids(M), _Users()
    g = I(_HUB)
    w1 = [U.new([g, I(_partner(i))]) for i in range(_F_LEN)]
    w1 += [U.new([I(35_000 + 2 * k), I(35_001 + 2 * k)]) for k in range(_F_BYSTANDERS // 2)]
    log = [w1] + [[U.new([g, I(_partner(100 * k) + 1)])] for k in range(1, _F_MOVING + 1)]
    return log + [[U.new([g, I(_partner(7))])]]


_P, _Q, _R, _S = 100, 200, 300, 400


def _log_g(M):
    I, U = _ids(M), _Users()
    p, q, r, s = I(_P), I(_Q), I(_R), I(_S)
    big = U.new([p, q] * 300)
    w1 = [big, U.new([r, s] * 180), U.new([p, I(50)])]
    w2 = [U.new([r, s] * 20)]
    w3 = [U.new([r, s] * 181)]
    w4 = [U.new([r, s] * 20), (big[0], [p])]
    return [w1, w2, w3, w4]


_LOGS = {"A": _log_a, "B": _log_b, "C": _log_c, "D": _log_d, "E": _log_e, "F": _log_f, "G": _log_g}


def _records(w, users):
    u = np.concatenate([np.full(len(it), uid, np.int32) for uid, it in users])
    it = np.concatenate([np.asarray(it, np.int32) for _, it in users])
    return u, it, np.full(len(u), 1000 * w + 500, np.int64)


# ---- the references ----------------------------------------------------------------------------------------------

def _oracle_state(oracle, ref, M):
    rows, rp, cols, exact, v16 = ref.global_rows()
    gi, gv32, gex = ref.global_rowsums()
    rs, rs32 = np.zeros(M, np.int64), np.zeros(M, np.int32)
    rs[gi], rs32[gi] = gex, gv32
    c = ref.counters()
    return dict(rows=rows, rp=rp, cols=cols, exact=exact, v16=v16, rs=rs, rs32=rs32,
                observed=(c["UserInteractionCounterObservedCooccurrences"], c["rescorer_observed"]))


def _assert_closed_form(oracle, st, users, items, M, where):
    """The oracle's global state == A^T A - diag(colsum A) over all records so far (per-user item lists)."""
    order = np.argsort(users, kind="stable")
    _, n = np.unique(users[order], return_counts=True)
    up = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    rp, cols, data, rowsums, observed = oracle.closed_form(up, items[order], M)
    lens = np.diff(rp)
    assert np.array_equal(np.flatnonzero(lens), st["rows"]), where
    assert np.array_equal(np.concatenate([[0], np.cumsum(lens[st["rows"]])]), st["rp"]), where
    assert np.array_equal(cols, st["cols"]) and np.array_equal(data, st["exact"]), where
    assert np.array_equal(oracle.to_i16(data), st["v16"]), where
    assert np.array_equal(rowsums, st["rs"]) and np.array_equal(oracle.to_i32(rowsums), st["rs32"]), where
    assert observed == st["observed"][0], where


@functools.lru_cache(maxsize=None)
def _reference(name, M, *args):
    """Per window of the log: its records, the oracle's window output, the oracle's global state after it (equal
    to the closed form), and the arena model's step.  Computed once per log."""
    from oracle import oracle

    log = _LOGS[name](*args, M)
    ref = oracle.OracleStream(1000, topk=_TOPK)
    model = _SlabModel(M)
    out, all_u, all_i = [], [], []
    for w, users in enumerate(log):
        u, it, ts = _records(w, users)
        ref.process_elements(u, it, ts)
        fired = ref.process_watermark(1000 * w + 999)
        assert len(fired) == 1 and fired[0].ts == 1000 * w + 999
        all_u.append(u)
        all_i.append(it)
        st = _oracle_state(oracle, ref, M)
        _assert_closed_form(oracle, st, np.concatenate(all_u), np.concatenate(all_i), M, f"{name} window {w}")
        out.append(dict(records=(u, it, ts), want=fired[0], state=st, step=model.window(fired[0])))
    return out


# ---- no GPU: every log has the property its case names ----------------------------------------------------------

def _row_step(step, a):
    """(old length, new columns, the row's delta columns' new flags) of row a in a model step."""
    r = int(np.flatnonzero(step["rows"] == a)[0])
    return int(step["old"][r]), int(step["added"][r]), step["new"][step["ridx"] == r]


@pytest.mark.parametrize("L,M", [(2047, _M0), (2048, _M0), (2049, _M0), (4096, _M0), (4097, _M0), (4097, _BIG)])
def test_log_a_reaches_its_branches(oracle, L, M):
    ref = _reference("A", M, L)
    h = _ids(M)(_HUB)
    old, added, new = _row_step(ref[1]["step"], h)
    assert old == L and added >= 6 and (~new).sum() >= 4  # moved, with matching deltas (add != 0) among them
    assert ref[1]["step"]["chunks"] >= -(-L // _CHUNK) + 2
    w = ref[1]["want"]
    r = int(np.flatnonzero(w.rows == h)[0])
    dc, x = w.cols[w.row_ptr[r]:w.row_ptr[r + 1]][new], [_ids(M)(_partner(i)) for i in range(L)]
    assert dc[0] < dc[1] < x[0] and x[-1] < dc[-2] < dc[-1] == M - 1  # before the first, after the last old column
    for b in (_CHUNK, 2 * _CHUNK):  # new columns right before and right after each chunk's last old column
        for j in (b - 2, b - 1, b):
            if j < L:
                assert np.any((dc > x[j]) & (dc < (x[j + 1] if j + 1 < L else M)))
    assert _row_step(ref[2]["step"], h)[:2] == (old + added, 0)  # window 3: in place
    assert ref[2]["step"]["chunks"] == 0 and not ref[2]["step"]["added"].any()
    if M == _BIG:
        assert w.cols.max() == M - 1 and np.sum(w.cols > 2 ** 19) > 10


def test_logs_reach_their_branches(oracle):
    """B moves more chunks than the grid has blocks; C adds no column; D's window has every kind of row; E's
    windows are empty and self-only; F compacts at least three more times and never touches its bystanders; G's
    cells cross 32,768 and 65,536 by in-place adds."""
    M = _M0
    I = _ids(M)
    B = _reference("B", M)
    assert B[1]["step"]["chunks"] > _GRID and B[1]["step"]["chunks"] >= _B_ROWS
    assert np.sum((B[1]["step"]["old"] == 1) & (B[1]["step"]["added"] == 1)) >= _B_ROWS
    assert B[2]["step"]["chunks"] == 0 and B[2]["step"]["nnz"] > 0

    C = _reference("C", M)
    for w in (1, 2):
        s = C[w]["step"]
        assert s["nnz"] > 0 and not s["added"].any() and s["chunks"] == 0 and not s["compacted"]
        assert s["stats"][1:3] == C[0]["step"]["stats"][1:3]
        assert s["rows"][0] == 0 and s["rows"][-1] == M - 1
    assert np.all(C[2]["state"]["exact"] > C[0]["state"]["exact"])

    for M_d, fresh in ((_M0, False), (_M0, True), (_BIG, False)):
        D = _reference("D", M_d, fresh)
        s, w = D[1]["step"], D[1]["want"]
        moved, inplace, created = (s["old"] > 0) & (s["added"] > 0), s["added"] == 0, s["old"] == 0
        assert moved.any() and inplace.any() and created.any()
        assert s["rows"][0] == 0 and s["rows"][-1] == M_d - 1 and w.cols[w.row_ptr[1] - 1] == M_d - 1
        assert (created if fresh else moved)[[0, -1]].all()
        before = D[0]["state"]["rows"]
        gap = np.flatnonzero(np.diff(s["rows"]) > 300)
        assert any(np.sum((before > s["rows"][i]) & (before < s["rows"][i + 1])) >= 300 for i in gap)
        assert len(np.setdiff1d(before, s["rows"])) >= 400  # untouched rows
        s3 = D[2]["step"]
        assert ((s3["old"] > 0) & (s3["added"] > 0)).any() and (s3["added"] == 0).any() and (s3["old"] == 0).any()

    E = _reference("E", M)
    assert E[1]["step"]["nnz"] == 0 and len(E[1]["want"].rows) == 0 and E[1]["step"]["stats"] == E[0]["step"]["stats"]
    assert E[2]["want"].rows.tolist() == [I(900)] and E[2]["want"].cols.tolist() == [I(900)]
    assert E[2]["want"].exact.tolist() == [20]
    assert E[3]["step"]["nnz"] > 0 and E[4]["want"].rows.tolist() == [I(10)]

    F = _reference("F", M)
    assert F[0]["step"]["compacted"] and F[-1]["step"]["stats"][3] - 1 >= 3
    assert not F[-1]["step"]["compacted"] and not F[-1]["step"]["added"].any()  # the last window: in place
    by = np.array([I(35_000 + k) for k in range(_F_BYSTANDERS)])
    assert all(not np.isin(by, f["step"]["rows"]).any() for f in F[1:]) and np.isin(by, F[0]["step"]["rows"]).all()
    for f in F[1:-1]:
        old, added, _ = _row_step(f["step"], I(_HUB))
        assert old >= _F_LEN > _CHUNK and added == 1
    assert all(f["step"]["stats"][2] == len(f["state"]["cols"]) for f in F)  # live = the sum of the row lengths

    G = _reference("G", M)
    p, q, r, s = I(_P), I(_Q), I(_R), I(_S)

    def cell(w, a, b):
        st = G[w]["state"]
        i = int(np.flatnonzero(st["rows"] == a)[0])
        sl = slice(st["rp"][i], st["rp"][i + 1])
        j = int(np.flatnonzero(st["cols"][sl] == b)[0])
        return int(st["exact"][sl][j]), int(st["v16"][sl][j])

    assert cell(0, p, q) == (90_000, 90_000 - 65_536) and cell(0, q, p)[0] == 90_000 and cell(0, p, p)[0] == 89_700
    assert cell(0, r, s)[0] < 32_768 <= cell(1, r, s)[0] and cell(1, r, s)[1] < 0
    assert cell(1, r, s)[0] < 65_536 <= cell(2, r, s)[0] and cell(2, s, r) == (65_561, 25)
    assert cell(2, r, r)[0] < 65_536 <= cell(3, r, r)[0] and cell(2, s, s)[0] < 65_536 <= cell(3, s, s)[0]
    assert cell(3, p, p)[0] == 89_700 + 600 and cell(3, p, q)[0] == 90_300 == cell(3, q, p)[0]
    for w in (1, 2):  # the r / s windows add in place
        assert not G[w]["step"]["added"].any()
    assert _row_step(G[3]["step"], p)[1] == 0 and _row_step(G[3]["step"], r)[1] == 0


# ---- the GPU side -----------------------------------------------------------------------------------------------

def _operator(pkg, M):
    return pkg.NonSampledUserInteractionCounterOneInputStreamOperator(1, "SECONDS", n_items=M, top_k=_TOPK)


def _assert_window_identical(got, want, where):
    assert_windows_equal(got, want)
    live = np.arange(_TOPK)[None, :] < want.topk_sizes[:, None]
    assert np.array_equal(got.topk_values[live], want.topk_values[live]), f"{where}: top-k items"
    assert np.array_equal(got.topk_scores[live], want.topk_scores[live], equal_nan=True), f"{where}: top-k scores"


def _blob_rows(blob):
    S = _sections(blob)
    return {k: np.frombuffer(blob, t, S[k][2], S[k][0])
            for k, t in ((ROW_IDS, "<i4"), (ROW_PTR, "<i8"), (ROW_COLS, "<i4"), (ROW_CNTS, "<u4"), (ROW_SUMS, "<i8"))}


def _check_rows(core, st, rows_at, where):
    """global_row of the rows st["rows"][rows_at]: columns, exact counts, cnt16."""
    for r in rows_at:
        a, sl = int(st["rows"][r]), slice(st["rp"][r], st["rp"][r + 1])
        c, n, n16 = core.global_row(a)
        assert np.array_equal(c, st["cols"][sl]), f"{where}: columns of global row {a}"
        assert np.array_equal(n.astype(np.int64), st["exact"][sl]), f"{where}: counts of global row {a}"
        assert np.array_equal(n16, st["v16"][sl]), f"{where}: cnt16 of global row {a}"


def _check_state(core, R, stats, every_row, where):
    """The arena's numbers and the whole global state after a window against the model and the oracle."""
    st = R["state"]
    assert core.global_slab_stats() == stats, f"{where}: (cap, bump, live, compactions)"
    assert stats[2] == len(st["cols"]) and stats[1] >= stats[2] and stats[0] >= stats[1]
    B = _blob_rows(core.snapshot())
    assert core.global_slab_stats() == stats  # (the snapshot reads, nothing else)
    assert np.array_equal(B[ROW_IDS], st["rows"]), f"{where}: the non-empty rows"
    assert np.array_equal(B[ROW_PTR], st["rp"]), f"{where}: row lengths"
    bad = np.flatnonzero((B[ROW_COLS] != st["cols"]) | (B[ROW_CNTS].astype(np.int64) != st["exact"]))
    assert not len(bad), (f"{where}: {len(bad)} entries differ, the first in global row "
                          f"{st['rows'][np.searchsorted(st['rp'], bad[0], 'right') - 1]}")
    assert np.array_equal(B[ROW_SUMS], st["rs"][st["rows"]])
    ex, v32 = core.global_rowsums()
    assert np.array_equal(ex, st["rs"]) and np.array_equal(v32, st["rs32"]), f"{where}: global row sums"
    assert core.global_observed() == st["observed"], f"{where}: observed"
    n = len(st["rows"])
    if every_row:
        at = range(n)
    else:
        touched = np.searchsorted(st["rows"], R["step"]["rows"])
        at = np.unique(np.concatenate([touched[::max(1, len(touched) // 600)], touched[-1:],
                                       np.arange(0, n, max(1, n // 200)), [n - 1]]).astype(np.int64)) if n else []
    _check_rows(core, st, at, where)


def _run(op, ref, w0, w1, model_stats=None, name=""):
    """Windows [w0, w1) of a log through the operator, everything checked after each."""
    for w in range(w0, w1):
        R = ref[w]
        assert op.process_elements(*R["records"]) == 0
        got = op.process_watermark(1000 * w + 999)
        assert len(got) == 1
        where = f"{name} window {w}"
        _assert_window_identical(got[0], R["want"], where)
        stats = model_stats[w] if model_stats else R["step"]["stats"]
        _check_state(op.core, R, stats, w == len(ref) - 1, where)


@pytest.mark.gpu
@pytest.mark.parametrize("L,M", [(2047, _M0), (2048, _M0), (2049, _M0), (4096, _M0), (4097, _M0), (4097, _BIG)])
def test_chunk_boundaries(pkg, oracle, torch_cuda, L, M):
    """A: the hub row's L old entries go through ceil(L / 2,048) blocks of k_gs_move_all."""
    ref = _reference("A", M, L)
    op = _operator(pkg, M)
    _run(op, ref, 0, len(ref), name=f"A L={L}")
    op.close()


@pytest.mark.gpu
def test_grid_stride(pkg, oracle, torch_cuda):
    """B: 3,000 moved one-chunk rows, every one compared (the last window compares every row)."""
    ref = _reference("B", _M0)
    op = _operator(pkg, _M0)
    _run(op, ref, 0, 2, name="B")
    st = ref[1]["state"]
    _check_rows(op.core, st, np.searchsorted(st["rows"], [_ids(_M0)(3 * i) for i in range(_B_ROWS)]), "B window 1")
    _run(op, ref, 2, 3, name="B")
    op.close()


@pytest.mark.gpu
def test_all_in_place(pkg, oracle, torch_cuda):
    """C: windows that add no column leave bump and live where they were; the counts grow."""
    ref = _reference("C", _M0)
    op = _operator(pkg, _M0)
    _run(op, ref, 0, 1, name="C")
    before, row0 = op.core.global_slab_stats(), op.core.global_row(0)
    _run(op, ref, 1, 2, name="C")
    assert op.core.global_slab_stats() == before and before[3] == 1
    assert np.array_equal(op.core.global_row(0)[0], row0[0]) and np.all(op.core.global_row(0)[1] == 2 * row0[1])
    _run(op, ref, 2, 3, name="C")
    assert op.core.global_slab_stats() == before and np.all(op.core.global_row(0)[1] > 2 * row0[1])
    op.close()


@pytest.mark.gpu
@pytest.mark.parametrize("M,edge_rows_new", [(_M0, False), (_M0, True), (_BIG, False)])
def test_mixed_window(pkg, oracle, torch_cuda, M, edge_rows_new):
    """D: moved, in-place, created and untouched rows in one window; rows 0 and M - 1 moved, or created."""
    ref = _reference("D", M, edge_rows_new)
    assert len(ref) == 3
    op = _operator(pkg, M)
    _run(op, ref, 0, 1, name="D")
    I = _ids(M)
    block = [op.core.global_row(I(a)) for a in range(5000, 5400)]  # untouched by window 2
    _run(op, ref, 1, len(ref) - 1, name="D")
    for a, old in zip(range(5000, 5400), block):
        assert all(np.array_equal(x, y) for x, y in zip(op.core.global_row(I(a)), old)), f"untouched row {I(a)}"
    _run(op, ref, len(ref) - 1, len(ref), name="D")
    op.close()


@pytest.mark.gpu
def test_empty_and_self_only_windows(pkg, oracle, torch_cuda):
    """E: a window without pairs, a window of one user repeating one item."""
    ref = _reference("E", _M0)
    op = _operator(pkg, _M0)
    _run(op, ref, 0, len(ref), name="E")
    c, n, _ = op.core.global_row(_ids(_M0)(900))
    assert c.tolist() == [_ids(_M0)(900), _ids(_M0)(901)] and n.tolist() == [20, 1]
    op.close()


@pytest.mark.gpu
def test_repeated_compaction(pkg, oracle, torch_cuda):
    """F: the getter's numbers equal the model's after every window, four compactions after the first among
    them; every row right after each; the bystander rows at the end as after window 1."""
    ref = _reference("F", _M0)
    op = _operator(pkg, _M0)
    _run(op, ref, 0, 1, name="F")
    I = _ids(_M0)
    by = [op.core.global_row(I(35_000 + k)) for k in range(_F_BYSTANDERS)]
    _run(op, ref, 1, len(ref), name="F")
    cap, bump, live, compactions = op.core.global_slab_stats()
    assert compactions == ref[-1]["step"]["stats"][3] >= 4 and live == len(ref[-1]["state"]["cols"])
    for k, old in enumerate(by):
        assert all(np.array_equal(x, y) for x, y in zip(op.core.global_row(I(35_000 + k)), old)), f"bystander {k}"
    op.close()


@pytest.mark.gpu
def test_wrapped_views(pkg, oracle, torch_cuda):
    """G: 90,000 in one window; in-place adds across 32,768 and 65,536; the four cells of (p, q) and (r, s)."""
    ref = _reference("G", _M0)
    op = _operator(pkg, _M0)
    I = _ids(_M0)
    p, q, r, s = I(_P), I(_Q), I(_R), I(_S)

    def cells(a, b):
        out = []
        for x, y in ((a, b), (b, a), (a, a), (b, b)):
            c, n, n16 = op.core.global_row(x)
            j = int(np.flatnonzero(c == y)[0])
            out.append((int(n[j]), int(n16[j])))
        return out

    _run(op, ref, 0, 1, name="G")
    assert cells(p, q) == [(90_000, 24_464), (90_000, 24_464), (89_700, 24_164), (89_700, 24_164)]
    assert cells(r, s) == [(32_400, 32_400), (32_400, 32_400), (32_220, 32_220), (32_220, 32_220)]
    _run(op, ref, 1, 2, name="G")
    assert cells(r, s) == [(32_800, -32_736), (32_800, -32_736), (32_600, 32_600), (32_600, 32_600)]
    _run(op, ref, 2, 3, name="G")
    assert cells(r, s) == [(65_561, 25), (65_561, 25), (65_180, -356), (65_180, -356)]
    _run(op, ref, 3, 4, name="G")
    assert cells(r, s) == [(65_961, 425), (65_961, 425), (65_560, 24), (65_560, 24)]
    assert cells(p, q) == [(90_300, 24_764), (90_300, 24_764), (90_300, 24_764), (89_700, 24_164)]
    op.close()


@pytest.mark.gpu
def test_restore_then_merge(pkg, oracle, torch_cuda):
    """H: a blob taken right after one of F's later compactions, restored into a fresh operator (bump = live = the
    entries, no compaction counted), then the rest of F's windows, moving ones and the in-place one: every window
    and every row against the oracle, the arena against the model restarted at the restore, and the final blob
    equal to the uninterrupted operator's."""
    ref = _reference("F", _M0)
    cut = max(w for w, f in enumerate(ref) if f["step"]["compacted"] and w + 3 < len(ref))
    assert cut > 0 and np.any(ref[cut + 1]["step"]["added"]) and not np.any(ref[-1]["step"]["added"])
    model, stats = _SlabModel(_M0), {}
    for w, f in enumerate(ref):
        model.window(f["want"])
        if w == cut:
            model.restore()
        stats[w] = model.stats()
    assert stats[cut] == (max(2 * ref[cut]["step"]["stats"][2], 4096),) + (ref[cut]["step"]["stats"][2],) * 2 + (0,)
    A = _operator(pkg, _M0)
    for w, f in enumerate(ref):
        A.process_elements(*f["records"])
        assert len(A.process_watermark(1000 * w + 999)) == 1
        if w == cut:
            assert A.core.global_slab_stats() == f["step"]["stats"]
            blob = A.snapshot()
    final = A.snapshot()
    A.close()
    B = _operator(pkg, _M0)
    B.restore(blob)
    assert B.core.global_slab_stats() == stats[cut]
    _check_state(B.core, ref[cut], stats[cut], True, "H restored")
    _run(B, ref, cut + 1, len(ref), model_stats=stats, name="H")
    assert B.core.global_slab_stats()[3] >= 1  # the restored arena compacted again
    assert B.snapshot() == final
    B.close()


@pytest.mark.gpu
def test_dense_state_has_no_slabs(pkg, torch_cuda):
    """Below 40,320 items the global rows are the dense matrix: the getter gives zeros."""
    with pkg.CooccurrenceCore(n_items=100, topk=0) as core:
        assert core.global_slab_stats() == (0, 0, 0, 0)
        core.submit_batch(999, [1], [0, 2], [3, 4])
        core.finish_window(999)
        assert core.global_slab_stats() == (0, 0, 0, 0)
    with pkg.CooccurrenceCore(n_items=_M0, topk=0) as core:
        assert core.global_slab_stats() == (0, 0, 0, 0)
        core.submit_batch(999, [1], [0, 2], [3, 4])
        core.finish_window(999)
        assert core.global_slab_stats() == (4096, 2, 2, 1)
