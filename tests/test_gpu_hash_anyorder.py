"""The any-order hash compaction of k_sp_main (sp_hash_compact, both shapes): the table is swept into registers,
the waves count their entries with ballots, and every entry is stored from its register at the wave's offset + the
ballot bits below its lane -- no scan over lanes, no staging in LDS, order (wave, register index, lane).  The self
term is taken off in the sweep by the lane that reads the row's own column.  Needs an MI355X.

Every GPU case: the any_order=True rows against rows summed directly from the lists (AtA - diag), the whole result
(host copy, every row sorted by column) entry by entry against the any_order=False run's, row_nnz equal to that
run's, and cooc_verify_batch clean on the any-order result (it reads the device rows as stored: holes, duplicates,
zero counts, wrong sums).

A release build has no handle on the chunks a row was counted in (the phase statistics exist in COOC_SP_STATS
builds only).  The logs are therefore built around a restatement of the planner (k_sp_est, est_distinct,
k_sp_plan: `_plan`), and a test that runs on any machine asserts from it, with margins, that the rows named here
are planned as the hash chunks and table sizes the cases need; the GPU cases rely on that construction.

Three logs:
  * the slot log (columns = ids, 4 tiles): every mid row of W = 9,216 pairs is planned as two hash chunks, tiles
    0-2 in a 4,096-slot table and tile 3 in a 1,024-slot table; every big row as one 8,192-slot chunk.  Its rows
    hold keys picked on the host by the table's hash, (column * 0x9E3779B1) >> (32 - lg H): every entry in the
    first wave's slots, in the last wave's, on both sides of the waves' share boundaries, a probe chain wrapping
    from slot H - 1 to slot 0; chunks of exactly one entry; a chunk that is empty after the self term; own columns
    whose count equals the self term (m = 1 in every list) and exceeds it; and a mid chunk of 2,300 entries, above
    the 2,048 the LDS staging took (the row beats its estimate: ids that occur nowhere else, distinct home slots
    in runs of 9, so no probe chain comes near the 64-probe limit).  The big shape's 4,096 cannot be reached this
    way: 4,300 more once-only ids raise every big row's estimate past one chunk's fill.
  * the mid-row log of test_gpu_mid4 (both flags): mid rows with a dense tile 0 that holds the row's own column
    beside hash chunks that do not, and big rows whose upper tiles are 8,192-slot hash chunks of ~2,200 entries.
  * the relabel log (default flags; the relabel is asserted): a hash chunk from tile 0 on whose ids are looked up
    in the hot-column map (hot partners) or shifted one tile down (partners that occur once: not hot).
"""
import numpy as np
import pytest

from tests.test_gpu_dense_stores import _count, _planned_dense, _same
from tests.test_gpu_mid4 import _BIG, _HEAD, _PROBES, _csr, _mid_log, _pair_work
from tests.test_gpu_sparse import _Brute, _check_rows, _Rows

_TW = 16384
_EST_K = 84
_FILL, _SLACK, _DENSE_PAIRS = 0.45, 4.0, 2.0 * _TW
_SHAPES = {True: dict(hmax=4096, maxtiles=32), False: dict(hmax=8192, maxtiles=64)}  # mid / big


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


# ---- the planner, restated -------------------------------------------------------------------------------------

class _Planner:
    """k_sp_est's table for a column-space frequency vector, and k_sp_plan's chunk plan of a whole row of pair work
    W: [(first tile, end tile, dense, table slots, expected keys)], with the smallest relative distance of any
    decision's quantity from its threshold (`margin`)."""

    def __init__(self, freq):
        freq = np.asarray(freq, np.float64)
        self.N = float(freq.sum())
        self.T = (len(freq) + _TW - 1) // _TW
        k = np.exp2(0.5 * np.arange(_EST_K))
        self.E = np.zeros((self.T, _EST_K))
        self.gmass = np.zeros(self.T)
        for t in range(self.T):
            f, mult = np.unique(freq[t * _TW:(t + 1) * _TW], return_counts=True)
            mult, f = mult[f > 0], f[f > 0]
            self.E[t] = (-np.expm1(-k[:, None] * f[None, :] / self.N) * mult[None, :]).sum(axis=1)
            self.gmass[t] = float((f * mult).sum()) / self.N

    def distinct(self, t, W):
        x = 2.0 * np.log2(float(W))
        k = int(x)
        if k >= _EST_K - 1:
            return self.E[t, _EST_K - 1]
        return self.E[t, k] + (x - k) * (self.E[t, k + 1] - self.E[t, k])

    def plan(self, W):
        mid = 4096 < W <= 65535
        hmax, maxtiles = _SHAPES[mid]["hmax"], _SHAPES[mid]["maxtiles"]
        hfill = _FILL * hmax
        chunks, margin = [], [1.0]

        def near(x, thr):
            margin.append(abs(x - thr) / thr)

        def close(cs, t, cur):
            H = 1024
            while H < hmax:
                near(_SLACK * cur + 64.0, H)
                if H >= _SLACK * cur + 64.0:
                    break
                H <<= 1
            chunks.append((cs, t, False, H, cur))

        cs, cur, n_in = -1, 0.0, 0
        for t in range(self.T):
            d, e = self.distinct(t, W), W * self.gmass[t]
            near(d, hfill)
            near(e, _DENSE_PAIRS)
            if d > hfill or e > _DENSE_PAIRS:
                if cs >= 0:
                    close(cs, t, cur)
                chunks.append((t, t + 1, True, 0, d))
                cs = -1
                continue
            if cs >= 0:
                near(cur + d, hfill)
            if cs < 0 or cur + d > hfill or n_in == maxtiles:
                if cs >= 0:
                    close(cs, t, cur)
                cs, cur, n_in = t, 0.0, 0
            cur += d
            n_in += 1
        if cs >= 0:
            close(cs, self.T, cur)
        return chunks, min(margin)


def _home(col, H):
    """The slot a column's probe chain starts at in an H-slot table."""
    lg = int(H).bit_length() - 1
    return ((np.asarray(col, np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - lg)


class _Picker:
    """Ids of a column range by home slot; an id is handed out once (`taken` is shared by every picker)."""

    def __init__(self, lo, hi, H, taken):
        self.ids = np.arange(lo, hi)
        self.home = _home(self.ids, H).astype(np.int64)
        self.taken = taken

    def take(self, slot, n=1):
        out = [int(x) for x in self.ids[self.home == slot] if int(x) not in self.taken][:n]
        assert len(out) == n, f"no unused id with home slot {slot}"
        self.taken.update(out)
        return out


# ---- the slot log ---------------------------------------------------------------------------------------------
_M = 4 * _TW
_F, _NA, _N3 = 40, 1293, 195  # background: _F lists of _NA ids of tiles 0-2 and _N3 of tile 3
_PRIV = 2300                  # the once-only ids of the row above the old staging limit


def _wave_slots(H, threads, wave):
    """The slots whose entries wave `wave` holds: thread tid takes slots 4 (tid + q threads) .. + 3."""
    s = np.arange(H)
    return s[((s // 4) % threads) // 64 == wave]


def _slot_log():
    """Returns (up, it, M, cases): cases[name] = dict(row=, H=, threads=, chunk=(lo, hi) columns of the chunk under
    test, slots= the slots its entries must occupy or None)."""
    rng = np.random.default_rng(77)
    taken = set()
    per = _NA // 3
    bg = np.concatenate([t * _TW + rng.choice(_TW, per, replace=False) for t in range(3)] +
                        [3 * _TW + rng.choice(_TW, _N3, replace=False)])
    taken.update(bg.tolist())
    lists = [rng.permutation(bg) for _ in range(_F)]
    pa, pb, pbig = (_Picker(0, 3 * _TW, 4096, taken), _Picker(3 * _TW, _M, 1024, taken),
                    _Picker(0, _M, 8192, taken))
    cases = {}

    def fresh(lo, hi):
        while True:
            x = int(rng.integers(lo, hi))
            if x not in taken:
                taken.add(x)
                return x

    def mid_row(name, a, keys, H, chunk, slots):
        # [a] x 64 + the keys, cycled to 80 positions: 144 long, W = 9,216 pairs
        taken.update([a] + list(keys))
        body = np.resize(np.asarray(keys, np.int64), 80)
        lists.append(rng.permutation(np.concatenate([np.full(64, a), body])))
        cases[name] = dict(row=a, H=H, threads=256, chunk=chunk, slots=slots)

    A, B = (0, 3 * _TW), (3 * _TW, _M)
    # 1,024-slot chunk (tile 3); the row's own column lies in tiles 0-2: that chunk holds the own column alone
    w0, w3 = _wave_slots(1024, 256, 0), _wave_slots(1024, 256, 3)
    s = w0[[0, 1, 2, 3, 100, 101, 254, 255]]
    mid_row("mid1k_first_wave", fresh(*A), sum((pb.take(x) for x in s), []), 1024, B, s)
    s = w3[[0, 1, 2, 3, 100, 101, 254, 255]]
    mid_row("mid1k_last_wave", fresh(*A), sum((pb.take(x) for x in s), []), 1024, B, s)
    s = np.array([255, 256, 511, 512, 767, 768])
    mid_row("mid1k_boundaries", fresh(*A), sum((pb.take(x) for x in s), []), 1024, B, s)
    mid_row("mid1k_wrap", fresh(*A), pb.take(1023, 3) + pb.take(1021), 1024, B, np.array([1021, 1023, 0, 1]))
    mid_row("mid1k_one_entry", fresh(*A), pb.take(517), 1024, B, np.array([517]))
    # 4,096-slot chunk (tiles 0-2); the own column in tile 3 (a one-entry chunk of its own)
    w0, w3 = _wave_slots(4096, 256, 0), _wave_slots(4096, 256, 3)
    s = w0[[0, 1, 255, 256, 257, 511, 512, 767, 768, 1023]]
    mid_row("mid4k_first_wave", fresh(*B), sum((pa.take(x) for x in s), []), 4096, A, s)
    s = w3[[0, 1, 255, 256, 257, 511, 512, 767, 768, 1023]]
    mid_row("mid4k_last_wave", fresh(*B), sum((pa.take(x) for x in s), []), 4096, A, s)
    s = np.array([255, 256, 1023, 1024, 3071, 3072])
    mid_row("mid4k_boundaries", fresh(*B), sum((pa.take(x) for x in s), []), 4096, A, s)
    mid_row("mid4k_wrap", fresh(*B), pa.take(4095, 3) + pa.take(4093), 4096, A, np.array([4093, 4095, 0, 1]))
    # m = 1 in every list: 64 lists [a] + 143 keys of tiles 0-2, a in tile 3 -- a's tile-3 chunk is empty after the
    # self term, and every key's row loses its own column (count 64 = self) from a chunk of 143 other entries
    a, keys = fresh(*B), [fresh(*A) for _ in range(143)]
    for _ in range(64):
        lists.append(rng.permutation(np.array([a] + keys)))
    cases["mid_self_vanishes"] = dict(row=a, H=1024, threads=256, chunk=B, slots=np.zeros(0, np.int64), keys=keys)
    # above the old staging limit: [x] x 4 + 2,300 once-only ids of tiles 0-2, home slots s with s % 16 < 9
    x = fresh(*B)
    want = [sl for sl in range(4096) if sl % 16 < 9][:_PRIV]
    priv = sum((pa.take(sl) for sl in want), [])
    taken.update(priv)
    lists.append(rng.permutation(np.concatenate([np.full(4, x), priv])))
    cases["mid_above_staging"] = dict(row=x, H=4096, threads=256, chunk=A, slots=np.array(want))
    # big rows ([b] x 256 + keys cycled to 44 positions: 300 long, W = 76,800): one 8,192-slot chunk over every tile,
    # the own column in it -- b is picked by its home slot as well
    def big_row(name, slots):
        ids = sum((pbig.take(sl) for sl in slots), [])
        b, keys = ids[0], ids[1:]
        taken.update(ids)
        lists.append(rng.permutation(np.concatenate([np.full(256, b), np.resize(np.asarray(keys, np.int64), 44)])))
        cases[name] = dict(row=b, H=8192, threads=512, chunk=(0, _M), slots=np.asarray(slots))

    w0, w7 = _wave_slots(8192, 512, 0), _wave_slots(8192, 512, 7)
    big_row("big_first_wave", w0[[0, 1, 255, 256, 257, 511, 512, 767, 768, 1023]])
    big_row("big_last_wave", w7[[0, 1, 255, 256, 257, 511, 512, 767, 768, 1023]])
    big_row("big_boundaries", [255, 256, 2047, 2048, 6143, 6144])
    ids = pbig.take(8191, 3) + pbig.take(8189)
    taken.update(ids)
    lists.append(rng.permutation(np.concatenate([np.full(256, ids[0]), np.resize(np.asarray(ids[1:], np.int64), 44)])))
    cases["big_wrap"] = dict(row=ids[0], H=8192, threads=512, chunk=(0, _M), slots=np.array([8189, 8191, 0, 1]))
    up, it = _csr(lists)
    return up, it, _M, cases


_SLOT = {}


def _slot():
    if not _SLOT:
        up, it, M, cases = _slot_log()
        _SLOT.update(up=up, it=it, M=M, cases=cases, brute=_Brute(up, it, M))
    return _SLOT


def _table_slots(cols, H):
    """The slots a linear-probing table of H slots holds after the columns were inserted (any order: the set of
    occupied slots does not depend on it), and the longest run of occupied slots (a probe chain's bound)."""
    occ = np.zeros(H, bool)
    for h in _home(cols, H).astype(np.int64):
        while occ[h]:
            h = (h + 1) & (H - 1)
        occ[h] = True
    run = best = 0
    for o in np.concatenate([occ, occ]):
        run = run + 1 if o else 0
        best = max(best, run)
    return np.flatnonzero(occ), min(best, H)


def test_slot_log_is_planned_as_built():
    """No GPU: the restated planner gives every mid case row of the slot log two hash chunks (tiles 0-2: 4,096
    slots; tile 3: 1,024) and every big one a single 8,192-slot chunk, each decision at least 4% from its
    threshold; and the rows' entries occupy the table slots the cases name."""
    L = _slot()
    up, it, M, cases, brute = L["up"], L["it"], L["M"], L["cases"], L["brute"]
    W = _pair_work(up, it, M)
    P = _Planner(np.bincount(it, minlength=M))
    for name, c in cases.items():
        a = c["row"]
        chunks, margin = P.plan(int(W[a]))
        shape = [(t0, t1, dense, H) for t0, t1, dense, H, _ in chunks]
        if c["threads"] == 256:
            assert W[a] == 9216, name
            assert shape == [(0, 3, False, 4096), (3, 4, False, 1024)], f"{name}: {chunks}"
        else:
            assert W[a] == 76800, name
            assert shape == [(0, 4, False, 8192)], f"{name}: {chunks}"
        assert margin >= 0.04, f"{name}: a planner decision is {margin:.3f} from its threshold"
        cols, cnt = brute.row(a)
        lo, hi = c["chunk"]
        inside = cols[(cols >= lo) & (cols < hi)]
        slots, run = _table_slots(inside, c["H"])
        assert np.array_equal(slots, np.sort(c["slots"])), name
        assert run < 32, name
        if c["threads"] == 256:  # the other chunk: the own column alone (count above self); or the 143 keys
            rest = cols[(cols < lo) | (cols >= hi)]
            assert rest.tolist() == (sorted(c["keys"]) if name == "mid_self_vanishes" else [a]), name
    c = cases["mid_self_vanishes"]
    assert len(brute.row(c["row"])[0]) == 143 and c["row"] not in brute.row(c["row"])[0]
    k = c["keys"][0]
    assert W[k] == 9216 and k not in brute.row(k)[0] and len(brute.row(k)[0]) == 143
    assert len(brute.row(cases["mid_above_staging"]["row"])[0]) == _PRIV + 1 and _PRIV > 2048
    assert len(brute.row(cases["mid1k_one_entry"]["row"])[0]) == 2


def _run_both_orders(pkg, torch, up, it, M, brute, sample, want_relabel, **kw):
    """any_order False then True with the flags kw: every check of the module docstring."""
    first = nnz = None
    for any_order in (False, True):
        where = f"{kw} any_order={any_order}"
        core, res = _count(pkg, torch, up, it, M, any_order=any_order, **kw)
        with core:
            lens = np.diff(up)
            assert res.observed == int(np.sum(lens * (lens - 1))), where
            relabelled = not np.array_equal(core.column_order(), np.arange(M))
            assert relabelled == want_relabel, where
            rows = _Rows(res, M)
            assert int(rows.nnz.sum()) == res.nnz, where
            chk = core.verify_batch()
            assert chk["rows_bad_sum"] == 0 and chk["rows_bad_entries"] == 0, where
            assert chk["sum_counts"] == chk["sum_rowsums"] == res.observed, where
            _check_rows(rows, brute, sample)
            got = core.copy_batch(res.nnz, res.observed)
        if first is None:
            first, nnz = got, rows.nnz.copy()
        else:
            _same(got, first, where)
            assert np.array_equal(rows.nnz, nnz), where
    return first


@pytest.mark.gpu
@pytest.mark.parametrize("column_order", [True, False])
def test_slot_log_vs_brute(pkg, torch_cuda, column_order):
    """column_order=True: columns are ids, the chunks and slots are the ones test_slot_log_is_planned_as_built
    asserts.  Default flags: the log's ids lie in every tile, so they are relabelled (asserted); the ~4,000 ids
    that occur all become hot, and the same rows run through the dense tile 0 instead."""
    L = _slot()
    cases = L["cases"]
    rng = np.random.default_rng(5)
    sample = [c["row"] for c in cases.values()] + cases["mid_self_vanishes"]["keys"][:3]
    sample += rng.choice(np.unique(L["it"]), 8, replace=False).tolist()
    _run_both_orders(pkg, torch_cuda, L["up"], L["it"], L["M"], L["brute"], sample, not column_order,
                     column_order=column_order)


# ---- both shapes beside dense tiles: the mid-row log ------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("column_order", [True, False])
def test_mid_log_hash_chunks_vs_brute(pkg, torch_cuda, column_order):
    """Head rows (mid; tile 0 dense and holding the row's own column -- asserted from the planner's rule -- the tail
    tiles in hash chunks that hold none of it), probe rows with the own column in a tail hash chunk (m = 1: it
    vanishes), big rows with 8,192-slot hash chunks above a dense tile 0 (asserted from the restated plan for
    columns = ids)."""
    up, it, M = _mid_log()
    brute = _Brute(up, it, M)
    W = _pair_work(up, it, M)
    heads = _HEAD[np.argsort(-W[_HEAD], kind="stable")[:3]]
    for a in heads:
        assert 4096 < W[a] <= 65535 and _planned_dense(up, it, M, int(a), 0, True)
    P = _Planner(np.bincount(it, minlength=M))
    for a in list(heads) + [int(_BIG[0]), 200_003]:
        chunks, _ = P.plan(int(W[a]))
        hashed = [c for c in chunks if not c[2]]
        assert chunks[0][2] and len(hashed) >= 2, f"row {a}: {chunks}"
        if W[a] > 65535:
            assert all(c[3] == 8192 for c in hashed), f"row {a}: {chunks}"
    assert W[_BIG[0]] > 65535 and 200_003 not in brute.row(200_003)[0]
    sample = np.concatenate([heads, list(_PROBES), _BIG[:2]])
    _run_both_orders(pkg, torch_cuda, up, it, M, brute, sample, not column_order, column_order=column_order)


# ---- a hash chunk from tile 0 on behind the relabel --------------------------------------------------------------
_MR = 300_000
_RA, _RB = 123_457, 40_001  # a mid row and a big row of the relabel log


def _relabel_log():
    """200,000 lists of two of the ten ids 8192..8201 (the mass: N ~ 4.5e5, so an id that occurs once or twice
    adds ~0.02 expected keys to a mid row's estimate); 16,600 filler ids twice each, in lists of 50 (more than
    the 16,384 hot columns occur at least twice: an id that occurs ONCE is not hot); row _RA: 64 lists of [_RA],
    100 keys that occur in all 64 lists (hot: looked up in the map) and one id of its own (not hot: its column
    is its id one tile up), W = 6,528; row _RB: one list of [_RB] x 256, 30 of those keys and 14 once-only ids,
    W = 76,800."""
    rng = np.random.default_rng(88)
    bulk = rng.integers(8192, 8202, (200_000, 2))
    pool = rng.permutation(np.setdiff1d(np.arange(20_000, _MR), [_RA, _RB]))
    fill, keys, once = pool[:16_600], pool[16_600:16_700], pool[16_700:16_700 + 64 + 14]
    lists = [row for row in bulk]
    lists += [x for x in rng.permutation(np.concatenate([fill, fill])).reshape(-1, 50)]
    for i in range(64):
        lists.append(rng.permutation(np.concatenate([[_RA], keys, once[i:i + 1]])))
    lists.append(rng.permutation(np.concatenate([np.full(256, _RB), keys[:30], once[64:]])))
    up, it = _csr(lists)
    return up, it, _MR, keys, once


def test_relabel_log_is_planned_as_built():
    """No GPU: in relabelled column space tile 0 holds the 16,384 most frequent ids, whichever of the twice-only
    fillers those are -- the multiset of its frequencies is what the estimate sees.  Row _RA's estimate over every
    tile stays below a mid hash chunk's fill with tile 0 far from dense: one hash chunk from tile 0 on."""
    up, it, M, keys, once = _relabel_log()
    f = np.bincount(it, minlength=M)
    W = _pair_work(up, it, M)
    assert W[_RA] == 64 * 102 and W[_RB] == 256 * 300
    assert np.count_nonzero(f >= 2) > _TW and np.all(f[once] == 1) and np.all(f[keys] >= 64)
    assert np.count_nonzero(f[:_TW] > 0) < _TW - _TW // 16  # (the hot ids are not already in tile 0: relabelled)
    hot = np.sort(f)[::-1][:_TW]
    rest = np.sort(f)[::-1][_TW:]
    cols = np.concatenate([hot, rest])  # tile 0, then every other id in some order: the totals do not depend on it
    P = _Planner(cols)
    d0 = P.distinct(0, int(W[_RA]))
    total = sum(P.distinct(t, int(W[_RA])) for t in range(P.T))
    assert d0 < 0.75 * _FILL * 4096 and total < 0.75 * _FILL * 4096, (d0, total)
    assert W[_RA] * P.gmass[0] < 0.75 * _DENSE_PAIRS


@pytest.mark.gpu
def test_relabel_log_mapped_hash_chunk_vs_brute(pkg, torch_cuda):
    """Default flags (relabelled: asserted).  Row _RA: 100 hot partners and 64 that are not, the own column
    vanishing (m = 1); row _RB: both kinds beside its own column (count 256 x 255)."""
    up, it, M, keys, once = _relabel_log()
    brute = _Brute(up, it, M)
    c, _ = brute.row(_RA)
    assert len(c) == 164 and _RA not in c
    c, _ = brute.row(_RB)
    assert len(c) == 45 and _RB in c
    sample = [_RA, _RB, 8192, 8201] + keys[:3].tolist() + once[:2].tolist() + once[-2:].tolist()
    _run_both_orders(pkg, torch_cuda, up, it, M, brute, sample, True)
