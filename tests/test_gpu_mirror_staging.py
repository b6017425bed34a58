"""The mirrored split rows' cells in per-source-row records (SpArgs.mrec: the record of the source row of column
rank rb >= 16,384 holds C[rb, split_row[slot]] at cell `slot`, n_split cells padded to 16) and the transposing
finalize (k_sp_tail_pass around k_sp_split_finalize: tiles of 64 source rows).  Every log is counted mirrored, in
both emission orders, and checked against rows summed directly from the lists; the whole host copy is compared
(by digest) with the same count under COOC_SP_MIRROR=0, which one child process makes for every log (the knob is
read when a core is created).  The GPU cases need an MI355X; the log properties are asserted without one.

The logs (_staging_log): U lists of L ids each (a row's pair work is L x its frequency, so a row splits above
2^23 / L lists).  A list holds every split id with probability 0.95 (else a uniform head id), n_head ids uniform over
the other ids below 8,192, and n_tail tail ids log-uniform over [16384, M), the hottest below the split
threshold and, where the log is large enough, in more than 65,535 lists (a mirrored cell above 65,535 from a big
source row).  Ids are kept (column_order=True: rank = id), so the tail ids are the mirror sources: big, mid --
light ones, whose tile 0 is part of a hash chunk, and heavy ones, whose tile 0 is dense -- small and tiny.  Planted:
id M - 1 in every 1,000th list (the last record), a block of 128 tail ids that occur nowhere (a whole tile of
untouched records), and the id `zero` in two lists that hold no split id and nowhere else (a source whose cells are
all zero).

Cases: n_split = 1 (a 16-cell record, 15 pads), 17 (two 64-B lines), 70 (more slots than lanes in a wave); split
rows at the ranks 0..3 and 300 (mslot holes below mirror_hi); tests/test_gpu_mirror.py's base log with the relabel
on; and universes of 16,384 + {1, 127, 128, 129} items through planner="large" (a single tail record; the last
tile one row short, full, and one row over).
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_mirror import _classes, _mirror_log, _sample
from tests.test_gpu_sparse import _Brute, _check_rows, _Rows

_TW = 16384  # k_sp_main's tile width
_B = 64      # the transposing finalize's tile (source rows)
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _staging_log(split_ids, L, U, M, n_tail, tail_p=1.0, gap=None, zero=None, seed=71):
    rng = np.random.default_rng(seed)
    split_ids = np.asarray(split_ids, np.int32)
    ns, n_head = len(split_ids), L - len(split_ids) - n_tail
    assert n_head >= 0
    free = np.setdiff1d(np.arange(8192, dtype=np.int32), split_ids)
    A = np.empty((U, L), np.int32)
    S = np.broadcast_to(split_ids, (U, ns)).copy()
    absent = rng.random((U, ns)) >= 0.95
    S[absent] = rng.choice(free, int(absent.sum()))
    A[:, :ns] = S
    A[:, ns:ns + n_head] = rng.choice(free, (U, n_head))
    span = M - _TW
    x = 2.0 * np.exp(rng.random((U, n_tail)) * np.log((span + 1) / 2.0))  # in [2, span + 1)
    t = _TW + np.minimum(x.astype(np.int64) - 2, span - 1)
    if gap is not None:
        t[(t >= gap[0]) & (t < gap[1])] += gap[1] - gap[0]
    if zero is not None:
        t[t == zero] -= 1
    thin = rng.random((U, n_tail)) >= tail_p
    t[thin] = rng.choice(free, int(thin.sum()))
    A[:, ns + n_head:] = t
    A[::1000, L - 1] = M - 1
    if zero is not None:
        clean = np.array([7, U // 2 + 7])
        A[clean, :ns] = rng.choice(free, (2, ns))
        A[clean, L - 2] = zero
    A = rng.permuted(A, axis=1)
    return np.arange(U + 1, dtype=np.int64) * L, np.ascontiguousarray(A.reshape(-1)), M


# name -> (builder arguments, core arguments, L, the split ids, checks of the CPU test)
_M1 = 200_000
_GAP = (_TW + 10 * _B, _TW + 12 * _B)
_CASES = {
    "ns1": (dict(split_ids=[0], L=30, U=320_000, M=_M1, n_tail=20, gap=_GAP, zero=_M1 - 2), dict(column_order=True)),
    "ns17": (dict(split_ids=list(range(17)), L=40, U=240_000, M=120_000, n_tail=15, gap=_GAP, zero=120_000 - 2),
             dict(column_order=True)),
    "ns70": (dict(split_ids=list(range(70)), L=90, U=100_000, M=100_000, n_tail=14, gap=_GAP, zero=100_000 - 2),
             dict(column_order=True)),
    "gaps": (dict(split_ids=[0, 1, 2, 3, 300], L=30, U=320_000, M=_M1, n_tail=20, gap=_GAP, zero=_M1 - 2),
             dict(column_order=True)),
    "base_relabelled": (None, dict()),
    "m_one": (dict(split_ids=[0], L=30, U=320_000, M=_TW + 1, n_tail=1, tail_p=0.25),
              dict(column_order=True, planner="large")),
    "m_bk_minus": (dict(split_ids=[0], L=30, U=320_000, M=_TW + 2 * _B - 1, n_tail=4, tail_p=0.5),
                   dict(column_order=True, planner="large")),
    "m_bk": (dict(split_ids=[0], L=30, U=320_000, M=_TW + 2 * _B, n_tail=4, tail_p=0.5),
             dict(column_order=True, planner="large")),
    "m_bk_plus": (dict(split_ids=[0], L=30, U=320_000, M=_TW + 2 * _B + 1, n_tail=4, tail_p=0.5),
                  dict(column_order=True, planner="large")),
}
_FULL = ("ns1", "ns17", "ns70", "gaps")  # the logs with sources of every class
# ... whose hottest tail id (a big row: 100,000 lists of 90 ids cannot hold it often enough below the split
# threshold) shares more than 65,535 lists with the first split id
_BIG_CELL = ("ns1", "ns17", "gaps")

_LOGS = {}


def _build(name):
    args, _ = _CASES[name]
    return _mirror_log("base") if args is None else _staging_log(**args)


def _log(name):
    """The case's log, its brute-force reference and the reference rows computed so far (shared by both orders)."""
    if name not in _LOGS:
        up, it, M = _build(name)
        _LOGS[name] = (up, it, M, _CachedBrute(up, it, M))
    return _LOGS[name]


class _CachedBrute:
    def __init__(self, up, it, M):
        self.brute, self.rows = _Brute(up, it, M), {}

    def row(self, a):
        if a not in self.rows:
            self.rows[a] = self.brute.row(a)
        return self.rows[a]


def _pair_work(up, it, M):
    L = int(up[1] - up[0])
    return L * np.bincount(it, minlength=M).astype(np.int64), L


def _digest(got):
    h = hashlib.sha256()
    for x in (got.row_ptr, got.cols, got.cnt, got.rowsum):
        h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()


def test_logs_split_the_intended_rows_and_hold_every_source_class():
    """From pair work alone: the intended rows split (and no other), every split row below rank 16,384, tail ids
    in every class of the four large logs (mid rows at both ends of the class: light and heavy tile 0), the
    planted empty tile, the all-zero source, the last id, and a big tail row in more than 65,535 lists with the
    split item."""
    for name, (args, _) in _CASES.items():
        up, it, M = _build(name)
        W, L = _pair_work(up, it, M)
        assert (len(it) // L) * L * (L - 1) <= 10 ** 9
        cls = {"split": W > 2 ** 23, "big": (W > 65535) & (W <= 2 ** 23), "mid": (W > 4096) & (W <= 65535),
               "small": (W > 256) & (W <= 4096), "tiny": (W > 0) & (W <= 256)}
        want = [0, 1, 2, 3, _TW] if args is None else args["split_ids"]
        assert np.array_equal(np.flatnonzero(cls["split"]), np.sort(want)), name
        assert W[M - 1] > 0, name
        if args is None:
            continue
        assert not cls["split"][_TW:].any()
        assert cls["big"][_TW:].any(), name
        if name in _FULL:
            for k in ("big", "mid", "small", "tiny"):
                assert cls[k][_TW:].sum() >= 5, (name, k)
            tail_mid = W[_TW:][cls["mid"][_TW:]]
            assert (tail_mid < 6000).any() and (tail_mid > 45000).any(), name
            assert not W[_GAP[0]:_GAP[1]].any() and W[_GAP[0] - 1] > 0 and W[_GAP[1]] > 0
            # the all-zero source: its two lists hold no split id
            lists = np.flatnonzero(it == args["zero"]) // L
            assert len(lists) == 2
            for u in lists:
                assert not np.isin(it[u * L:(u + 1) * L], want).any()
            # a mirrored cell above 65,535: the hottest tail id beside the first split id
            assert cls["big"][_TW], name
            if name in _BIG_CELL:
                A = it.reshape(-1, L)
                assert ((A == _TW).any(axis=1) & (A == want[0]).any(axis=1)).sum() > 65535, name


_CHILD = r"""
import json
import sys
import torch
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
pkg = ge.load_package()
from tests.test_gpu_mirror_staging import _CASES, _build, _digest
dev = torch.device("cuda")
out = {}
for name, (_, kw) in _CASES.items():
    up, it, M = _build(name)
    for any_order in (False, True):
        with pkg.CooccurrenceCore(n_items=M, device=0, any_order=any_order, **kw) as core:
            res = core.count_device(torch.from_numpy(up).to(dev), torch.from_numpy(it).to(dev))
            torch.cuda.current_stream().synchronize()
            assert core.last_mirror_rows() == 0
            out[f"{name}/{int(any_order)}"] = _digest(core.copy_batch(res.nnz, res.observed))
json.dump(out, open(sys.argv[2], "w"))
"""


@pytest.fixture(scope="module")
def mirror_off_digests(tmp_path_factory, torch_cuda):
    """Every log counted with COOC_SP_MIRROR=0, ordered and any-order, by one child process: the host copies'
    digests."""
    path = tmp_path_factory.mktemp("mstage_off") / "digests.json"
    env = dict(os.environ, COOC_SP_MIRROR="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, _ROOT, str(path)], env=env, cwd=_ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.load(open(path))


@pytest.mark.gpu
@pytest.mark.parametrize("any_order", [False, True])
@pytest.mark.parametrize("name", list(_CASES))
def test_record_staging_vs_brute_and_mirror_off(pkg, torch_cuda, mirror_off_digests, name, any_order):
    torch = torch_cuda
    up, it, M, brute = _log(name)
    kw = _CASES[name][1]
    W, L = _pair_work(up, it, M)
    split = np.flatnonzero(W > 2 ** 23)
    dev = torch.device("cuda")
    with pkg.CooccurrenceCore(n_items=M, device=0, any_order=any_order, **kw) as core:
        res = core.count_device(torch.from_numpy(up).to(dev), torch.from_numpy(it).to(dev))
        torch.cuda.current_stream().synchronize()
        assert core.last_mirror_rows() == len(split) > 0
        assert res.observed == (len(it) // L) * L * (L - 1)
        rows = _Rows(res, M)
        assert int(rows.rowsum.sum()) == res.observed and int(rows.nnz.sum()) == res.nnz
        chk = core.verify_batch()
        assert chk["rows_bad_sum"] == 0 and chk["rows_bad_entries"] == 0
        assert chk["sum_counts"] == chk["sum_rowsums"] == res.observed
        _check_rows(rows, brute, split)
        if name in _FULL or name == "base_relabelled":
            sample = _sample(it, M)
        else:  # the small universes: tail ids at both ends and around the tile edge
            present = np.flatnonzero(W[_TW:] > 0) + _TW
            sample = np.unique(np.concatenate([present[:3], present[-3:], present[(present >= _TW + _B - 2) &
                                                                                    (present < _TW + _B + 2)]]))
        _check_rows(rows, brute, sample)
        if name in _FULL:
            _check_rows(rows, brute, [_TW, _GAP[0] - 1, _GAP[1], _CASES[name][0]["zero"], M - 1])
        if name in _BIG_CELL:
            c, v = rows.row(int(split[0]))
            assert int(v[c == _TW][0]) > 65535  # the mirrored cell of the big source row 16384
        got = core.copy_batch(res.nnz, res.observed)
    assert _digest(got) == mirror_off_digests[f"{name}/{int(any_order)}"]
