"""Split rows whose columns above the first tile come from the transposed rows (C[a, b] = C[b, a]): when every
split row's column lies in tile 0, a split share walks the lists' tile-0 parts only and the rows of column rank
>= 16,384 store their tile-0 entries into the split rows' staging rows (k_sp_main's dense and hash compactions,
the runs of k_sp_small and k_sp_tiny).  Against rows summed directly from the lists, and against the same run
with COOC_SP_MIRROR=0 in a child process (the knob is read when a core is created).  Needs an MI355X.

The log (320,000 lists of 30 ids, M = 200,000; N = 9.6e6, P = 2.784e8): the items 0..3 in every list, item 0 a
second time in every fifth list, 6 ids uniform in [4, 16384) (5 beside the second item 0), 20 tail ids
log-uniform over [16384, M) (id 16384 + floor(e^(u ln(M - 16384))) - 1), the columns 16384 and M - 1 planted in
every 1,000th list.  Rows by pair work: 5 split (0..3 and the hottest tail id 16384), 241 big, 3,957 mid, 78,019
small, 115,423 tiny; tail ids in every class.  About 4,900 tail ids are more frequent than the uniform head ids:
the relabel moves them into tile 0.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_sparse import _Brute, _check_rows, _Rows

pytestmark = pytest.mark.gpu

_TW = 16384  # k_sp_main's tile width
_M = 200_000
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _mirror_log(variant="base", seed=31, U=320_000, M=_M):
    """variant: "base"; "ranked": the same log with the ids renumbered by descending frequency (every hot item
    below 16,384: the relabel is skipped); "swap": ids 4 and 16384 exchanged (with kept ids every split row is
    in tile 0 and the big and mid rows 16385.. lie above it: mirror sources in k_sp_main's both shapes);
    "tail_split": id 20000 in every list (with kept ids a split row outside tile 0)."""
    rng = np.random.default_rng(seed)
    L = np.empty((U, 30), np.int32)
    L[:, 0:4] = np.arange(4)
    L[:, 4:10] = rng.integers(4, _TW, (U, 6))
    L[::5, 4] = 0
    span = M - _TW
    L[:, 10:30] = _TW + np.minimum(np.exp(rng.random((U, 20)) * np.log(span)).astype(np.int64) - 1, span - 1)
    L[::1000, 10] = _TW
    L[::1000, 11] = M - 1
    if variant == "tail_split":
        L[:, 12] = 20000
    L = rng.permuted(L, axis=1)
    it = L.reshape(-1)
    if variant == "ranked":
        rank = np.empty(M, np.int32)
        rank[np.argsort(-np.bincount(it, minlength=M), kind="stable")] = np.arange(M, dtype=np.int32)
        it = rank[it]
    elif variant == "swap":
        m = np.arange(M, dtype=np.int32)
        m[4], m[_TW] = _TW, 4
        it = m[it]
    return np.arange(U + 1, dtype=np.int64) * 30, np.ascontiguousarray(it, np.int32), M


def _classes(it, M):
    W = 30 * np.bincount(it, minlength=M).astype(np.int64)
    return {"split": W > 2 ** 23, "big": (W > 65535) & (W <= 2 ** 23), "mid": (W > 4096) & (W <= 65535),
            "small": (W > 256) & (W <= 4096), "tiny": (W > 0) & (W <= 256)}


def _sample(it, M, n=60, seed=5):
    """n rows, every class among them, tail ids of every non-split class among them."""
    rng = np.random.default_rng(seed)
    cls = _classes(it, M)
    tail = np.arange(M) >= _TW
    picks = []
    for name in ("big", "mid", "small", "tiny"):
        for part in (cls[name] & tail, cls[name] & ~tail):
            ids = np.flatnonzero(part)
            if len(ids):
                picks.append(rng.choice(ids, min(len(ids), 7), replace=False))
    picks = np.unique(np.concatenate(picks + [[_TW, M - 1]]))
    rest = np.setdiff1d(np.flatnonzero(~cls["split"] & (np.bincount(it, minlength=M) > 0)), picks)
    return np.concatenate([picks, rng.choice(rest, n - len(picks), replace=False)])


_LOGS = {}


def _log(variant):
    if variant not in _LOGS:
        up, it, M = _mirror_log(variant)
        _LOGS[variant] = (up, it, M, _Brute(up, it, M))
    return _LOGS[variant]


def _count_and_check(pkg, torch, variant, any_order, want_mirror, copy=False, **kw):
    """One count of the variant's log: observed, the row sums' total, cooc_verify_batch, every split row and 60
    sampled rows against the brute-force rows.  Returns the core's sorted host copy (copy=True)."""
    up, it, M, brute = _log(variant)
    cls = _classes(it, M)
    dev = torch.device("cuda")
    with pkg.CooccurrenceCore(n_items=M, device=0, any_order=any_order, **kw) as core:
        res = core.count_device(torch.from_numpy(up).to(dev), torch.from_numpy(it).to(dev))
        torch.cuda.current_stream().synchronize()
        n_mirror = core.last_mirror_rows()
        print(f"{variant} any_order={any_order} {kw}: mirror rows {n_mirror}, nnz {res.nnz}, "
              f"split {int(cls['split'].sum())}")
        if want_mirror:
            assert n_mirror == int(cls["split"].sum()) > 0
        else:
            assert n_mirror == 0
        lens = np.diff(up)
        assert res.observed == int(np.sum(lens * (lens - 1)))
        rows = _Rows(res, M)
        assert int(rows.rowsum.sum()) == res.observed and int(rows.nnz.sum()) == res.nnz
        chk = core.verify_batch()
        assert chk["rows_bad_sum"] == 0 and chk["rows_bad_entries"] == 0
        assert chk["sum_counts"] == chk["sum_rowsums"] == res.observed
        _check_rows(rows, brute, np.flatnonzero(cls["split"]))
        _check_rows(rows, brute, _sample(it, M))
        return core.copy_batch(res.nnz, res.observed) if copy else None


_CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
pkg = ge.load_package()
from tests.test_gpu_mirror import _mirror_log
up, it, M = _mirror_log("base")
dev = torch.device("cuda")
for any_order in (False, True):
    with pkg.CooccurrenceCore(n_items=M, device=0, any_order=any_order) as core:
        res = core.count_device(torch.from_numpy(up).to(dev), torch.from_numpy(it).to(dev))
        torch.cuda.current_stream().synchronize()
        assert core.last_mirror_rows() == 0
        got = core.copy_batch(res.nnz, res.observed)
    np.savez(sys.argv[2] + f"/off_{int(any_order)}.npz", row_ptr=got.row_ptr, cols=got.cols, cnt=got.cnt,
             rowsum=got.rowsum)
"""


@pytest.fixture(scope="module")
def mirror_off_runs(tmp_path_factory, torch_cuda):
    """The base log counted with COOC_SP_MIRROR=0, ordered and any-order, by one child process."""
    out = tmp_path_factory.mktemp("mirror_off")
    env = dict(os.environ, COOC_SP_MIRROR="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, _ROOT, str(out)], env=env, cwd=_ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


@pytest.mark.parametrize("any_order", [False, True])
def test_mirrored_split_rows_vs_brute_and_knob_off(pkg, torch_cuda, mirror_off_runs, any_order):
    """The base log: mirroring on, the split rows' whole rows and 60 sampled rows of every class exact, and the
    whole result (host copy, every row sorted by column) identical to the COOC_SP_MIRROR=0 child's."""
    up, it, M, _ = _log("base")
    cls = _classes(it, M)
    assert int(cls["split"].sum()) == 5 and all(int(cls[k].sum()) > 0 for k in cls)
    assert all(int(cls[k][_TW:].sum()) > 0 for k in ("big", "mid", "small", "tiny"))
    got = _count_and_check(pkg, torch_cuda, "base", any_order, True, copy=True)
    off = np.load(os.path.join(str(mirror_off_runs), f"off_{int(any_order)}.npz"))
    assert np.array_equal(got.row_ptr, off["row_ptr"]) and np.array_equal(got.cols, off["cols"])
    assert np.array_equal(got.cnt, off["cnt"]) and np.array_equal(got.rowsum, off["rowsum"])


@pytest.mark.parametrize("any_order", [False, True])
def test_mirrored_split_rows_item_ranked_ids(pkg, torch_cuda, any_order):
    """Ids already in frequency order: no relabel, the five split rows are the ids 0..4."""
    _count_and_check(pkg, torch_cuda, "ranked", any_order, True)


@pytest.mark.parametrize("any_order", [False, True])
def test_mirror_sources_in_both_shapes_kept_ids(pkg, torch_cuda, any_order):
    """Kept ids with the hottest tail id moved to id 4: the big and mid rows 16385.. have column ranks above tile
    0, so the dense and hash compactions of both k_sp_main shapes store into the staging rows."""
    up, it, M, _ = _log("swap")
    cls = _classes(it, M)
    assert not cls["split"][_TW:].any() and cls["big"][_TW:].sum() > 100 and cls["mid"][_TW:].sum() > 1000
    _count_and_check(pkg, torch_cuda, "swap", any_order, True, column_order=True)


def test_split_row_outside_tile0_is_not_mirrored(pkg, torch_cuda):
    """Kept ids and id 20000 in every list: a split row outside tile 0 switches mirroring off; exact."""
    up, it, M, _ = _log("tail_split")
    assert _classes(it, M)["split"][20000]
    _count_and_check(pkg, torch_cuda, "tail_split", True, False, column_order=True)


def test_deferred_row_repeats_without_mirroring(pkg, torch_cuda):
    """A split row (item 0, in every list) plus a row built to overflow its hash table (three lists of 2,500 ids
    that occur nowhere else, as tests/test_gpu_mid4.py): the overflowing row, a mirror source with kept ids,
    leaves through the sort path, so the run is repeated without mirroring.  Exact, both orders."""
    torch = torch_cuda
    rng = np.random.default_rng(41)
    U, M, ovf = 290_000, 300_000, 250_000
    L = np.empty((U, 31), np.int32)
    L[:, 0] = 0
    L[:, 1:10] = rng.integers(1, 2000, (U, 9))
    L[:, 10:30] = rng.integers(_TW, _TW + 3000, (U, 20))
    L[:, 30] = rng.integers(2000, 2048, U)  # 48 rows above the mid class: a big-shape launch beside the mid one
    own = rng.permutation(np.arange(100_000, 100_000 + _TW))[:7500].reshape(3, 2500)
    extra = [np.concatenate([[ovf], own[k], [0, 7, 7]]).astype(np.int32) for k in range(3)]
    it = np.concatenate([rng.permuted(L, axis=1).reshape(-1)] + extra)
    up = np.concatenate([np.arange(U + 1, dtype=np.int64) * 31, U * 31 + np.cumsum([len(x) for x in extra])])
    brute = _Brute(up, it, M)
    lens = np.diff(up)
    dev = torch.device("cuda")
    sample = np.concatenate([[0, ovf, 7, int(own[0, 0]), int(own[2, 17])], rng.integers(1, 2000, 6),
                             rng.integers(_TW, _TW + 3000, 6)])
    for any_order in (False, True):
        with pkg.CooccurrenceCore(n_items=M, device=0, any_order=any_order, column_order=True) as core:
            res = core.count_device(torch.from_numpy(up).to(dev), torch.from_numpy(it).to(dev))
            torch.cuda.current_stream().synchronize()
            assert core.last_sort_rows()[0] >= 1, "the overflowing row was not deferred"
            assert core.last_mirror_rows() == 0
            assert res.observed == int(np.sum(lens * (lens - 1)))
            rows = _Rows(res, M)
            assert int(rows.rowsum.sum()) == res.observed and int(rows.nnz.sum()) == res.nnz
            chk = core.verify_batch()
            assert chk["rows_bad_sum"] == 0 and chk["rows_bad_entries"] == 0
            assert chk["sum_counts"] == chk["sum_rowsums"] == res.observed
            _check_rows(rows, brute, sample)


def test_owned_parts_do_not_mirror_and_equal_the_whole(pkg, torch_cuda):
    """count_device_owned over 2 parts of the base log: mirroring off (a part does not count every row), and each
    part's rows equal the whole count's."""
    torch = torch_cuda
    from flink_cooccurrence_amd import sharding

    up, it, M, _ = _log("base")
    dev = torch.device("cuda")
    up_d, it_d = torch.from_numpy(up).to(dev), torch.from_numpy(it).to(dev)
    freq_d = torch.from_numpy(np.bincount(it, minlength=M).astype(np.int64)).to(dev)
    owner_d = sharding.snake_owner(freq_d, 2)
    owner = owner_d.cpu().numpy()
    picks = np.concatenate([np.flatnonzero(_classes(it, M)["split"]), _sample(it, M, seed=9)])
    with pkg.CooccurrenceCore(n_items=M, device=0) as core:
        whole = core.count_device(up_d, it_d)
        torch.cuda.current_stream().synchronize()
        assert core.last_mirror_rows() == 5
        w = _Rows(whole, M)
        want = {int(a): w.row(int(a)) for a in picks}
        w_nnz, w_rowsum = w.nnz.copy(), w.rowsum.copy()
    nnz_total = 0
    for part in range(2):
        with pkg.CooccurrenceCore(n_items=M, device=0) as core:
            res = core.count_device_owned(up_d, it_d, owner_d, part, freq_d, int(len(it)))
            torch.cuda.current_stream().synchronize()
            assert core.last_mirror_rows() == 0
            r = _Rows(res, M)
            mine = owner == part
            assert np.array_equal(r.nnz[mine], w_nnz[mine]) and np.all(r.nnz[~mine] == 0)
            assert np.array_equal(r.rowsum[mine], w_rowsum[mine])
            nnz_total += res.nnz
            for a, (wc, wn) in want.items():
                if owner[a] == part:
                    gc, gn = r.row(a)
                    assert np.array_equal(gc, wc) and np.array_equal(gn, wn)
    assert nnz_total == whole.nnz
