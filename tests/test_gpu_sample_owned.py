"""cooc_sample_owned on one GPU, single process: without a communicator and on a world-1 communicator whose
collectives fail if called it is cooc_sample_device, array for array; with keys it is cooc_sample_device run on the
key space; two calls agree; its argument errors are cooc_sample_device's plus a negative key, and the context stays
usable.  The multi-rank windows are in tests/test_sample_owned_multiproc.py."""
import ctypes

import numpy as np
import pytest

import _sampled_model as sm
from test_gpu_sampled_comm import _never_called_ops

pytestmark = pytest.mark.gpu

SEED = 0x5EED
N_USERS, N_ITEMS, ITEM_CUT, USER_CUT = 12, 24, 20, 4


@pytest.fixture(scope="module", autouse=True)
def torch_cuda():
    """torch's runtime comes up before the library's first context, as in the other device-tensor tests"""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def log(torch_cuda):
    """sm.reference_log() on the device: users, items, window_ptr"""
    torch = torch_cuda
    windows = sm.reference_log()
    recs = [r for w in windows for r in w]
    dev = torch.device("cuda:0")
    users = torch.tensor([u for u, _ in recs], dtype=torch.int32, device=dev)
    items = torch.tensor([i for _, i in recs], dtype=torch.int32, device=dev)
    wp = np.concatenate([[0], np.cumsum([len(w) for w in windows])]).astype(np.int64)
    return users, items, wp


@pytest.fixture(scope="module")
def reference(pkg, log):
    """one sample_device call on the reference log: computed once, shared, left unchanged"""
    users, items, wp = log
    with pkg.CooccurrenceCore(n_items=N_ITEMS) as core:
        out = core.sample_device(users, items, N_USERS, ITEM_CUT, USER_CUT, seed=SEED, window_ptr=wp)
    assert out[4]["replacements"] > 0 and out[4]["feedbacks"] > 0 and out[4]["rejected"] > 0
    return out


def _same(a, b):
    import torch

    assert a[4] == b[4]
    for x, y in zip(a[:4], b[:4]):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)


@pytest.mark.parametrize("comm", ["none", "world1"])
def test_equals_sample_device(pkg, log, reference, comm):
    users, items, wp = log
    with pkg.CooccurrenceCore(n_items=N_ITEMS) as core:
        if comm == "world1":
            core.comm_init_ops(0, 1, _never_called_ops(pkg))
        out = core.sample_owned(users, items, N_USERS, None, ITEM_CUT, USER_CUT, seed=SEED, window_ptr=wp)
        _same(out, reference)
        again = core.sample_owned(users, items, N_USERS, None, ITEM_CUT, USER_CUT, seed=SEED, window_ptr=wp)
        _same(again, out)  # determinism
        _same(core.sample_device(users, items, N_USERS, ITEM_CUT, USER_CUT, seed=SEED, window_ptr=wp), reference)


@pytest.mark.parametrize("comm", ["none", "world1"])
def test_keys_equal_sample_device_on_the_key_space(pkg, log, reference, comm):
    """user_key = base + 3 j: the draw is keyed by the key, everything else by the index"""
    import torch

    from flink_cooccurrence_amd import sharding

    users, items, wp = log
    base = 1000
    keys = base + 3 * torch.arange(N_USERS, dtype=torch.int32, device=users.device)
    with pkg.CooccurrenceCore(n_items=N_ITEMS) as core:
        if comm == "world1":
            core.comm_init_ops(0, 1, _never_called_ops(pkg))
        want = core.sample_device(base + 3 * users, items, base + 3 * N_USERS, ITEM_CUT, USER_CUT, seed=SEED,
                                  window_ptr=wp)
        got = sharding.sample_owned(core, users, items, N_USERS, keys, ITEM_CUT, USER_CUT, seed=SEED, window_ptr=wp)
        again = core.sample_owned(users, items, N_USERS, keys, ITEM_CUT, USER_CUT, seed=SEED, window_ptr=wp)
    _same(again, got)
    assert got[4] == want[4]
    # the keys change the draws (from the model alone), and the call follows them
    by_index, by_key = (sm.SampledModel(N_ITEMS, ITEM_CUT, USER_CUT, SEED) for _ in range(2))
    for w in sm.reference_log():
        by_index.window(w)
        by_key.window([(base + 3 * u, i) for u, i in w])
    assert any(by_key.H[base + 3 * u] != by_index.H[u] for u in by_index.H)
    assert {key: by_key.H.get(key, []) for key in keys.tolist()} == \
        {key: got[1][got[0][j]:got[0][j + 1]].tolist() for j, key in enumerate(keys.tolist())}
    k = keys.long()
    wp_, gp = want[0].cpu().numpy(), got[0].cpu().numpy()
    wi, gi = want[1].cpu().numpy(), got[1].cpu().numpy()
    for j, key in enumerate(k.tolist()):
        assert gi[gp[j]:gp[j + 1]].tolist() == wi[wp_[key]:wp_[key + 1]].tolist(), f"user {j}"
    assert int(wp_[-1]) == int(gp[-1])
    assert torch.equal(got[2], want[2][k]) and int(want[2].sum()) == int(got[2].sum())
    assert torch.equal(got[3], want[3])


def test_a_rank_without_users(pkg):
    """n_users == 0 with n_records == 0: an empty CSR, zero counters"""
    import torch

    empty = torch.zeros(0, dtype=torch.int32, device="cuda:0")
    with pkg.CooccurrenceCore(n_items=N_ITEMS) as core:
        res_ptr, res_items, total, item_count, info = core.sample_owned(empty, empty, 0, None, ITEM_CUT, USER_CUT,
                                                                        window_ptr=[0, 0, 0])
        assert res_ptr.tolist() == [0] and res_items.numel() == 0 and total.numel() == 0
        assert int(item_count.abs().sum()) == 0 and set(info.values()) == {0}


def _raw(core, n, users, items, n_users=N_USERS, keys=None, n_windows=1, wp=None, item_cut=ITEM_CUT,
         user_cut=USER_CUT, res_ptr=None, res_items=None, res_cap=None, info=True):
    """cooc_sample_owned as given (no wrapper in between): its status and info"""
    from flink_cooccurrence_amd import _lib

    inf = _lib.CoocSampleInfo()
    wp = None if wp is None else np.ascontiguousarray(wp, np.int64)
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = _lib.load().cooc_sample_owned(
        core._h, n, vp(users), vp(items), n_users, vp(keys), n_windows,
        None if wp is None else wp.ctypes.data_as(_lib.i64p), item_cut, user_cut, SEED, vp(res_ptr), vp(res_items),
        (0 if res_items is None else res_items.numel()) if res_cap is None else res_cap, None, None, None,
        ctypes.byref(inf) if info else None)
    return st, inf


@pytest.mark.parametrize("comm", ["none", "world1"])
def test_errors(pkg, log, reference, comm):
    """cooc_sample_device's COOC_ERR_ARG cases and a negative key, each followed by a valid call"""
    import torch

    from flink_cooccurrence_amd import _lib

    users_ok, items_ok, wp8 = log
    users, items = users_ok.clone(), items_ok.clone()
    n = int(users.numel())
    dev = users.device
    res_ptr = torch.empty(N_USERS + 1, dtype=torch.int64, device=dev)
    res_items = torch.empty(n, dtype=torch.int32, device=dev)
    keys = torch.arange(N_USERS, dtype=torch.int32, device=dev)
    with pkg.CooccurrenceCore(n_items=N_ITEMS) as core:
        if comm == "world1":
            core.comm_init_ops(0, 1, _never_called_ops(pkg))

        def still_works():
            _same(core.sample_owned(users_ok, items_ok, N_USERS, None, ITEM_CUT, USER_CUT, seed=SEED, window_ptr=wp8),
                  reference)

        def refused(match=None, **kw):
            args = dict(n=n, users=users, items=items, res_ptr=res_ptr, res_items=res_items, n_windows=8, wp=wp8)
            args.update(kw)
            st, inf = _raw(core, **args)
            assert st == _lib.COOC_ERR_ARG
            if match is not None:
                assert match in _lib.load().cooc_last_error(core._h).decode()
            still_works()
            return inf

        for cut in (0, -1, 32768):
            refused(item_cut=cut)
            refused(user_cut=cut)
        refused(n_users=0)  # (allowed only without records)
        refused(n_users=-3)
        bad = wp8.copy()
        bad[0] = 1
        refused(wp=bad)
        bad = wp8.copy()
        bad[-1] = n - 1
        refused(wp=bad)
        bad = wp8.copy()
        bad[3], bad[4] = bad[4], bad[3]
        refused(wp=bad)
        refused(wp=None, n_windows=2)
        refused(n_windows=0)
        refused(res_ptr=None)
        refused(res_items=None, res_cap=n)
        refused(users=None)
        refused(items=None)
        refused(info=False, match="info is NULL")
        refused(res_cap=-1)
        refused(n=-1, wp=None, n_windows=1)
        refused(n=1 << 31, wp=None, n_windows=1)
        # ids out of range, in the middle of a window: found on the device, nothing written
        for where, col, value in ((200, users, N_USERS), (333, items, -1), (100, items, N_ITEMS), (45, users, -7)):
            keep = int(col[where])
            col[where] = value
            res_ptr.fill_(-5)
            res_items.fill_(-5)
            refused(match=f"record {where}:")
            assert int((res_ptr != -5).sum()) == 0 and int((res_items != -5).sum()) == 0
            col[where] = keep
        # a negative key: the first one is named, nothing written
        keys[7], keys[9] = -1, -4
        res_ptr.fill_(-5)
        refused(keys=keys, match="user_key[7] = -1")
        assert int((res_ptr != -5).sum()) == 0
        with pytest.raises(_lib.IllegalArgumentException, match="negative"):
            core.sample_owned(users, items, N_USERS, keys, ITEM_CUT, USER_CUT, seed=SEED, window_ptr=wp8)
        # res_cap below the reservoirs' size: the size needed comes back
        need = reference[4]["reservoir_items"]
        inf = refused(res_cap=need - 1)
        assert inf.reservoir_items == need
        with pytest.raises(_lib.IllegalArgumentException):
            core.sample_owned(users, items, N_USERS, None, ITEM_CUT, USER_CUT, seed=SEED, window_ptr=wp8, res_cap=0)
        assert core.last_sample_info["reservoir_items"] == need
        _same(core.sample_owned(users, items, N_USERS, None, ITEM_CUT, USER_CUT, seed=SEED, window_ptr=wp8,
                                res_cap=need), reference)
