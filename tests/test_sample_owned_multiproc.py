"""cooc_sample_owned across ranks: p = 2 and p = 3 processes on the box's one GPU, the communicator over gloo
(cooc_comm_ops through sharding.init_comm_torch_ops), every rank holding its users' shard (user u on rank u mod p)
of a log in device memory.  The contract (include/cooc.h, "device-side sampler across GPUs"): window w of the job is
R_0[w] || R_1[w] || ..., and the union of the ranks' outputs equals, bit for bit, one cooc_sample_device call over
the serialised log with the keys as user ids -- and tests/_sampled_model.SampledModel fed the same.

One spawn per world size runs, in this order: the dictated log of tests/_sampled_comm.py in a 300-item and a
70,000-item universe (cuts 5/2; it reaches the multi-rank branches, checked on the model before anything is
compared; window 6 has no feedback on any rank, windows 1-3 more than a wave's worth), the wide log of
tests/_sample_owned.py (700 records per rank and window, an empty rank-window), two disagreeing calls after which
the communicator still works, and at p = 2 the pipeline sample_owned -> count_owned -> topk_owned.  Needs an
MI355X."""
import datetime
import os
import pickle
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (at collection, before any test opens the GPU through the library: torch.cuda finds it)

import _sample_owned as so
import _sampled_comm as sc
from test_multiproc_gpu import _free_port, _rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
TOPK = 5
E2E = "dictated-70000"


def _logs(world):
    """name -> (windows, n_items, item_cut, user_cut)"""
    return {"dictated-300": (sc.dictated_log(world, 300)[0], 300, sc.ITEM_CUT, sc.USER_CUT),
            "dictated-70000": (sc.dictated_log(world, 70_000)[0], 70_000, sc.ITEM_CUT, sc.USER_CUT),
            "wide": (so.wide_log(world), so.WIDE_ITEMS, so.WIDE_ITEM_CUT, so.WIDE_USER_CUT)}


def _host(out):
    return [t.cpu().numpy() for t in out[:4]] + [out[4]]


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    for p in (ROOT, TESTS):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist

    import __graft_entry__

    pkg = __graft_entry__.load_package()
    from flink_cooccurrence_amd import _lib, sharding

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    # (a mismatched collective fails after a minute instead of hanging)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    out, cores, kept = {}, {}, {}

    def call(core, item_cut, user_cut, users, items, keys, wp):
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        return sharding.sample_owned(core, to(users), to(items), len(keys), to(keys), item_cut, user_cut,
                                     seed=sc.SEED, window_ptr=wp)

    # ---- 1., 2.: the dictated log in both universes, the wide log
    for name, (windows, n_items, item_cut, user_cut) in _logs(world).items():
        core = cores[name] = pkg.CooccurrenceCore(n_items=n_items, device=0)
        sharding.init_comm_torch_ops(core)
        kept[name] = call(core, item_cut, user_cut, *so.shard(windows, rank))
        out[name] = _host(kept[name])
        if name == "wide":  # determinism: a second call on the same inputs
            out["wide-again"] = _host(call(core, item_cut, user_cut, *so.shard(windows, rank)))
    # ---- 4.: disagreement, then a valid call on the same communicator
    windows, _, item_cut, user_cut = _logs(world)["dictated-300"]
    users, items, keys, wp = so.shard(windows, rank)
    core = cores["dictated-300"]
    messages = []
    bad_items = items.copy()
    bad_items[5] = 300
    for args in ((users, items, keys, np.append(wp, wp[-1]) if rank == 1 else wp),  # one more (empty) window
                 (users, bad_items if rank == 0 else items, keys, wp)):               # an item out of range
        try:
            call(core, item_cut, user_cut, *args)
            messages.append(None)
        except _lib.IllegalArgumentException as e:
            messages.append(str(e))
    out["messages"] = messages
    out["after-errors"] = _host(call(core, item_cut, user_cut, users, items, keys, wp))
    # ---- 5.: end to end, the reservoirs into count_owned and topk_owned
    if world == 2:
        core = cores[E2E]
        M = core.n_items
        res = sharding.count_owned(core, kept[E2E][0], kept[E2E][1])
        torch.cuda.current_stream().synchronize()
        rp, cols, cnt, rowsum = _rows(res.owned, M)
        tk = sharding.topk_owned(core, res, TOPK)
        torch.cuda.current_stream().synchronize()
        out["e2e"] = dict(rp=rp, cols=cols, cnt=cnt, rowsum=rowsum, owner=res.owner.cpu().numpy(),
                          observed=int(res.observed), sizes=tk.sizes.cpu().numpy(), values=tk.values.cpu().numpy(),
                          scores=tk.scores.cpu().numpy(), tk_rowsum=tk.rowsum.cpu().numpy())
    for core in cores.values():
        core.close()
    with open(os.path.join(out_dir, f"rank{rank}.pkl"), "wb") as f:
        pickle.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


_SPAWNED: dict = {}


def _parts(world, tmp_path_factory):
    """the ranks' results at `world`: one spawn per world size, shared by every test of the module"""
    if world not in _SPAWNED:
        import torch.multiprocessing as mp

        out_dir = tmp_path_factory.mktemp(f"world{world}")
        mp.spawn(_worker, args=(world, _free_port(), str(out_dir)), nprocs=world, join=True)
        _SPAWNED[world] = [pickle.load(open(out_dir / f"rank{r}.pkl", "rb")) for r in range(world)]
    return _SPAWNED[world]


_SINGLE: dict = {}


def _single(pkg, world, name):
    """one cooc_sample_device call over the serialised log, the job-wide ids as user indices (made once per log)"""
    if (world, name) not in _SINGLE:
        import torch

        windows, n_items, item_cut, user_cut = _logs(world)[name]
        users, items, wp = so.serial_log(windows)
        dev = torch.device("cuda:0")
        with pkg.CooccurrenceCore(n_items=n_items, device=0) as core:
            out = core.sample_device(torch.from_numpy(users).to(dev), torch.from_numpy(items).to(dev),
                                     int(users.max()) + 1, item_cut, user_cut, seed=sc.SEED, window_ptr=wp)
            _SINGLE[(world, name)] = _host(out)
    return _SINGLE[(world, name)]


def _assert_log(pkg, parts, world, name, key=None):
    windows, n_items, item_cut, user_cut = _logs(world)[name]
    model, decisions = so.model_of(windows, n_items, item_cut, user_cut, sc.SEED)
    s_ptr, s_items, s_total, s_count, s_info = _single(pkg, world, name)
    for r, p in enumerate(parts):
        keys = so.rank_users(windows, r)
        res_ptr, res_items, total, item_count, info = p[key or name]
        # against the model
        ptr, items, tot, count, want = so.expected_rank(model, decisions, keys, r, n_items)
        assert info == want, f"rank {r}"
        assert np.array_equal(res_ptr, ptr) and np.array_equal(res_items, items), f"rank {r}: reservoirs (slot order)"
        assert np.array_equal(total, tot) and np.array_equal(item_count, count), f"rank {r}"
        # against the single call over the serialised log
        for j, u in enumerate(keys):
            assert res_items[res_ptr[j]:res_ptr[j + 1]].tolist() == s_items[s_ptr[u]:s_ptr[u + 1]].tolist(), f"user {u}"
        assert np.array_equal(total, s_total[keys])
        assert np.array_equal(item_count, s_count) and np.array_equal(item_count, parts[0][key or name][3])
        assert info["item_counter_sum"] == s_info["item_counter_sum"]
    for k in ("rejected", "fills", "replacements", "feedbacks", "users", "reservoir_items"):
        assert sum(p[key or name][4][k] for p in parts) == s_info[k], k
    assert int(s_total.sum()) == sum(int(p[key or name][2].sum()) for p in parts)  # no user outside the shards


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.mark.parametrize("n_items", [300, 70_000])
@pytest.mark.parametrize("world", [2, 3])
def test_dictated_log(pkg, torch_cuda, tmp_path_factory, world, n_items):
    windows, marks = sc.dictated_log(world, n_items)
    # the log must reach the multi-rank branches: from the model's run, before anything of the library is looked at
    got, _, _ = sc.reached(world, windows, n_items, marks)
    assert got >= set("abcdef"), f"the log no longer reaches {sorted(set('abcdef') - got)}"
    _, decisions = so.model_of(windows, n_items, sc.ITEM_CUT, sc.USER_CUT, sc.SEED)
    feedbacks = [sum(d == "b" for ds in by_rank for d in ds) for by_rank in decisions]
    assert feedbacks[6] == 0 and sum(len(R) for R in windows[6]) > 0  # no list gathered
    assert all(f > 64 for f in feedbacks[1:4])
    _assert_log(pkg, _parts(world, tmp_path_factory), world, f"dictated-{n_items}")


@pytest.mark.parametrize("world", [2, 3])
def test_wide_log(pkg, torch_cuda, tmp_path_factory, world):
    windows = so.wide_log(world)
    _, decisions = so.model_of(windows, so.WIDE_ITEMS, so.WIDE_ITEM_CUT, so.WIDE_USER_CUT, sc.SEED)
    rank_windows = [ds for by_rank in decisions for ds in by_rank]
    assert any(len(ds) > 256 and sum(d == "b" for d in ds) >= 65 for ds in rank_windows)
    assert any(d[0] == "k" for ds in rank_windows for d in ds)
    assert any(not ds for ds in rank_windows)
    got, _, _ = sc.reached(world, windows, so.WIDE_ITEMS, None, so.WIDE_ITEM_CUT, so.WIDE_USER_CUT, sc.SEED)
    assert "a" in got
    parts = _parts(world, tmp_path_factory)
    _assert_log(pkg, parts, world, "wide")
    for p in parts:  # determinism
        assert p["wide-again"][4] == p["wide"][4]
        assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(p["wide-again"][:4], p["wide"][:4]))


@pytest.mark.parametrize("world", [2, 3])
def test_disagreement_fails_every_rank_and_leaves_the_communicator_usable(pkg, torch_cuda, tmp_path_factory, world):
    parts = _parts(world, tmp_path_factory)
    for r, p in enumerate(parts):
        windows_differ, bad_item = p["messages"]
        assert windows_differ is not None and bad_item is not None, f"rank {r} did not fail"
        assert "rank 1 passed n_windows 9" in windows_differ and "rank 0 n_windows 8" in windows_differ
        if r == 0:  # the failing rank names its own cause, the others name the rank
            assert "record 5:" in bad_item and "item 300 (of 300)" in bad_item
        else:
            assert "rank 0 failed its checks" in bad_item
    _assert_log(pkg, parts, world, "dictated-300", key="after-errors")
    for p in parts:
        assert p["after-errors"][4] == p["dictated-300"][4]
        assert all(np.array_equal(a, b) for a, b in zip(p["after-errors"][:4], p["dictated-300"][:4]))


def test_end_to_end_sample_count_topk(pkg, torch_cuda, tmp_path_factory):
    """p = 2, 70,000 items: sample_owned -> count_owned -> topk_owned equals one process's sample_device ->
    count_device -> topk_batch on the serialised log"""
    import torch

    world = 2
    parts = _parts(world, tmp_path_factory)
    windows, M, item_cut, user_cut = _logs(world)[E2E]
    users, items, wp = so.serial_log(windows)
    dev = torch.device("cuda:0")
    with pkg.CooccurrenceCore(n_items=M, device=0) as core:
        res_ptr, res_items, _, _, _ = core.sample_device(torch.from_numpy(users).to(dev), torch.from_numpy(items).to(dev),
                                                         int(users.max()) + 1, item_cut, user_cut, seed=sc.SEED,
                                                         window_ptr=wp)
        whole = core.count_device(res_ptr, res_items)
        torch.cuda.current_stream().synchronize()
        w_rp, w_cols, w_cnt, w_rowsum = _rows(whole, M)
        sizes = torch.empty(M, dtype=torch.int32, device=dev)
        vals = torch.empty((M, TOPK), dtype=torch.int32, device=dev)
        scores = torch.empty((M, TOPK), dtype=torch.float64, device=dev)
        core.topk_batch_device(TOPK, sizes, vals, scores)
        torch.cuda.current_stream().synchronize()
        w_sz, w_v, w_sc = sizes.cpu().numpy(), vals.cpu().numpy(), scores.cpu().numpy()
        observed = int(whole.observed)
    assert observed > 0 and int(w_rowsum.sum()) == observed
    owner = parts[0]["e2e"]["owner"]
    assert np.array_equal(owner, parts[1]["e2e"]["owner"])
    w_nnz = np.diff(w_rp)
    covered = np.zeros(M, bool)
    for r, p in enumerate(parts):
        e = p["e2e"]
        mine = owner == r
        covered |= mine
        nnz = np.diff(e["rp"])
        assert e["observed"] == observed
        assert np.all(nnz[~mine] == 0) and np.array_equal(nnz[mine], w_nnz[mine])
        assert np.array_equal(e["rowsum"][mine], w_rowsum[mine]) and np.array_equal(e["tk_rowsum"], w_rowsum)
        for a in np.flatnonzero(mine & (w_nnz > 0)):
            sl, ws = slice(e["rp"][a], e["rp"][a + 1]), slice(w_rp[a], w_rp[a + 1])
            o1, o2 = np.argsort(e["cols"][sl], kind="stable"), np.argsort(w_cols[ws], kind="stable")
            assert np.array_equal(e["cols"][sl][o1], w_cols[ws][o2]) and np.array_equal(e["cnt"][sl][o1], w_cnt[ws][o2])
        assert np.all(e["sizes"][~mine] == 0) and np.array_equal(e["sizes"][mine], w_sz[mine])
        for a in np.flatnonzero(mine & (w_sz > 0)):
            n = int(w_sz[a])
            assert np.array_equal(e["values"][a, :n], w_v[a, :n]), f"row {a}"
            assert np.array_equal(e["scores"][a, :n], w_sc[a, :n], equal_nan=True), f"row {a}"
    assert covered.all() and any(np.any(np.diff(p["e2e"]["rp"]) > 0) for p in parts)
