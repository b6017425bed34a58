"""cooc_count_owned / cooc_topk_owned below 40,320 items across ranks: 2 and 3 processes on the box's one GPU, the
communicator over gloo (cooc_comm_ops through sharding.init_comm_torch_ops), user u on rank u mod world.  The contract
(include/cooc.h, "small universes"): row a is complete on rank a mod world, the result is a padded CSR over all
n_items rows with every other row empty, it is the context's batch result (cooc_copy_batch*, cooc_verify_batch,
cooc_topk_owned*, cooc_topk_items read it), and a failure on one rank fails every rank before any payload moves.

One spawn per world size, every child under a time limit (tests/_owned_small.spawn), runs in this order: log A twice
(determinism) with its top-k, log A from host arrays, the calls with one item id out of range on rank 1 and with a
malformed host user_ptr on rank 0, followed by a valid one, at two ranks the replay of the JVM operators' call
sequence, log A capped by user_cut = 3, log C (the last rank without users), at three ranks log B (M = 2: rank 2
owns no row; M = 7), a second context at n_items = 70,000 (the large-universe exchange, unchanged), and at two
ranks the split-row log.  Everything is compared with == against oracle.closed_form and oracle.rows_topk over the
whole log.

Log A's expected matrix has non-empty rows on every rank at world 2 and 3 (asserted below from the closed form).
Without the feature every case but the 70,000-item control fails with COOC_ERR_ARG.  Needs an MI355X."""
import datetime
import os
import pickle
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (at collection, before any test opens the GPU through the library: torch.cuda finds it)

import _owned_small as osm
from test_multiproc_gpu import _d2h, _free_port, _rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
TOPK = osm.TOPK
RANGE = (37, 173)  # rows of copy_batch_range: owned and non-owned ones at both world sizes
MIXED = [0, 1, 2, 3, 5, 44, 150, 151, 299, 300]  # topk_items: owned and non-owned at both world sizes
REPLAY_WINDOW = (5000, 5999)


def _count(core, sharding, torch, up, it, M, topk=True):
    """one count_owned (and topk_owned) on this rank's users -> everything the checks read, as host arrays"""
    dev = torch.device("cuda", 0)
    res = sharding.count_owned(core, torch.from_numpy(up).to(dev), torch.from_numpy(it).to(dev))
    torch.cuda.current_stream().synchronize()
    rp, cols, cnt, rowsum = _rows(res.owned, M)
    b = core.copy_batch(int(res.owned.nnz), int(res.owned.observed))
    if M < sharding.SMALL_UNIVERSE_ITEMS:  # (device rows in ascending column order: the host copy is the same arrays)
        assert np.array_equal(b.row_ptr, rp) and np.array_equal(b.cols, cols) and np.array_equal(b.cnt, cnt)
    assert np.array_equal(b.rowsum, rowsum)
    v = core.verify_batch()
    out = dict(rp=rp, cols=cols, cnt=cnt, cnt16=b.cnt16, rowsum=rowsum, owner=res.owner.cpu().numpy(),
               observed=int(res.observed), local_observed=int(res.local_observed), n_users_all=int(res.n_users_all),
               n_all=int(res.n_interactions_all), gathered=int(res.gathered_bytes), nnz=int(res.owned.nnz),
               n_items=int(res.owned.n_items), verify=v)
    tk = None
    if topk:
        t = sharding.topk_owned(core, res, TOPK)
        torch.cuda.current_stream().synchronize()
        sizes = t.sizes.cpu().numpy()
        live = np.arange(TOPK)[None, :] < sizes[:, None]  # (the library writes a heap's first `size` entries only)
        tk = dict(sizes=sizes, values=np.where(live, t.values.cpu().numpy(), 0),
                  scores=np.where(live, t.scores.cpu().numpy(), 0.0), rowsum=t.rowsum.cpu().numpy())
    return out, tk, res


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

    torch.cuda.set_device(0)
    # (a mismatched collective fails after a minute instead of hanging)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    out = {}
    up_a, it_a, M = osm.log_a()
    up, it = osm.shard(up_a, it_a, world, rank)
    with pkg.CooccurrenceCore(n_items=M, device=0) as core:
        sharding.init_comm_torch_ops(core)
        # ---- log A, twice; the info's device views; range copies; top-k through both entry points
        out["a"], out["a_topk"], res = _count(core, sharding, torch, up, it, M)
        info_counts = core.count_owned(torch.from_numpy(up).cuda(), torch.from_numpy(it).cuda())[1]
        torch.cuda.current_stream().synchronize()
        out["a_item_counts"] = _d2h(info_counts.item_counts, M, np.int64)
        out["a_again"], out["a_again_topk"], _ = _count(core, sharding, torch, up, it, M)
        rp = out["a_again"]["rp"]
        n = int(rp[RANGE[1]] - rp[RANGE[0]])
        out["a_range"] = core.copy_batch_range(RANGE[0], RANGE[1], max(n, 1)) + (n,)
        core.topk_owned_host(TOPK)  # (collective) the heaps into the context's buffers, for topk_items
        out["a_items"] = core.topk_items(MIXED, TOPK)
        # ---- the same from host arrays (a JVM subtask's call)
        b, info = core.count_owned_host(up, it)
        winfo, _ = core.count_owned_host_info(up, it)
        out["a_host"] = dict(rp=b.row_ptr, cols=b.cols, cnt=b.cnt, cnt16=b.cnt16, rowsum=b.rowsum,
                             observed=int(info.observed), local_observed=int(info.local_observed),
                             winfo=(int(winfo.nnz), int(winfo.observed), int(winfo.n_rows)))
        # ---- errors never leave a peer waiting: rank 1 passes one item id equal to M, then everyone a valid log
        bad = it.copy()
        if rank == 1:
            bad[3] = M
        try:
            sharding.count_owned(core, torch.from_numpy(up).cuda(), torch.from_numpy(bad).cuda())
            out["message"] = None
        except _lib.IllegalArgumentException as e:
            out["message"] = str(e)
        # (the same for a check made on the host before anything reaches the device: rank 0's user_ptr[0] != 0)
        bad_up = up.copy()
        if rank == 0:
            bad_up[0] = 1
        try:
            core.count_owned_host(bad_up, it)
            out["message_host"] = None
        except _lib.IllegalArgumentException as e:
            out["message_host"] = str(e)
        out["a_after_error"], _, _ = _count(core, sharding, torch, up, it, M, topk=False)
        # ---- the JVM operators' call sequence at M = 301 (the driver class of test_owned_operator_replay)
        if world == 2:
            from test_owned_operator_replay import _OwnedSubtask

            op = _OwnedSubtask(core, M, TOPK)
            users = np.repeat(np.arange(len(up_a) - 1), np.diff(up_a))
            for k in np.flatnonzero(users % world == rank):
                op.process_element(int(users[k]), int(it_a[k]), REPLAY_WINDOW[0] + int(k) % 999)
            assert op.process_watermark(REPLAY_WINDOW[0] - 1) is None
            out["replay"] = op.process_watermark(REPLAY_WINDOW[1])
    # ---- user_cut = 3: the union is the closed form of the capped log
    with pkg.CooccurrenceCore(n_items=M, device=0, user_cut=3) as core:
        sharding.init_comm_torch_ops(core)
        out["cut"], _, _ = _count(core, sharding, torch, up, it, M, topk=False)
    # ---- log C: the last rank holds no user and still takes part
    with pkg.CooccurrenceCore(n_items=M, device=0) as core:
        sharding.init_comm_torch_ops(core)
        up_c, it_c = osm.shard(up_a, it_a, world, rank, ranks_with_users=world - 1)
        assert (len(up_c) == 1) == (rank == world - 1)
        out["c"], out["c_topk"], _ = _count(core, sharding, torch, up_c, it_c, M)
    # ---- log B: fewer rows than ranks (M = 2 at three ranks: rank 2 owns no row), and M = 7
    if world == 3:
        for Mb in (2, 7):
            up_b, it_b, _ = osm.log_b(Mb)
            with pkg.CooccurrenceCore(n_items=Mb, device=0) as core:
                sharding.init_comm_torch_ops(core)
                out[f"b{Mb}"], out[f"b{Mb}_topk"], _ = _count(core, sharding, torch, *osm.shard(up_b, it_b, world, rank),
                                                              Mb)
    # ---- a second context at n_items = 70,000 still takes the large-universe exchange
    up_l, it_l, Ml = osm.log_70000()
    with pkg.CooccurrenceCore(n_items=Ml, device=0) as core:
        sharding.init_comm_torch_ops(core)
        out["large"], _, _ = _count(core, sharding, torch, *osm.shard(up_l, it_l, world, rank), Ml, topk=False)
    # ---- split rows on the owner
    if world == 2:
        up_s, it_s, Ms = osm.log_split()
        with pkg.CooccurrenceCore(n_items=Ms, device=0) as core:
            sharding.init_comm_torch_ops(core)
            core.set_kernel_timing(True)
            up_r, it_r = osm.shard(up_s, it_s, world, rank)
            res, info = core.count_owned(torch.from_numpy(up_r).cuda(), torch.from_numpy(it_r).cuda())
            torch.cuda.current_stream().synchronize()
            b = core.copy_batch(int(res.nnz), int(res.observed))
            out["split"] = dict(rp=b.row_ptr, cols=b.cols, cnt=b.cnt, rowsum=b.rowsum, observed=int(info.observed),
                                local_observed=int(info.local_observed), kernel_ms=core.last_kernel_ms(),
                                verify=core.verify_batch())
    with open(os.path.join(out_dir, f"rank{rank}.pkl"), "wb") as f:
        pickle.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


_SPAWNED: dict = {}


def _parts(world, tmp_path_factory):
    """the ranks' results at `world`: one spawn per world size, shared by every test of the module"""
    if world not in _SPAWNED:
        out_dir = tmp_path_factory.mktemp(f"world{world}")
        osm.spawn(_worker, (world, _free_port(), str(out_dir)), world, f"count_owned at {world} ranks")
        _SPAWNED[world] = [pickle.load(open(out_dir / f"rank{r}.pkl", "rb")) for r in range(world)]
    return _SPAWNED[world]


_WANT: dict = {}


def _want(oracle, name):
    """the closed form of a whole log, computed once"""
    if name not in _WANT:
        up, it, M = {"a": osm.log_a, "b2": lambda: osm.log_b(2), "b7": lambda: osm.log_b(7)}[name.split("-")[0]]()
        if name.endswith("-cut"):
            up, it = osm.capped(up, it, 3)
        _WANT[name] = (up, it, M, oracle.closed_form(up, it, M))
    return _WANT[name]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _assert_info(parts, world, up, it, M, key):
    lens = np.diff(up)
    for r, p in enumerate(parts):
        e = p[key]
        assert e["n_items"] == M and e["n_users_all"] == len(lens) and e["n_all"] == len(it)
        assert np.array_equal(e["owner"], np.arange(M) % world)
        assert e["observed"] == int(np.sum(lens * (lens - 1)))
        v = e["verify"]
        assert v["rows_bad_sum"] == 0 and v["rows_bad_entries"] == 0 and v["entries"] == e["nnz"] == len(e["cols"])
        assert (e["gathered"] > 0) == (world > 1)


@pytest.mark.parametrize("world", [2, 3])
def test_log_a_rows_info_and_readers(pkg, oracle, torch_cuda, tmp_path_factory, world):
    up, it, M, want = _want(oracle, "a")
    rp = want[0]
    for r in range(world):  # the log must give every rank a non-empty row, and leave some rows and users empty
        assert np.any(np.diff(rp)[r::world] > 0)
    assert np.any(np.diff(rp) == 0) and set(np.diff(up)[:4].tolist()) == {0, 1, 2}
    parts = _parts(world, tmp_path_factory)
    osm.assert_union(parts, world, want, "a")
    _assert_info(parts, world, up, it, M, "a")
    for r, p in enumerate(parts):
        assert np.array_equal(p["a_item_counts"], np.bincount(it, minlength=M)), f"rank {r}: info.item_counts"
        # two calls on the same inputs: byte-equal outputs
        for k in ("rp", "cols", "cnt", "cnt16", "rowsum"):
            assert p["a_again"][k].tobytes() == p["a"][k].tobytes(), k
        for k in ("sizes", "values", "scores", "rowsum"):
            assert p["a_again_topk"][k].tobytes() == p["a_topk"][k].tobytes(), k
        # a range that spans owned and non-owned rows: the same entries as the whole copy
        cols, cnt, cnt16, n = p["a_range"]
        sl = slice(p["a"]["rp"][RANGE[0]], p["a"]["rp"][RANGE[1]])
        assert n == sl.stop - sl.start > 0
        assert np.array_equal(cols[:n], p["a"]["cols"][sl]) and np.array_equal(cnt[:n], p["a"]["cnt"][sl])
        assert np.array_equal(cnt16[:n], p["a"]["cnt16"][sl])


@pytest.mark.parametrize("world", [2, 3])
def test_log_a_topk(pkg, oracle, torch_cuda, tmp_path_factory, world):
    up, it, M, want = _want(oracle, "a")
    rp, cols, data, rowsums, _ = want
    heaps = osm.expected_heaps(oracle, rp, cols, data, rowsums, np.flatnonzero(np.diff(rp)))
    parts = _parts(world, tmp_path_factory)
    osm.assert_heaps(parts, world, heaps, "a_topk")
    for r, p in enumerate(parts):
        assert np.array_equal(p["a_topk"]["rowsum"], rowsums), f"rank {r}: the all-reduced row sums"
        sizes, values, scores = p["a_items"]  # topk_items on owned and non-owned items
        for j, a in enumerate(MIXED):
            v, sc = heaps.get(a, ((), ())) if a % world == r else ((), ())
            assert int(sizes[j]) == len(v), f"rank {r}, item {a}"
            assert np.array_equal(values[j, :len(v)], v) and np.array_equal(scores[j, :len(v)], sc, equal_nan=True)


@pytest.mark.parametrize("world", [2, 3])
def test_host_arrays_user_cut_and_a_rank_without_users(pkg, oracle, torch_cuda, tmp_path_factory, world):
    up, it, M, want = _want(oracle, "a")
    parts = _parts(world, tmp_path_factory)
    osm.assert_union(parts, world, want, "a_host")
    for p in parts:  # winfo: nnz, the owned rows' pairs, rows with entries
        nnz = np.diff(p["a"]["rp"])
        assert p["a_host"]["winfo"] == (int(nnz.sum()), p["a"]["local_observed"], int(np.count_nonzero(nnz)))
    up_c, it_c, _, want_cut = _want(oracle, "a-cut")
    assert want_cut[4] < want[4]
    osm.assert_union(parts, world, want_cut, "cut")
    _assert_info(parts, world, up_c, it_c, M, "cut")
    osm.assert_union(parts, world, want, "c")
    _assert_info(parts, world, up, it, M, "c")
    rp, cols, data, rowsums, _ = want
    osm.assert_heaps(parts, world, osm.expected_heaps(oracle, rp, cols, data, rowsums, np.flatnonzero(np.diff(rp))),
                     "c_topk")


@pytest.mark.parametrize("M", [2, 7])
def test_fewer_rows_than_ranks(pkg, oracle, torch_cuda, tmp_path_factory, M):
    world = 3
    up, it, _, want = _want(oracle, f"b{M}")
    parts = _parts(world, tmp_path_factory)
    osm.assert_union(parts, world, want, f"b{M}")
    _assert_info(parts, world, up, it, M, f"b{M}")
    rp, cols, data, rowsums, _ = want
    assert np.all(np.diff(rp) > 0)
    if M == 2:
        assert parts[2]["b2"]["nnz"] == 0 and parts[2]["b2"]["local_observed"] == 0  # rank 2 owns no row
    osm.assert_heaps(parts, world, osm.expected_heaps(oracle, rp, cols, data, rowsums, np.arange(M)), f"b{M}_topk")


@pytest.mark.parametrize("world", [2, 3])
def test_a_large_universe_context_keeps_the_history_exchange(pkg, torch_cuda, tmp_path_factory, world):
    """n_items = 70,000 in the same processes: the frequency-snake owner map and the whole-log count, as before"""
    import torch

    up, it, M = osm.log_70000()
    parts = _parts(world, tmp_path_factory)
    dev = torch.device("cuda", 0)
    with pkg.CooccurrenceCore(n_items=M, device=0) as core:
        whole = core.count_device(torch.from_numpy(up).to(dev), torch.from_numpy(it).to(dev))
        torch.cuda.current_stream().synchronize()
        w_rp, w_cols, w_cnt, w_rowsum = _rows(whole, M)
        observed = int(whole.observed)
    owner = parts[0]["large"]["owner"]
    assert len(set(owner.tolist())) == world and not np.array_equal(owner, np.arange(M) % world)
    for r, p in enumerate(parts):
        e = p["large"]
        assert np.array_equal(e["owner"], owner) and e["observed"] == observed
        mine = owner == r
        nnz = np.diff(e["rp"])
        assert np.all(nnz[~mine] == 0) and np.array_equal(nnz[mine], np.diff(w_rp)[mine])
        assert np.array_equal(e["rowsum"][mine], w_rowsum[mine])
        for a in np.flatnonzero(mine & (nnz > 0)):
            sl, ws = slice(e["rp"][a], e["rp"][a + 1]), slice(w_rp[a], w_rp[a + 1])
            o1, o2 = np.argsort(e["cols"][sl], kind="stable"), np.argsort(w_cols[ws], kind="stable")
            assert np.array_equal(e["cols"][sl][o1], w_cols[ws][o2]) and np.array_equal(e["cnt"][sl][o1], w_cnt[ws][o2])
    assert sum(p["large"]["local_observed"] for p in parts) == observed


@pytest.mark.parametrize("world", [2, 3])
def test_an_item_out_of_range_fails_every_rank_and_the_next_call_works(pkg, oracle, torch_cuda, tmp_path_factory,
                                                                      world):
    _, _, M, want = _want(oracle, "a")
    parts = _parts(world, tmp_path_factory)
    for r, p in enumerate(parts):
        assert p["message"] is not None, f"rank {r} did not fail"
        if r == 1:  # the failing rank names the id, the others name the rank
            assert f"interaction 3: item {M} (of {M})" in p["message"]
        else:
            assert "rank 1 failed its checks" in p["message"]
        assert p["message_host"] is not None, f"rank {r} did not fail"
        assert ("user_ptr[0] must be 0" if r == 0 else "rank 0 failed its checks") in p["message_host"]
    osm.assert_union(parts, world, want, "a_after_error")
    for p in parts:
        for k in ("rp", "cols", "cnt", "rowsum"):
            assert np.array_equal(p["a_after_error"][k], p["a"][k])


def test_split_rows_on_the_owner(pkg, torch_cuda, tmp_path_factory):
    """2,200 users x the same 2,000 items of 2,003: every row holds 2,200 x 1,999 pairs, above the 2^22-pair chunk;
    every off-diagonal count among the 2,000 items is 2,200, the 3 other rows are empty"""
    world = 2
    parts = _parts(world, tmp_path_factory)
    U, K, M = osm.SPLIT_USERS, osm.SPLIT_ITEMS, osm.SPLIT_M
    assert U * (K - 1) > 1 << 22
    for r, p in enumerate(parts):
        e = p["split"]
        nnz = np.diff(e["rp"])
        mine = (np.arange(M) % world == r) & (np.arange(M) < K)
        assert np.all(nnz[mine] == K - 1) and np.all(nnz[~mine] == 0)
        assert np.all(e["rowsum"][mine] == U * (K - 1)) and np.all(e["rowsum"][~mine] == 0)
        assert np.all(e["cnt"] == U)
        cols = e["cols"].reshape(-1, K - 1)
        rows = np.flatnonzero(mine)
        full = np.arange(K)
        assert np.array_equal(cols, np.stack([full[full != a] for a in rows]))
        assert e["observed"] == U * K * (K - 1) and e["local_observed"] == len(rows) * U * (K - 1)
        assert e["kernel_ms"] > 0  # the counting kernel ran (cooc_last_kernel_ms)
        assert e["verify"]["rows_bad_sum"] == 0 and e["verify"]["rows_bad_entries"] == 0


def test_operator_replay_at_301_items(pkg, oracle, torch_cuda, tmp_path_factory):
    """the JVM operators' call sequence (test_owned_operator_replay's driver) on log A: rows in the int16 view, int32
    row sums, and every owned row's heap"""
    world = 2
    _, _, M, want = _want(oracle, "a")
    rp, cols, data, rowsums, observed = want
    parts = _parts(world, tmp_path_factory)
    heaps = osm.expected_heaps(oracle, rp, cols, data, rowsums, np.flatnonzero(np.diff(rp)))
    seen = {}
    for r, p in enumerate(parts):
        out = p["replay"]
        assert out is not None and out["timestamp"] == REPLAY_WINDOW[1] and out["job_observed"] == observed
        for a, (c, v16) in out["rows"].items():
            assert a % world == r and a not in seen
            seen[a] = r
            assert np.array_equal(c, cols[rp[a]:rp[a + 1]]) and np.array_equal(v16, osm.views(data[rp[a]:rp[a + 1]])[0])
        rs32 = osm.views(rowsums)[1]
        assert out["rowsums"] == {int(a): int(rs32[a]) for a in np.flatnonzero(rs32) if a % world == r}
        assert set(out["heaps"]) == {a for a in heaps if a % world == r}
        for a, (v, sc) in out["heaps"].items():
            assert np.array_equal(v, heaps[a][0]) and np.array_equal(sc, heaps[a][1], equal_nan=True), f"row {a}"
    assert set(seen) == set(np.flatnonzero(np.diff(rp)).tolist())
    assert sum(p["replay"]["observed"] for p in parts) == observed
