"""The sampled pipeline across ranks at the universe where the cuts matter: n_items = 300, item_cut 20, user_cut 4,
seed 0xC0FFEE, the wide log of tests/_sample_owned.py, 2 processes on the box's one GPU with the communicator over
gloo.  sharding.sample_owned -> count_owned -> topk_owned: cooc_sample_owned's reservoirs are "a valid input of
cooc_count_owned" (include/cooc.h) below 40,320 items too, where the count is the records exchange (row a on rank
a mod 2).  The union of the ranks' rows and heaps equals one process running sample_device -> count_device ->
topk_batch over the serialised log.  Mirrors test_sample_owned_multiproc's 70,000-item end-to-end test.  Needs an
MI355X."""
import datetime
import os
import pickle
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (at collection, before any test opens the GPU through the library: torch.cuda finds it)

import _owned_small as osm
import _sample_owned as so
from test_multiproc_gpu import _free_port, _rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
WORLD, N_ITEMS, ITEM_CUT, USER_CUT, SEED, TOPK = 2, 300, 20, 4, 0xC0FFEE, 5


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    for p in (ROOT, TESTS):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist

    import __graft_entry__

    pkg = __graft_entry__.load_package()
    from flink_cooccurrence_amd import sharding

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    users, items, keys, wp = so.shard(so.wide_log(world), rank)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    with pkg.CooccurrenceCore(n_items=N_ITEMS, device=0) as core:
        sharding.init_comm_torch_ops(core)
        res_ptr, res_items, _, _, info = sharding.sample_owned(core, to(users), to(items), len(keys), to(keys), ITEM_CUT,
                                                               USER_CUT, seed=SEED, window_ptr=wp)
        res = sharding.count_owned(core, res_ptr, res_items)
        torch.cuda.current_stream().synchronize()
        rp, cols, cnt, rowsum = _rows(res.owned, N_ITEMS)
        tk = sharding.topk_owned(core, res, TOPK)
        torch.cuda.current_stream().synchronize()
        out = dict(rp=rp, cols=cols, cnt=cnt, rowsum=rowsum, owner=res.owner.cpu().numpy(), observed=int(res.observed),
                   local_observed=int(res.local_observed), sizes=tk.sizes.cpu().numpy(), values=tk.values.cpu().numpy(),
                   scores=tk.scores.cpu().numpy(), tk_rowsum=tk.rowsum.cpu().numpy(), info=info)
    with open(os.path.join(out_dir, f"rank{rank}.pkl"), "wb") as f:
        pickle.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def test_sample_count_topk_at_300_items(pkg, torch_cuda, tmp_path):
    import torch

    osm.spawn(_worker, (WORLD, _free_port(), str(tmp_path)), WORLD, "sample_owned -> count_owned at 300 items")
    parts = [pickle.load(open(tmp_path / f"rank{r}.pkl", "rb")) for r in range(WORLD)]
    users, items, wp = so.serial_log(so.wide_log(WORLD))
    dev = torch.device("cuda:0")
    M = N_ITEMS
    with pkg.CooccurrenceCore(n_items=M, device=0, output="csr") as core:
        res_ptr, res_items, _, _, s_info = core.sample_device(torch.from_numpy(users).to(dev),
                                                              torch.from_numpy(items).to(dev), int(users.max()) + 1,
                                                              ITEM_CUT, USER_CUT, seed=SEED, window_ptr=wp)
        whole = core.count_device(res_ptr, res_items)
        torch.cuda.current_stream().synchronize()
        w_rp, w_cols, w_cnt, w_rowsum = _rows(whole, M)
        observed = int(whole.observed)
        w_sz, w_v, w_sc = core.topk_batch(TOPK)
    # the cuts matter here: records were rejected by the item cut and reservoirs replaced or fed back
    assert s_info["rejected"] > 0 and s_info["replacements"] + s_info["feedbacks"] > 0
    assert sum(p["info"]["rejected"] for p in parts) == s_info["rejected"]
    assert observed > 0 and int(w_rowsum.sum()) == observed
    w_nnz = np.diff(w_rp)
    for r, p in enumerate(parts):
        mine = np.arange(M) % WORLD == r
        assert np.array_equal(p["owner"], np.arange(M) % WORLD) and p["observed"] == observed
        nnz = np.diff(p["rp"])
        assert np.all(nnz[~mine] == 0) and np.array_equal(nnz[mine], w_nnz[mine]) and np.any(nnz > 0)
        assert np.array_equal(p["rowsum"][mine], w_rowsum[mine]) and np.array_equal(p["tk_rowsum"], w_rowsum)
        for a in np.flatnonzero(mine & (w_nnz > 0)):
            sl, ws = slice(p["rp"][a], p["rp"][a + 1]), slice(w_rp[a], w_rp[a + 1])
            assert np.array_equal(p["cols"][sl], w_cols[ws]) and np.array_equal(p["cnt"][sl], w_cnt[ws]), f"row {a}"
        assert np.all(p["sizes"][~mine] == 0) and np.array_equal(p["sizes"][mine], w_sz[mine])
        for a in np.flatnonzero(mine & (w_sz > 0)):
            n = int(w_sz[a])
            assert np.array_equal(p["values"][a, :n], w_v[a, :n]), f"row {a}"
            assert np.array_equal(p["scores"][a, :n], w_sc[a, :n], equal_nan=True), f"row {a}"
    assert sum(p["local_observed"] for p in parts) == observed
