"""The sampled mode across GPUs: p = 2 and p = 3 subtasks, each holding the keyBy(user) shard of a window's records
(user u on subtask u mod p), its users' reservoirs and totals and a replica of the item counters.  The contract
(include/cooc.h, "sampled mode at world > 1"): a window's arrival order is R_0 || R_1 || ... (rank-major), so the
union of the subtasks' outputs and state equals, bit for bit, a single sampled context fed each window in that
order -- and tests/_sampled_model.SampledModel fed the same.

Processes on the box's one GPU, the communicator over gloo (cooc_comm_ops), the dictated log of
tests/_sampled_comm.py (8 windows, about 1,900 records, 130 users), which reaches every branch of the multi-rank
window -- checked from the model's run before anything is compared: the item cut falling inside a higher rank's
records, a rejection caused by lower ranks alone, a counter committed on a rank that saw no record of the item, a
feedback crossing ranks, a rank without records, a window that changes no slot, a minus run on one rank only, a key
whose nets cancel across ranks.  Both decision modes; dense rows, row slabs and a 1e6-item universe; one case
through the operator mirror with different watermark sequences on the subtasks.  Needs an MI355X."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (at collection, before any test opens the GPU through the library: torch.cuda finds it)

import _sampled_comm as sc
import _sampled_model as sm
from test_gpu_sampled import _check_window
from test_gpu_sampled_device_mode import _same_window
from test_streaming_multiproc import _free_port, _union

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
INT64_MAX = (1 << 63) - 1
TOPK = 5


def _arrays(recs):
    return np.array([u for u, _ in recs], np.int32), np.array([i for _, i in recs], np.int32)


def _submit(core, wi, recs):
    """one window by submit_batch / finish_window; one CSR row per record keeps any arrival order"""
    users, items = _arrays(recs)
    ts = wi * 1000 + 999
    if len(recs):
        core.submit_batch(ts, users, np.arange(len(recs) + 1, dtype=np.int64), items)
    return core.finish_window(ts)


def _worker(rank, world, port, out_dir, n_items, planner, on, via_operator):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    for p in (ROOT, TESTS):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist

    import __graft_entry__

    pkg = __graft_entry__.load_package()
    from flink_cooccurrence_amd import sharding

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    windows, _ = sc.dictated_log(world, n_items)
    core = pkg.CooccurrenceCore(n_items=n_items, topk=TOPK, user_cut=sc.USER_CUT, planner=planner)
    sharding.init_comm_torch_ops(core)  # the order: join, then enable
    core.sampling_enable(sc.ITEM_CUT, sc.SEED, on=on)
    got, runs = [], []
    for wi, per_rank in enumerate(windows):
        if not via_operator:
            got.append(_submit(core, wi, per_rank[rank]))
            runs.append(core.last_window_runs())
            continue
        users, items = _arrays(per_rank[rank])
        assert core.op_process_elements(users, items, np.full(len(users), wi * 1000 + 1, np.int64)) == 0
        # subtask 1 receives only every third watermark: the windows still fire together, in order
        if not (rank == 1 and wi % 3 != 2):
            got += core.op_process_watermark(wi * 1000 + 999)
    if via_operator:
        got += core.op_process_watermark(INT64_MAX)
    mine = sorted({u for w in windows for u, _ in w[rank]})
    log_items = sorted({i for w in windows for R in w for _, i in R})
    out = dict(windows=got, runs=runs, counters=core.sampling_counters(), acc=core.op_counters(),
               observed=core.global_observed(), rowsums=core.global_rowsums(),
               users={u: core.user_history(u) for u in mine},
               rows={a: core.global_row(a) for a in log_items + [1, n_items - 2]})
    core.close()
    with open(os.path.join(out_dir, f"rank{rank}.pkl"), "wb") as f:
        pickle.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


CASES = [  # world, n_items, planner, decided on, through the operator mirror
    pytest.param(2, 300, "auto", "device", False, id="p2-dense-device"),
    pytest.param(3, 300, "auto", "device", False, id="p3-dense-device"),
    pytest.param(3, 300, "auto", "host", False, id="p3-dense-host"),
    pytest.param(2, 40_500, "auto", "device", False, id="p2-slabs-device"),
    pytest.param(3, 40_500, "auto", "host", False, id="p3-slabs-host"),
    pytest.param(3, 1_000_000, "auto", "device", False, id="p3-1e6-device"),
    pytest.param(2, 1_000_000, "auto", "host", False, id="p2-1e6-host"),
    pytest.param(2, 300, "general", "device", True, id="p2-operator-lag-device"),
]


@pytest.mark.parametrize("world,n_items,planner,on,via_operator", CASES)
def test_subtasks_equal_the_serialised_single_context(pkg, oracle, torch_cuda, tmp_path, world, n_items, planner, on,
                                                      via_operator):
    import torch.multiprocessing as mp

    windows, marks = sc.dictated_log(world, n_items)
    # the log must reach the new branches: from the model's run, before anything of the library is looked at
    got, _, _ = sc.reached(world, windows, n_items, marks)
    assert got == set(sc.BRANCHES), f"the log no longer reaches {sorted(set(sc.BRANCHES) - got)}"

    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), n_items, planner, on, via_operator), nprocs=world,
             join=True)
    parts = [pickle.load(open(tmp_path / f"rank{r}.pkl", "rb")) for r in range(world)]
    assert all(len(p["windows"]) == len(windows) for p in parts), [len(p["windows"]) for p in parts]

    model = sm.SampledModel(n_items, sc.ITEM_CUT, sc.USER_CUT, sc.SEED)
    read = [0, n_items - 1, marks["x"], marks["y"]]
    with pkg.CooccurrenceCore(n_items=n_items, topk=TOPK, user_cut=sc.USER_CUT, item_cut=sc.ITEM_CUT,
                              sample_seed=sc.SEED, planner=planner) as single:
        for wi, per_rank in enumerate(windows):
            recs = sc.serial(per_rank)
            want = _submit(single, wi, recs)
            len_before = {u: len(model.H.get(u, [])) for u, _ in recs}
            mw = model.window(recs)
            # oracle 2, then oracle 1 (the single context against the model: rows, cnt16, row sums, heaps, state)
            union = _union([p["windows"][wi] for p in parts])
            if mw.delta:
                _same_window(union, want)
            else:  # (f): an empty window on every rank, though the counters moved
                assert len(want.rows) == len(want.topk_rows) == 0 and want.observed == 0
                assert all(len(p["windows"][wi].rows) == len(p["windows"][wi].rs_items) == 0 and
                           len(p["windows"][wi].topk_rows) == 0 and p["windows"][wi].observed == 0 for p in parts)
            _check_window(single, model, want, mw, oracle, TOPK, rows_to_read=read)
            rows = mw.rows()
            assert {int(a): dict(zip(union.cols[s:e].tolist(), union.exact[s:e].tolist()))
                    for a, s, e in zip(union.rows, union.row_ptr[:-1], union.row_ptr[1:])} == rows
            assert union.rs_exact.tolist() == [mw.rowsum[a] for a in sorted(rows)]
            for r, p in enumerate(parts):  # each row on its owner
                assert all(int(a) % world == r for a in p["windows"][wi].rows)
                assert all(int(a) % world == r for a in p["windows"][wi].topk_rows)
            if not via_operator:  # the rank's own counting runs: 0 no slot changed here, 2 with a minus run (a
                                  # replaced slot that existed before the window)
                by_rank = _decisions_by_rank(mw, per_rank)
                minus = [any(d[0] == "k" and int(d[1:]) < len_before[u] for (u, _), d in zip(R, ds))
                         for R, ds in zip(per_rank, by_rank)]
                changed = [any(d[0] in "fk" for d in ds) for ds in by_rank]
                assert [p["runs"][wi] for p in parts] == [2 if m else 1 if c else 0 for m, c in zip(minus, changed)]
            if wi == marks["window"]:  # (h): the key whose nets cancel across ranks, with count 0, its row rescored
                x, y = marks["x"], marks["y"]
                owner = parts[x % world]["windows"][wi]
                r = owner.rows.tolist().index(x)
                cols = owner.cols[owner.row_ptr[r]:owner.row_ptr[r + 1]].tolist()
                assert owner.exact[owner.row_ptr[r] + cols.index(y)] == 0
                assert x in owner.topk_rows.tolist() and x in owner.rs_items.tolist()
        # ---- the state at the end
        want_ctr = single.sampling_counters()
        assert want_ctr == model.counters()
        for k in ("item_cut_rejections", "fills", "replacements", "feedbacks", "users"):
            assert sum(p["counters"][k] for p in parts) == want_ctr[k], k
        # the item counters are replicated: the job's sum on every rank
        assert all(p["counters"]["item_counter_sum"] == want_ctr["item_counter_sum"] for p in parts)
        for r, p in enumerate(parts):
            assert set(p["users"]) == {u for u in model.total if u % world == r}
            for u, (items, total) in p["users"].items():
                assert items.tolist() == model.H.get(u, []) and total == model.total[u], f"user {u}"
                si, st = single.user_history(u)
                assert np.array_equal(items, si) and total == st
        want_acc = single.op_counters()
        for k in want_acc:
            if k == "rescorer_observed":  # the job's on every subtask: it scores against the broadcast row sums
                assert all(p["acc"][k] == want_acc[k] for p in parts)
            else:
                assert sum(p["acc"][k] for p in parts) == want_acc[k], k
        ex, v32 = single.global_rowsums()
        grows = model.global_rows()
        for r, p in enumerate(parts):
            assert np.array_equal(p["rowsums"][0], ex) and np.array_equal(p["rowsums"][1], v32)
            assert p["observed"][1] == single.global_observed()[1]
            for a, (cols, cnt, cnt16) in p["rows"].items():
                want_row = grows.get(a, {}) if a % world == r else {}  # each row on its owner only
                assert dict(zip(cols.tolist(), cnt.tolist())) == want_row, f"global row {a} on rank {r}"
                assert cnt16.tolist() == [sm.i16(v) for v in want_row.values()]
                if a % world == r:
                    sc_, sn, s16 = single.global_row(a)
                    assert np.array_equal(cols, sc_) and np.array_equal(cnt, sn) and np.array_equal(cnt16, s16)
        assert sum(p["observed"][0] for p in parts) == single.global_observed()[0]


def _decisions_by_rank(mw, per_rank):
    """the model's decisions of a serialised window, rank by rank"""
    out, at = [], 0
    for R in per_rank:
        out.append(mw.decisions[at:at + len(R)])
        at += len(R)
    return out


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch
