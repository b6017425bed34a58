"""Checkpoint and restore across GPUs: p = 2 subtasks of the streaming operator (the harness of
tests/test_streaming_multiproc.py: two processes on the box's one GPU, the communicator over gloo through
sharding.init_comm_torch_ops).  After the chunk nearest the middle of the stream both subtasks finish their
watermark loop -- so both have finished the same windows -- take their blobs, close their operators, create new
ones, join the communicator and restore, each from its own blob, then continue.  The union of the two subtasks'
windows (before and after the restore) equals an uninterrupted OracleStream's window by window, and the
accumulators add up; rank 0's blob on rank 1 is refused.  A C1-shaped log at M = 300 (the owners' rows in the dense
matrix) and at M = 40,500 (row slabs), and once with different watermark sequences on the two subtasks.
Needs an MI355X.
"""
import os
import pickle
import sys

import numpy as np
import pytest

from tests.test_streaming_multiproc import CHUNK, INT64_MAX, ROOT, _free_port, _union

pytestmark = pytest.mark.gpu


def _records(kind):
    sys.path.insert(0, ROOT)
    import __graft_entry__

    __graft_entry__.load_package()
    from flink_cooccurrence_amd import datagen

    M = 300 if kind == "c1" else 40_500
    d = datagen.config_c1(seed=1 if kind == "c1" else 5, U=2000, M=M, mean=20.0)
    users, items, ts = datagen.to_records(d["user_ptr"], d["items"], d["ts"])
    return users, items, ts, M


def _worker(rank, world, port, out_dir, kind, topk, lag):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist

    import __graft_entry__

    pkg = __graft_entry__.load_package()
    from flink_cooccurrence_amd import sharding

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    users, items, ts, M = _records(kind)

    def new_operator():
        op = pkg.NonSampledUserInteractionCounterOneInputStreamOperator(1, "SECONDS", n_items=M, top_k=topk)
        sharding.init_comm_torch_ops(op.core)  # (a restore checks the blob's rank and world against it)
        return op

    op = new_operator()
    n_chunks = (len(users) + CHUNK - 1) // CHUNK
    got, info, foreign = [], None, None
    for j, lo in enumerate(range(0, len(users), CHUNK)):
        sl = slice(lo, lo + CHUNK)
        mine = users[sl] % world == rank  # keyBy(0)
        op.process_elements(users[sl][mine], items[sl][mine], ts[sl][mine])
        checkpoint = j == n_chunks // 2 - 1
        # lag: subtask 1 receives only every third watermark -- but the one before the checkpoint reaches both
        if checkpoint or not (lag and rank == 1 and j % 3 != 2):
            got += op.process_watermark(int(ts[sl][-1]) - 1)
        if checkpoint:  # both loops returned fired = 0: the same windows are finished on both subtasks
            blob = op.snapshot()
            info = op.core.last_snapshot_info
            op.close()
            with open(os.path.join(out_dir, f"blob{rank}.bin"), "wb") as f:
                f.write(blob)
            dist.barrier()
            op = new_operator()
            if rank == 1:
                other = open(os.path.join(out_dir, "blob0.bin"), "rb").read()
                try:
                    op.restore(other)
                    foreign = "accepted"
                except pkg.IllegalArgumentException as e:
                    foreign = e.status
            assert op.restore(blob) == info
            assert op.snapshot() == blob
    got += op.process_watermark(INT64_MAX)
    out = dict(windows=got, acc=op.accumulators(), rowsums=op.core.global_rowsums(), info=info, foreign=foreign,
               rows={a: op.core.global_row(a) for a in range(rank, M, world * 7)})
    op.close()
    with open(os.path.join(out_dir, f"rank{rank}.pkl"), "wb") as f:
        pickle.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("kind,lag", [("c1", False), ("slabs", False), ("c1", True)])
def test_two_subtasks_checkpoint_and_resume(pkg, oracle, torch_cuda, tmp_path, kind, lag):
    import torch.multiprocessing as mp

    from tests._helpers import assert_windows_equal

    world, topk = 2, 10
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), kind, topk, lag), nprocs=world, join=True)
    parts = [pickle.load(open(tmp_path / f"rank{r}.pkl", "rb")) for r in range(world)]
    users, items, ts, M = _records(kind)
    ref = oracle.OracleStream(1000, topk=topk)
    want = []
    for lo in range(0, len(users), CHUNK):
        sl = slice(lo, lo + CHUNK)
        ref.process_elements(users[sl], items[sl], ts[sl])
        want += ref.process_watermark(int(ts[sl][-1]) - 1)
    want += ref.process_watermark(INT64_MAX)
    for r, p in enumerate(parts):
        assert (p["info"]["rank"], p["info"]["world"]) == (r, world)
        assert p["info"]["n_users"] > 0 and p["info"]["global_rows"] > 0 and p["info"]["pending_records"] > 0
    assert parts[1]["foreign"] == 1  # COOC_ERR_ARG: rank 0's blob on rank 1
    n = [len(p["windows"]) for p in parts]
    assert n[0] == n[1] == len(want) >= 20, (n, len(want))
    for i, w in enumerate(want):
        assert_windows_equal(_union([p["windows"][i] for p in parts]), w)
    want_acc = ref.counters()
    acc = {k: sum(p["acc"][k] for p in parts) for k in parts[0]["acc"] if k != "rescorer_observed"}
    assert acc == {k: v for k, v in want_acc.items() if k != "rescorer_observed"}
    assert all(p["acc"]["rescorer_observed"] == want_acc["rescorer_observed"] for p in parts)
    gi, gv32, gex = ref.global_rowsums()
    for p in parts:
        ex, v32 = p["rowsums"]
        assert np.array_equal(ex[gi], gex) and np.array_equal(v32[gi], gv32)
    rows, rp, cols, exact, v16 = ref.global_rows()
    pos = {int(a): r for r, a in enumerate(rows)}
    for p in parts:
        for a, (c, x, x16) in p["rows"].items():
            r = pos.get(a)
            if r is None:
                assert len(c) == 0
                continue
            assert np.array_equal(c, cols[rp[r]:rp[r + 1]]) and np.array_equal(x.astype(np.int64), exact[rp[r]:rp[r + 1]])


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch
