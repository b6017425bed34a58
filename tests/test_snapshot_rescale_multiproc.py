"""Rescaling across processes: a job of W_old subtasks (the harness of tests/test_streaming_multiproc.py: processes on
the box's one GPU, the communicator over gloo) streams the first half of a C1-shaped log with keyBy(user) =
user % W_old, finishes its watermark loop, takes its blobs and exits.  A job of W_new subtasks then starts, every
subtask joins the communicator and restores ALL blobs with restore_parts (the MOD route), and streams the second
half with user % W_new.  Each new subtask's snapshot right after the restore equals tests/_snapblob.py's
expected_part byte for byte; the union of the windows, before and after, equals an uninterrupted OracleStream's
window by window; the accumulators add up to the oracle's, the rescorer's total is the oracle's on every rank, and
the sampled global rows and all row sums match.  At most 3 processes hold the GPU at a time.  Needs an MI355X.
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


def _worker(rank, world, port, out_dir, kind, topk, lag, phase, w_old):
    """phase 0: the old job up to the checkpoint; phase 1: the new job from the old job's blobs to the end"""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch

    import __graft_entry__

    pkg = __graft_entry__.load_package()
    from flink_cooccurrence_amd import sharding

    torch.cuda.set_device(0)
    if world > 1:
        import torch.distributed as dist

        dist.init_process_group("gloo", rank=rank, world_size=world)
    users, items, ts, M = _records(kind)
    op = pkg.NonSampledUserInteractionCounterOneInputStreamOperator(1, "SECONDS", n_items=M, top_k=topk)
    if world > 1:
        sharding.init_comm_torch_ops(op.core)
    n_chunks = (len(users) + CHUNK - 1) // CHUNK
    half = n_chunks // 2
    out = {}
    if phase == 1:
        blobs = [open(os.path.join(out_dir, f"blob{r}.bin"), "rb").read() for r in range(w_old)]
        out["info"] = op.restore_parts(blobs)
        out["snapshot"] = op.snapshot()
        assert out["info"] == op.core.last_snapshot_info
    got = []
    for j in range(0 if phase == 0 else half, half if phase == 0 else n_chunks):
        sl = slice(j * CHUNK, (j + 1) * CHUNK)
        mine = users[sl] % world == rank  # keyBy(0)
        op.process_elements(users[sl][mine], items[sl][mine], ts[sl][mine])
        checkpoint = phase == 0 and j == half - 1
        # lag: subtask 1 receives only every third watermark -- but the one before the checkpoint reaches all
        if checkpoint or not (lag and rank == 1 and j % 3 != 2):
            got += op.process_watermark(int(ts[sl][-1]) - 1)
    if phase == 0:  # every loop returned fired = 0: the same windows are finished on every subtask
        with open(os.path.join(out_dir, f"blob{rank}.bin"), "wb") as f:
            f.write(op.snapshot())
        out["info"] = op.core.last_snapshot_info
    else:
        got += op.process_watermark(INT64_MAX)
        out.update(acc=op.accumulators(), rowsums=op.core.global_rowsums(),
                   rows={a: op.core.global_row(a) for a in range(rank, M, world * 7)})
    out["windows"] = got
    op.close()
    with open(os.path.join(out_dir, f"phase{phase}_rank{rank}.pkl"), "wb") as f:
        pickle.dump(out, f)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.parametrize("w_old,w_new,kind,lag", [(2, 3, "c1", False), (3, 2, "c1", False), (1, 2, "c1", False),
                                                  (2, 3, "slabs", False), (2, 3, "c1", True)])
def test_rescale_and_resume(pkg, oracle, torch_cuda, tmp_path, w_old, w_new, kind, lag):
    import torch.multiprocessing as mp

    from tests import _snapblob as sb
    from tests._helpers import assert_windows_equal

    topk = 10
    assert max(w_old, w_new) <= 3
    mp.spawn(_worker, args=(w_old, _free_port(), str(tmp_path), kind, topk, lag, 0, w_old), nprocs=w_old, join=True)
    blobs = [open(tmp_path / f"blob{r}.bin", "rb").read() for r in range(w_old)]
    mp.spawn(_worker, args=(w_new, _free_port(), str(tmp_path), kind, topk, lag, 1, w_old), nprocs=w_new, join=True)
    old = [pickle.load(open(tmp_path / f"phase0_rank{r}.pkl", "rb")) for r in range(w_old)]
    new = [pickle.load(open(tmp_path / f"phase1_rank{r}.pkl", "rb")) for r in range(w_new)]
    # the blobs of the old job are the parts the issue describes
    for r, p in enumerate(old):
        assert (p["info"]["rank"], p["info"]["world"]) == (r, w_old)
        assert p["info"]["n_users"] > 0 and p["info"]["global_rows"] > 0 and p["info"]["pending_records"] > 0
    # every new rank right after the restore: expected_part, byte for byte
    for r, p in enumerate(new):
        want = sb.expected_part(blobs, r, w_new, sb.keep_mod(w_new, r))
        assert p["snapshot"] == want, f"new rank {r}"
        assert p["info"] == pkg.CooccurrenceCore.snapshot_info(want)
    assert sum(p["info"]["n_users"] for p in new) == sum(p["info"]["n_users"] for p in old)
    assert sum(p["info"]["history_items"] for p in new) == sum(p["info"]["history_items"] for p in old)
    # the windows of both jobs against the uninterrupted oracle
    users, items, ts, M = _records(kind)
    ref = oracle.OracleStream(1000, topk=topk)
    want = []
    for lo in range(0, len(users), CHUNK):
        sl = slice(lo, lo + CHUNK)
        ref.process_elements(users[sl], items[sl], ts[sl])
        want += ref.process_watermark(int(ts[sl][-1]) - 1)
    want += ref.process_watermark(INT64_MAX)
    n_old = {len(p["windows"]) for p in old}
    n_new = {len(p["windows"]) for p in new}
    assert len(n_old) == len(n_new) == 1, (n_old, n_new)
    n_old, n_new = n_old.pop(), n_new.pop()
    assert n_old >= 5 and n_new >= 5 and n_old + n_new == len(want) >= 20, (n_old, n_new, len(want))
    for i, w in enumerate(want):
        job, k = (old, i) if i < n_old else (new, i - n_old)
        assert_windows_equal(_union([p["windows"][k] for p in job]), w)
    want_acc = ref.counters()
    acc = {k: sum(p["acc"][k] for p in new) for k in new[0]["acc"] if k != "rescorer_observed"}
    assert acc == {k: v for k, v in want_acc.items() if k != "rescorer_observed"}
    assert all(p["acc"]["rescorer_observed"] == want_acc["rescorer_observed"] for p in new)
    gi, gv32, gex = ref.global_rowsums()
    for p in new:
        ex, v32 = p["rowsums"]
        assert np.array_equal(ex[gi], gex) and np.array_equal(v32[gi], gv32)
    rows, rp, cols, exact, v16 = ref.global_rows()
    pos = {int(a): r for r, a in enumerate(rows)}
    for p in new:
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
