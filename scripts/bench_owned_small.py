#!/usr/bin/env python3
"""One-GPU cost of the small-universe owned window (cooc_count_owned / cooc_topk_owned below 40,320 items) next
to the single-GPU calls it extends, on datagen's C2 log.

A world-1 communicator over operations that only copy this rank's buffers to themselves runs the whole records
exchange (plan, agreement, arena all-gather, row counts and descriptors to their owner, owner count, expansion), so
the figures are the exchange's fixed work on one GPU, not a p > 1 time: no transfer crosses a link here.  The calls
alternate -- cooc_count_device, cooc_count_owned, cooc_topk_batch_device, cooc_topk_owned -- one warm-up round, then
--steps timed rounds, the host clock around calls that end in a synchronise.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def self_copy_ops(_lib):
    """cooc_comm_ops of a one-rank world, on the stream given"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]

    def copy(dst, src, n, stream):
        return hip.hipMemcpyAsync(dst, src, n, 3, stream) if n else 0

    def allreduce(_user, _buf, _n, _stream):
        return 0

    def allgather(_user, d_send, d_recv, nbytes, stream):
        return copy(d_recv, d_send, nbytes, stream)

    def alltoallv(_user, d_send, send_off, send_bytes, d_recv, recv_off, _recv_bytes, stream):
        return copy((d_recv or 0) + recv_off[0], (d_send or 0) + send_off[0], send_bytes[0], stream)

    return _lib.CoocCommOps(_lib.ALLREDUCE_FN(allreduce), _lib.ALLGATHER_FN(allgather), _lib.ALLTOALLV_FN(alltoallv))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--topk", type=int, default=10)
    args = ap.parse_args()
    import torch

    import __graft_entry__

    pkg = __graft_entry__.load_package()
    from flink_cooccurrence_amd import _lib, datagen

    d = datagen.config_c2(seed=2)
    up_h, it_h, M = d["user_ptr"], d["items"], d["n_items"]
    dev = torch.device("cuda", 0)
    up, it = torch.from_numpy(up_h).to(dev), torch.from_numpy(it_h).to(dev)
    sizes = torch.empty(M, dtype=torch.int32, device=dev)
    vals = torch.empty((M, args.topk), dtype=torch.int32, device=dev)
    scores = torch.empty((M, args.topk), dtype=torch.float64, device=dev)
    # the single-GPU calls keep their own choice of layout (dense at C2 density) and, for the like-for-like line, the
    # padded CSR the owned window always returns
    single = pkg.CooccurrenceCore(n_items=M, device=0)
    single_csr = pkg.CooccurrenceCore(n_items=M, device=0, output="csr")
    owned = pkg.CooccurrenceCore(n_items=M, device=0)
    owned.comm_init_ops(0, 1, self_copy_ops(_lib))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def topk_owned():
        owned.topk_owned(args.topk, sizes, vals, scores)

    calls = {
        "count_device": lambda: single.count_device(up, it),
        "count_device_csr": lambda: single_csr.count_device(up, it),
        "count_owned": lambda: owned.count_owned(up, it),
        "topk_batch_device": lambda: single.topk_batch_device(args.topk, sizes, vals, scores),
        "topk_batch_device_csr": lambda: single_csr.topk_batch_device(args.topk, sizes, vals, scores),
        "topk_owned": topk_owned,
    }
    ms = {k: [] for k in calls}
    observed = {}
    for step in range(args.steps + 1):  # round 0 is the warm-up
        for name, fn in calls.items():
            t, out = timed(fn)
            if step:
                ms[name].append(round(t, 3))
            if name == "count_device":
                observed[name] = int(out.observed)
            if name == "count_owned":
                observed[name] = int(out[1].observed)
    assert observed["count_owned"] == observed["count_device"] == datagen.ordered_pairs(up_h)
    print(json.dumps({"config": "c2", "n_items": M, "n_users": len(up_h) - 1, "n_interactions": len(it_h),
                      "ordered_pairs": observed["count_device"], "topk": args.topk, "world": 1,
                      "device": torch.cuda.get_device_name(0), "ms": ms}))
    for c in (single, single_csr, owned):
        c.close()


if __name__ == "__main__":
    main()
