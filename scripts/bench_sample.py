#!/usr/bin/env python3
"""The device-side sampler (cooc_sample_device) on the C4 log: 138,493 users, 20,000,263 records, 26,744 items,
cuts 500 / 500.

The log's records in the arrival order of scripts/bench_stream.py (window after window, users ascending, a user's
records by time) are uploaded once; the sampler then runs over them as --windows windows and as one window, and
the same log goes through the sampled streaming mode (the host sampler, cooc_submit_batch + cooc_finish_window)
beside it.  The streaming figure is whole-window time and includes the counting; the device figure is the sampling
stage alone.  With the same seed both make the same decisions, so their counters are compared as well.

--owned times cooc_sample_owned on a context with a world-1 communicator beside cooc_sample_device on a plain one
instead: the same windowed log, one job, the two alternating, --repeats timed calls each.  At world 1 both run the
same launches; the p > 1 exchange is not timed here.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=100)
    ap.add_argument("--users", type=int, default=138_493)
    ap.add_argument("--item-cut", type=int, default=500)
    ap.add_argument("--user-cut", type=int, default=500)
    ap.add_argument("--seed", type=lambda v: int(v, 0), default=0xC0FFEE)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-stream", action="store_true", help="skip the streaming sampled mode")
    ap.add_argument("--count", action="store_true", help="also count the pairs over the final reservoirs")
    ap.add_argument("--owned", action="store_true",
                    help="time cooc_sample_owned on a world-1 communicator beside cooc_sample_device: one job, "
                         "alternating, --repeats runs each (nothing else is run)")
    args = ap.parse_args()

    import torch

    import __graft_entry__

    pkg = __graft_entry__.load_package()
    from flink_cooccurrence_amd import datagen

    torch.cuda.init()
    t0 = time.time()
    if args.users == 138_493:
        d = datagen.config_c4(n_windows=args.windows)
    else:  # reduced log (same shape) for quick runs
        d = datagen.config_c2(U=args.users, N=int(20_000_263 * args.users / 138_493))
        rng = np.random.Generator(np.random.PCG64(4))
        d["ts"] = datagen.spread_over_windows(rng, d["user_ptr"], args.windows, 1000)
    up, it, ts, M = d["user_ptr"], d["items"], d["ts"], d["n_items"]
    lens = np.diff(up)
    n_users, n = len(lens), int(up[-1])
    owner = np.repeat(np.arange(n_users, dtype=np.int32), lens)
    win = ts // 1000
    order = np.lexsort((ts, owner, win))
    u_sorted, i_sorted = owner[order].astype(np.int32), it[order].astype(np.int32)
    bounds = np.searchsorted(win[order], np.arange(args.windows + 1)).astype(np.int64)
    gen_s = time.time() - t0

    dev = torch.device("cuda:0")
    d_users, d_items = torch.from_numpy(u_sorted).to(dev), torch.from_numpy(i_sorted).to(dev)
    out = {"config": "C4 log through cooc_sample_device (seed 4 log, arrival order of bench_stream.py)",
           "users": n_users, "records": n, "n_items": M, "item_cut": args.item_cut, "user_cut": args.user_cut,
           "seed": args.seed, "datagen_s": gen_s}
    if args.owned:
        from flink_cooccurrence_amd import _lib

        # a world-1 communicator whose collectives fail if called: at world 1 the call makes none
        ops = _lib.CoocCommOps(_lib.ALLREDUCE_FN(lambda *a: 1), _lib.ALLGATHER_FN(lambda *a: 1),
                               _lib.ALLTOALLV_FN(lambda *a: 1))
        with pkg.CooccurrenceCore(n_items=M, device=0) as plain, pkg.CooccurrenceCore(n_items=M, device=0) as joined:
            joined.comm_init_ops(0, 1, ops)
            calls = {"sample_device": lambda: plain.sample_device(d_users, d_items, n_users, args.item_cut,
                                                                  args.user_cut, seed=args.seed, window_ptr=bounds),
                     "sample_owned": lambda: joined.sample_owned(d_users, d_items, n_users, None, args.item_cut,
                                                                 args.user_cut, seed=args.seed, window_ptr=bounds)}
            secs = {k: [] for k in calls}
            infos = {}
            for r in range(args.repeats + 1):  # the first call of each sizes the scratch
                for k, fn in calls.items():
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    res = fn()
                    secs[k].append(time.perf_counter() - t1)
                    infos[k] = res[4]
                    del res
        for k, s in secs.items():
            best = float(np.median(s[1:]))
            out[k] = {"n_windows": args.windows, "call_ms": [round(v * 1e3, 3) for v in s], "median_ms": best * 1e3,
                      "ms_per_window": best * 1e3 / args.windows, "records_per_s": n / best, "info": infos[k]}
        out["config"] = "C4 log: cooc_sample_owned on a world-1 communicator beside cooc_sample_device, alternating"
        out["infos_equal"] = infos["sample_device"] == infos["sample_owned"]
        print(json.dumps(out), flush=True)
        return
    with pkg.CooccurrenceCore(n_items=M, device=0) as core:
        for name, wp, n_w in (("windows", bounds, args.windows), ("one_window", None, 1)):
            secs = []
            for r in range(args.repeats + 1):  # the first call sizes the scratch
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                res = core.sample_device(d_users, d_items, n_users, args.item_cut, args.user_cut, seed=args.seed,
                                         window_ptr=wp)
                secs.append(time.perf_counter() - t1)
            best = float(np.median(secs[1:]))
            out[name] = {"n_windows": n_w, "call_ms": [round(s * 1e3, 3) for s in secs], "median_ms": best * 1e3,
                         "ms_per_window": best * 1e3 / n_w, "records_per_s": n / best, "info": res[4]}
            if name == "windows":
                windows_info = res[4]
                if args.count:
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    cres = core.count_device(res[0], res[1])
                    torch.cuda.synchronize()
                    out["count_over_reservoirs"] = {"ms": (time.perf_counter() - t1) * 1e3,
                                                    "ordered_pairs": int(cres.observed), "nnz": int(cres.nnz)}
            del res

    if not args.no_stream:
        batches = []
        for w in range(args.windows):
            s, e = int(bounds[w]), int(bounds[w + 1])
            uu = u_sorted[s:e]
            starts = np.concatenate([[0], np.nonzero(np.diff(uu))[0] + 1]) if e > s else np.zeros(0, np.int64)
            user_ptr = np.concatenate([starts, [e - s]]).astype(np.int64)
            batches.append((w * 1000 + 999, uu[starts].astype(np.int32), user_ptr, i_sorted[s:e]))
        with pkg.CooccurrenceCore(n_items=M, window_size_ms=1000, device=0, user_cut=args.user_cut,
                                  item_cut=args.item_cut, sample_seed=args.seed) as core:
            lat = []
            for ts_w, uid, uptr, items in batches:
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                core.submit_batch(ts_w, uid, uptr, items)
                core.finish_window_info(ts_w)
                lat.append(time.perf_counter() - t1)
            c = core.sampling_counters()
        lat_ms = np.array(lat) * 1e3
        out["streaming_sampled_mode"] = {
            "what": "whole windows (host sampler + counting), as bench_stream.py --item-cut --user-cut",
            "window_ms_median": float(np.median(lat_ms)), "window_ms_mean": float(lat_ms.mean()),
            "total_s": float(np.sum(lat)), "records_per_s": n / float(np.sum(lat)), "sampling_counters": c}
        out["counters_equal_streaming"] = [c[k] for k in ("item_cut_rejections", "fills", "replacements", "feedbacks",
                                                          "users", "item_counter_sum")] == \
            [windows_info[k] for k in ("rejected", "fills", "replacements", "feedbacks", "users", "item_counter_sum")]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
