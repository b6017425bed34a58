#!/usr/bin/env python3
"""Device ingest on the C4 log: 20,000,263 "user,item,timestamp" lines from bytes to the CSR and the windowed records.

The log is the C2-shaped one `bench.py --config c4` streams (datagen.config_c4, seed 4: 138,493 users, 26,744 items,
event times over 100 tumbling 1 s windows), in arrival order (ascending timestamps, datagen.to_records).  It is
rendered as text on the GPU and copied to the host once; then, warmed and timed with device events, each ending in a
synchronise:

  h2d      the copy of the text to the device (from pageable host memory, as a caller's bytes are; pinned beside it)
  parse    CooccurrenceCore.parse_interactions_device (both calls: the count and the fill)
  prepare  CooccurrenceCore.prepare_log with the default block of 100,000 records per watermark

and, on the same box, the path a caller had before: parse_interactions (one host thread) plus the numpy grouping
(the stable sort by window, the stable sort by user, the dense user indices).  One JSON line: milliseconds, bytes/s
and records/s for each (the fastest of --repeats, the slowest beside it), and the ratio host / device (the device side with the copy included).  The two paths'
outputs are compared as well.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def render_text(torch, users, items, ts):
    """"u,i,t\\n" lines of non-negative device tensors as one uint8 device tensor."""
    def digits(x):
        d = torch.ones_like(x)
        p = 10
        for _ in range(18):
            d += (x >= p).to(x.dtype)
            p *= 10
        return d

    fields = [users.to(torch.int64), items.to(torch.int64), ts.to(torch.int64)]
    nd = [digits(f) for f in fields]
    line = nd[0] + nd[1] + nd[2] + 3
    end = torch.cumsum(line, 0)
    start = end - line
    text = torch.empty(int(end[-1]), dtype=torch.uint8, device=users.device)
    at = start
    for f, d, sep in zip(fields, nd, (44, 44, 10)):  # ',' ',' '\n'
        p = 1
        for k in range(int(d.max())):
            m = d > k
            text[(at + d - 1 - k)[m]] = (48 + (f // p) % 10)[m].to(torch.uint8)
            p *= 10
        text[at + d] = sep
        at = at + d + 1
    return text


def host_group(users, items, ts, size):
    """what a caller did with numpy: firing order, the CSR by user, dense user indices (no late record in an
    ascending log)"""
    win = ts // size
    fire = np.argsort(win, kind="stable")
    wts, first = np.unique(win[fire], return_index=True)
    user_ids, rec_user = np.unique(users[fire], return_inverse=True)
    csr = np.argsort(rec_user, kind="stable")
    user_ptr = np.concatenate([[0], np.cumsum(np.bincount(rec_user, minlength=len(user_ids)))]).astype(np.int64)
    return (rec_user.astype(np.int32), items[fire], user_ids, user_ptr, items[fire][csr],
            np.concatenate([first, [len(fire)]]).astype(np.int64), wts * size + size - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=0, help="only the log's first N records (0: all)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--block", type=int, default=100_000, help="records per watermark")
    args = ap.parse_args()

    import torch

    import __graft_entry__

    pkg = __graft_entry__.load_package()
    from flink_cooccurrence_amd import datagen

    def stage(msg):
        print(f"[{time.perf_counter() - t_start:7.1f} s] {msg}", file=sys.stderr, flush=True)

    t_start = time.perf_counter()
    torch.cuda.init()
    dev = torch.device("cuda:0")
    d = datagen.config_c4()
    users, items, ts = datagen.to_records(d["user_ptr"], d["items"], d["ts"])
    if args.records:
        users, items, ts = users[:args.records], items[:args.records], ts[:args.records]
    n, size = len(users), int(d["window_ms"])
    text_dev = render_text(torch, *(torch.from_numpy(a).to(dev) for a in (users, items, ts)))
    host_text = text_dev.cpu()
    data = host_text.numpy().tobytes()
    pinned = host_text.pin_memory()
    n_bytes = len(data)
    del text_dev
    stage(f"{n} records rendered as {n_bytes} bytes of text")

    spread = {}  # the fastest repeat of a measurement -> its slowest

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()  # warm
        all_ms, out = [], None
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            a.record()
            out = fn()
            b.record()
            torch.cuda.synchronize()
            all_ms.append(a.elapsed_time(b))
        spread[min(all_ms)] = max(all_ms)
        return min(all_ms), out

    def wall(fn):
        all_ms, out = [], None
        for _ in range(max(1, args.repeats - 1)):
            t0 = time.perf_counter()
            out = fn()
            all_ms.append((time.perf_counter() - t0) * 1e3)
        spread[min(all_ms)] = max(all_ms)
        return min(all_ms), out

    with pkg.CooccurrenceCore(n_items=int(d["n_items"]), window_size_ms=size) as core:
        pageable = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        h2d_ms, text = timed(lambda: pageable.to(dev))
        h2d_pinned_ms, _ = timed(lambda: pinned.to(dev, non_blocking=True))
        parse_ms, recs = timed(lambda: core.parse_interactions_device(text))
        prep_ms, log = timed(lambda: core.prepare_log(*recs, records_per_watermark=args.block))
        stage(f"device: h2d {h2d_ms:.1f} ms, parse {parse_ms:.1f} ms, prepare {prep_ms:.1f} ms")
        host_parse_ms, hrecs = wall(lambda: pkg.parse_interactions(data))
        host_group_ms, hlog = wall(lambda: host_group(*hrecs, size))
        stage(f"host: parse {host_parse_ms:.1f} ms, grouping {host_group_ms:.1f} ms")
        # the two paths agree
        for g, h in zip(recs, hrecs):
            assert np.array_equal(g.cpu().numpy(), h)
        assert log.info["n_late"] == 0 and log.info["n_kept"] == n
        got = (log.rec_user, log.rec_item, log.user_ids, log.user_ptr, log.user_items)
        for g, h in zip(got, hlog[:5]):
            assert np.array_equal(g.cpu().numpy(), h)
        assert np.array_equal(log.window_ptr, hlog[5]) and np.array_equal(log.window_ts, hlog[6])

    def rate(ms):
        return {"ms": round(ms, 3), **({"ms_slowest": round(spread[ms], 3)} if ms in spread else {}), "bytes_per_s": round(n_bytes / ms * 1e3), "records_per_s": round(n / ms * 1e3)}

    dev_ms, host_ms = h2d_ms + parse_ms + prep_ms, host_parse_ms + host_group_ms
    print(json.dumps({
        "workload": f"C4 log as text: {n} records, {n_bytes} bytes, {log.info['n_users']} users, "
                    f"{log.info['n_windows']} windows, {args.block} records per watermark",
        "h2d": rate(h2d_ms), "h2d_pinned": rate(h2d_pinned_ms), "parse_device": rate(parse_ms),
        "prepare_log": rate(prep_ms), "device_total": rate(dev_ms),
        "host_parse": rate(host_parse_ms), "host_group": rate(host_group_ms), "host_total": rate(host_ms),
        "host_over_device": round(host_ms / dev_ms, 2), "device_no_slower": dev_ms <= host_ms,
    }))


if __name__ == "__main__":
    main()
