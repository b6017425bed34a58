"""What a checkpoint costs: cooc_snapshot_prepare, the device -> host copy, the host -> device write and
cooc_restore_finish, timed separately on two states (recorded in DESIGN.md §5c, not gated):

  c4     the `bench.py --config c4` log after its 100 windows: dense global rows;
  slabs  a C1-shaped log over 1e6 items: row slabs.

Every timed call synchronises the context's stream before it returns, so the wall clock around the call is the
device work plus the call's host-side table work; median of 10 after 2 warm-ups.  Per phase: milliseconds, blob
bytes, bytes moved over HBM and bytes per second, beside the bandwidth-bound estimate (bytes moved / the 8 TB/s
HBM peak of DESIGN §4).  Dense compaction moves 4 M^2 read plus the packed bytes written; the other device passes
read and write the blob once.  The median C4 window time of the same run says what a checkpoint costs relative to
a window.  --rescale adds cooc_restore_finish_parts: the blob split on the host into the 2 blobs of a job of 2
subtasks and restored into a world-1 context, beside the plain restore_finish of the same run (the split and the
expected result come from tests/_snapblob.py, the one numpy statement of the rescaling rule, instead of a second
copy here).  --other-lib PATH adds the plain restore_finish of the same blob through another build of the library
loaded beside this one: with the parent commit's libcooc_hip.so, the parent's restore on the same box in the same
invocation.  --item-cut N (with --user-cut, default 500, and --sample-on host|device) adds the SAMPLED C4 state:
the same log through a sampled context (the reference job's default is -ic 500 -uc 500), timed through
cooc_sampling_snapshot_prepare / cooc_sampling_restore_* right after the unsampled state of the same log, in the
same job, so the two lines compare.  Prints one JSON line per state.

  python scripts/bench_snapshot.py [--state c4|slabs|both] [--rescale] [--other-lib libcooc_hip.so]
                                   [--item-cut 500 [--user-cut 500] [--sample-on host|device]]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8e12
WARMUP, REPS = 2, 10


def _median_ms(fn, setup=None, cleanup=None):
    out = []
    for i in range(WARMUP + REPS):
        arg = setup() if setup else None
        t0 = time.perf_counter()
        fn(arg)
        dt = time.perf_counter() - t0
        if cleanup:
            cleanup(arg)
        if i >= WARMUP:
            out.append(dt * 1e3)
    return float(np.median(out))


def measure(pkg, core, make_core, label, n_items, dense, extra, rescale=False, window_size_ms=1000, sampled=False):
    from flink_cooccurrence_amd import _lib

    L = _lib.load()
    h = core._h
    info = _lib.CoocSnapshotInfo()
    # a sampled context goes through the entry points of its own blob format
    snapshot_prepare = L.cooc_sampling_snapshot_prepare if sampled else L.cooc_snapshot_prepare
    restore_begin = L.cooc_sampling_restore_begin if sampled else L.cooc_restore_begin
    restore_write = L.cooc_sampling_restore_write if sampled else L.cooc_restore_write
    restore_finish = L.cooc_sampling_restore_finish if sampled else L.cooc_restore_finish

    def prepare(_):
        _lib.check(snapshot_prepare(h, ctypes.byref(info)), h)

    prepare_ms = _median_ms(prepare, cleanup=lambda _: _lib.check(L.cooc_snapshot_release(h), h))
    prepare(None)
    blob = np.empty(info.bytes, np.uint8)
    step = 1 << 30

    def copy_out(_):
        for off in range(0, info.bytes, step):
            n = min(step, info.bytes - off)
            _lib.check(L.cooc_snapshot_copy(h, off, n, ctypes.c_void_p(blob.ctypes.data + off)), h)

    d2h_ms = _median_ms(copy_out)
    _lib.check(L.cooc_snapshot_release(h), h)

    write_ms, finish_ms = [], []
    for i in range(WARMUP + REPS):
        fresh = make_core()
        fh = fresh._h
        _lib.check(restore_begin(fh, info.bytes), fh)
        t0 = time.perf_counter()
        for off in range(0, info.bytes, step):
            n = min(step, info.bytes - off)
            _lib.check(restore_write(fh, off, n, ctypes.c_void_p(blob.ctypes.data + off)), fh)
        t1 = time.perf_counter()
        rinfo = _lib.CoocSnapshotInfo()
        _lib.check(restore_finish(fh, ctypes.byref(rinfo)), fh)
        t2 = time.perf_counter()
        if i >= WARMUP:
            write_ms.append((t1 - t0) * 1e3)
            finish_ms.append((t2 - t1) * 1e3)
        if i == WARMUP + REPS - 1:
            again = fresh.snapshot_sampled() if sampled else fresh.snapshot()
            assert again == blob.tobytes(), "the restored context's blob differs"
        fresh.close()

    nbytes = int(info.bytes)
    # bytes over HBM: prepare reads the state and writes the image (dense: the whole matrix read), then reads the
    # image once for the checksums; restore_finish reads the image twice (checksums, validation) and writes the
    # state (dense: the matrix zeroed first)
    m2 = 4 * n_items * n_items if dense else 0
    moved = {"prepare": (m2 * 2 if dense else nbytes) + 2 * nbytes, "restore_finish": 3 * nbytes + (m2 if dense else nbytes)}
    rec = dict(state=label, n_items=n_items, representation="dense" if dense else "slabs", blob_bytes=nbytes,
               info={k: v for k, v in info.as_dict().items() if k not in ("bytes", "format", "rank", "world")})
    for name, ms in (("prepare", prepare_ms), ("copy_d2h", d2h_ms), ("write_h2d", float(np.median(write_ms))),
                     ("restore_finish", float(np.median(finish_ms)))):
        b = moved.get(name, nbytes)
        rec[name] = dict(ms=round(ms, 3), bytes_moved=b, bytes_per_s=round(b / (ms * 1e-3), 1),
                         estimate_ms=round(b / HBM_PEAK * 1e3, 3) if name in moved else None)
    if rescale and not sampled:  # (a sampled context is single-subtask: nothing to rescale)
        rec["restore_finish_parts"] = measure_rescale(pkg, make_core, blob, n_items, dense)
    if OTHER_LIB and not sampled:
        ms = measure_other_library(OTHER_LIB, blob, n_items, window_size_ms)
        b = moved["restore_finish"]
        rec["restore_finish_other_library"] = dict(library=OTHER_LIB, ms=round(ms, 3), bytes_moved=b,
                                                   bytes_per_s=round(b / (ms * 1e-3), 1))
    rec.update(extra)
    print(json.dumps(rec), flush=True)


OTHER_LIB = None  # --other-lib: another build of libcooc_hip.so (the parent commit's) to time restore_finish with


def measure_other_library(path, blob, n_items, window_size_ms):
    """The plain cooc_restore_finish of the same blob through ANOTHER build of the library, loaded beside this one
    (its own ctypes handle, only the six calls below bound, so an older build without the newer entry points
    loads): the parent commit's restore on the same box, in the same invocation, timed as above.  Build it from a
    checkout of that commit (make -C flink-cooccurrence_amd/csrc) and pass its libcooc_hip.so."""
    from flink_cooccurrence_amd import _lib

    L = ctypes.CDLL(path)
    for name in ("cooc_create", "cooc_destroy", "cooc_last_error", "cooc_restore_begin", "cooc_restore_write",
                 "cooc_restore_finish"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _lib._SIGS[name]

    def ok(status, h):
        if status != _lib.COOC_OK:
            raise RuntimeError(f"{path}: status {status}: {(L.cooc_last_error(h) or b'').decode(errors='replace')}")

    step = 1 << 30
    finish_ms = []
    for i in range(WARMUP + REPS):
        cfg = _lib.CoocConfig(0, n_items, 10, 0, window_size_ms, 0, 0)  # make_core()'s configuration
        h = ctypes.c_void_p()
        ok(L.cooc_create(ctypes.byref(cfg), ctypes.byref(h)), None)
        try:
            ok(L.cooc_restore_begin(h, len(blob)), h)
            for off in range(0, len(blob), step):
                n = min(step, len(blob) - off)
                ok(L.cooc_restore_write(h, off, n, ctypes.c_void_p(blob.ctypes.data + off)), h)
            rinfo = _lib.CoocSnapshotInfo()
            t0 = time.perf_counter()
            ok(L.cooc_restore_finish(h, ctypes.byref(rinfo)), h)
            if i >= WARMUP:
                finish_ms.append((time.perf_counter() - t0) * 1e3)
        finally:
            L.cooc_destroy(h)
    return float(np.median(finish_ms))


def measure_rescale(pkg, make_core, blob, n_items, dense):
    """--rescale: the world-1 blob split on the host into the 2 blobs a job of 2 subtasks would have taken (rows by
    a mod 2, users by u mod 2; tests/_snapblob.py), then cooc_restore_finish_parts of the two into a world-1
    context, timed like restore_finish above and reported beside it (the plain restore of the one equivalent
    blob, same run).  The parts path reads what the plain path reads -- every part's image for the checksums,
    the validation and the install -- plus the parts' row-sum sections and M-sized tables."""
    from flink_cooccurrence_amd import _lib
    from tests import _snapblob as sb

    L = _lib.load()
    parts = [np.frombuffer(p, np.uint8) for p in sb.split(blob.tobytes(), 2, lambda u: np.asarray(u, np.int64) % 2)]
    sizes = np.array([len(p) for p in parts], np.int64)
    route = _lib.CoocUserRoute(_lib.COOC_ROUTE_MOD, 0, 0, None)
    step = 1 << 30
    write_ms, finish_ms = [], []
    for i in range(WARMUP + REPS):
        fresh = make_core()
        fh = fresh._h
        _lib.check(L.cooc_restore_begin_parts(fh, len(parts), sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))), fh)
        t0 = time.perf_counter()
        for k, p in enumerate(parts):
            for off in range(0, len(p), step):
                n = min(step, len(p) - off)
                _lib.check(L.cooc_restore_write_part(fh, k, off, n, ctypes.c_void_p(p.ctypes.data + off)), fh)
        t1 = time.perf_counter()
        rinfo = _lib.CoocSnapshotInfo()
        _lib.check(L.cooc_restore_finish_parts(fh, ctypes.byref(route), ctypes.byref(rinfo)), fh)
        t2 = time.perf_counter()
        if i >= WARMUP:
            write_ms.append((t1 - t0) * 1e3)
            finish_ms.append((t2 - t1) * 1e3)
        if i == WARMUP + REPS - 1:
            want = sb.expected_part([p.tobytes() for p in parts], 0, 1, sb.keep_all)
            assert fresh.snapshot() == want, "the rescaled context's blob differs from the expected one"
        fresh.close()
    total = int(sizes.sum())
    moved = 3 * total + (4 * n_items * n_items if dense else int(len(blob)))
    ms = float(np.median(finish_ms))
    return dict(n_parts=2, part_bytes=[int(x) for x in sizes], ms=round(ms, 3), bytes_moved=moved,
                bytes_per_s=round(moved / (ms * 1e-3), 1), estimate_ms=round(moved / HBM_PEAK * 1e3, 3),
                write_h2d_ms=round(float(np.median(write_ms)), 3))


def state_c4(pkg, rescale=False, sampling=None):
    """sampling: None, or (item_cut, user_cut, sample_on) to time the sampled state of the same log after the
    unsampled one"""
    import bench

    d, batches = bench.c4_batches(100)
    M = d["n_items"]
    make = lambda: pkg.CooccurrenceCore(n_items=M, topk=10, window_size_ms=1000, device=0)  # noqa: E731
    with make() as warm:
        for ts_w, uid, uptr, items in batches[:10]:
            warm.submit_batch(ts_w, uid, uptr, items)
            warm.finish_window_info(ts_w)
    core = make()
    lat = []
    for ts_w, uid, uptr, items in batches:
        t0 = time.perf_counter()
        core.submit_batch(ts_w, uid, uptr, items)
        core.finish_window_info(ts_w)
        lat.append((time.perf_counter() - t0) * 1e3)
    measure(pkg, core, make, "c4 after 100 windows", M, True, dict(c4_window_median_ms=round(float(np.median(lat)), 3)),
            rescale)
    core.close()
    if sampling is None:
        return
    item_cut, user_cut, sample_on = sampling
    make_s = lambda: pkg.CooccurrenceCore(n_items=M, topk=10, window_size_ms=1000, device=0, user_cut=user_cut,  # noqa: E731
                                          item_cut=item_cut, sample_seed=1, sample_on=sample_on)
    core = make_s()
    lat = []
    for ts_w, uid, uptr, items in batches:  # (the CSR order of a submit is the arrival order)
        t0 = time.perf_counter()
        core.submit_batch(ts_w, uid, uptr, items)
        core.finish_window_info(ts_w)
        lat.append((time.perf_counter() - t0) * 1e3)
    extra = dict(c4_window_median_ms=round(float(np.median(lat)), 3), item_cut=item_cut, user_cut=user_cut,
                 sample_on=sample_on, sampling_counters=core.sampling_counters())
    measure(pkg, core, make_s, f"c4 sampled ({item_cut}/{user_cut}, decided on the {sample_on}) after 100 windows", M, True,
            extra, sampled=True)
    core.close()


def state_slabs(pkg, rescale=False):
    from flink_cooccurrence_amd import datagen

    M = 1_000_000
    d = datagen.config_c1(seed=5, U=20_000, M=M, mean=20.0)
    users, items, ts = datagen.to_records(d["user_ptr"], d["items"], d["ts"])
    make = lambda: pkg.CooccurrenceCore(n_items=M, topk=10, window_size_ms=10_000, device=0)  # noqa: E731
    core = make()
    for lo in range(0, len(users), 50_000):
        sl = slice(lo, lo + 50_000)
        core.op_process_elements(users[sl], items[sl], ts[sl])
        core.op_process_watermark(int(ts[sl][-1]) - 1)
    measure(pkg, core, make, "C1-shaped, 20,000 users over 1e6 items", M, False, {}, rescale, window_size_ms=10_000)
    core.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--state", choices=["c4", "slabs", "both"], default="both")
    ap.add_argument("--rescale", action="store_true",
                    help="also time cooc_restore_finish_parts of the blob split into 2 parts, beside restore_finish")
    ap.add_argument("--other-lib", metavar="LIBCOOC_HIP_SO",
                    help="also time the plain restore_finish of the same blob through this other build of the library "
                         "(the parent commit's), in the same invocation")
    ap.add_argument("--item-cut", type=int, default=0,
                    help="also time the sampled C4 state with this item cut (the reference's default: 500)")
    ap.add_argument("--user-cut", type=int, default=500, help="the sampled state's reservoir size (with --item-cut)")
    ap.add_argument("--sample-on", choices=["host", "device"], default="host",
                    help="where the sampled state's windows are decided (with --item-cut)")
    args = ap.parse_args()
    global OTHER_LIB
    OTHER_LIB = os.path.abspath(args.other_lib) if args.other_lib else None
    import __graft_entry__

    pkg = __graft_entry__.load_package()
    if args.state in ("c4", "both"):
        state_c4(pkg, args.rescale, (args.item_cut, args.user_cut, args.sample_on) if args.item_cut > 0 else None)
    if args.state in ("slabs", "both"):
        state_slabs(pkg, args.rescale)


if __name__ == "__main__":
    main()
