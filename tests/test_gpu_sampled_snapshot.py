"""Checkpoint and restore of a sampled streaming context (snapshot_sampled / restore_sampled, the format-2 blob)
on the GPU, against the pure-Python model of the sampled mode (tests/_sampled_model.py) and the numpy statement of
the blob (tests/_snapblob_sampled.py): a run resumed from a blob equals the uninterrupted run, window by window, for
every pair of (host, device) decision modes and every representation of the global rows; the blob is canonical
across those; the device sampler's per-slot arrays grow to the restored slots; buffered windows travel; the device
validation refuses each kind of bad content and leaves a usable context; the interface's boundaries.

The log is the model's reference log with two extra records (70_000_000, 0) in window 4: item 0 is at the item cut
by then, so both are rejected and that user ends with a total and no reservoir; its id is above 2^26 (the hash-map
path of the slot lookup).  Global keys vanish in windows 1-5 and 7, so a slab holds zero-count entries at every cut
point.  _log() asserts all of that through the model before any test uses the GPU."""
import functools

import numpy as np
import pytest

import _sampled_model as sm
import _snapblob as f1
import _snapblob_sampled as f2

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE
ITEM_CUT, USER_CUT, TOPK = 20, 4, 5
LONER = 70_000_000
CUTS = (1, 4, 6)  # a snapshot after window 1, 4, 6 (0-based)
INFO_KEYS = ("bytes", "n_users", "history_items", "global_rows", "global_entries", "pending_windows",
             "pending_records", "format", "rank", "world")
KINDS = {"dense": (24, 1, "auto"), "slabs": (24, 1, "general"), "large": (40_500, 40_500 // 24, "auto")}


@functools.lru_cache(maxsize=None)
def _log(spread: int):
    n_items = 24 if spread == 1 else 40_500
    windows = sm.reference_log(spread=spread)
    windows[4] = windows[4] + [(LONER, 0), (LONER, 0)]
    # the preconditions, through the model alone
    model = sm.SampledModel(n_items, ITEM_CUT, USER_CUT, SEED)
    vanished = []
    for wi, recs in enumerate(windows):
        if wi == 4:
            assert model.item_count[0] == ITEM_CUT, "item 0 must be at the cut before window 4"
        before = set(model.G)
        mw = model.window(recs)
        vanished.append(len(before - set(model.G)))
        if wi == 4:
            assert mw.decisions[-2:] == ["r", "r"], "both extra records must be rejected"
    assert model.total[LONER] == 2 and LONER not in model.H and LONER >= 1 << 26
    assert vanished == [0, 14, 2, 19, 4, 10, 0, 6], "keys must vanish from the global rows in windows 1-5 and 7"
    return tuple(tuple(w) for w in windows)


def _core(pkg, kind, mode, **kw):
    n_items, _, planner = KINDS[kind]
    args = dict(n_items=n_items, topk=TOPK, user_cut=USER_CUT, item_cut=ITEM_CUT, sample_seed=SEED, planner=planner,
                sample_on=mode)
    args.update(kw)
    return pkg.CooccurrenceCore(**args)


def _model_at(kind, n_windows):
    """the model after the log's first n_windows windows"""
    n_items, spread, _ = KINDS[kind]
    model = sm.SampledModel(n_items, ITEM_CUT, USER_CUT, SEED)
    for recs in _log(spread)[:n_windows]:
        model.window(list(recs))
    return model


def _feed(core, wi, recs):
    users = np.array([u for u, _ in recs], np.int32)
    items = np.array([i for _, i in recs], np.int32)
    assert core.op_process_elements(users, items, np.full(len(recs), wi * 1000 + 1, np.int64)) == 0


def _fire(core, wi, recs):
    """window wi (1 s windows) through the operator mirror: its records in arrival order, then its watermark"""
    _feed(core, wi, recs)
    out = core.op_process_watermark(wi * 1000 + 999)
    assert len(out) == 1 and out[0].ts == wi * 1000 + 999
    return out[0]


def _check_window(core, model, w, mw, oracle, topk, rows_to_read=None):
    """one fired window and the state after it against the model (the checks of test_gpu_sampled, restated)"""
    rows = mw.rows()
    got, got16 = {}, {}
    for r, a in enumerate(w.rows.tolist()):
        s, e = int(w.row_ptr[r]), int(w.row_ptr[r + 1])
        assert np.all(np.diff(w.cols[s:e]) > 0), "delta columns not ascending"
        got[a] = dict(zip(w.cols[s:e].tolist(), w.exact[s:e].tolist()))
        got16[a] = dict(zip(w.cols[s:e].tolist(), w.v16[s:e].tolist()))
    assert got == rows, "signed delta rows differ"
    assert got16 == {a: {b: sm.i16(v) for b, v in r.items()} for a, r in rows.items()}, "cnt16 differs"
    assert w.rs_items.tolist() == sorted(rows)
    assert w.rs_exact.tolist() == [mw.rowsum[a] for a in sorted(rows)]
    assert w.rs_v32.tolist() == [sm.i32(mw.rowsum[a]) for a in sorted(rows)]
    assert w.observed == mw.observed
    assert len(w.rows) == len(rows) and len(w.cols) == sum(len(r) for r in rows.values())
    assert core.sampling_counters() == model.counters()
    oc = core.op_counters()
    assert oc["UserInteractionCounterObservedCooccurrences"] == model.observed_exact
    assert oc["RowSumProcessWindowRowSum"] == model.rowsum_acc
    assert oc["ItemRowRescorerRescoredItems"] == model.rescored
    assert oc["rescorer_observed"] == model.observed_rescorer
    assert core.global_observed() == (model.observed_exact, model.observed_rescorer)
    for u, t in model.total.items():  # every reservoir and total, the users without a reservoir included
        items, total = core.user_history(u)
        assert items.tolist() == model.H.get(u, []) and total == t, f"user {u}"
    grows = model.global_rows()
    M = model.n_items
    for a in (range(M) if rows_to_read is None else sorted(set(rows_to_read) | set(model.rs))):
        cols, cnt, cnt16 = core.global_row(a)
        want = grows.get(a, {})
        assert dict(zip(cols.tolist(), cnt.tolist())) == want, f"global row {a}"
        assert cnt16.tolist() == [sm.i16(v) for v in want.values()]
    ex, v32 = core.global_rowsums()
    want_rs = np.zeros(M, np.int64)
    for a, v in model.rs.items():
        want_rs[a] = v
    assert np.array_equal(ex, want_rs) and np.array_equal(v32, model.rs32())
    if topk:
        rp, cols, c16 = [0], [], []
        for a in sorted(rows):
            r = grows.get(a, {})
            cols += list(r)
            c16 += [sm.i16(v) for v in r.values()]
            rp.append(len(cols))
        sizes, vals, scores = oracle.rows_topk(sorted(rows), rp, cols, np.array(c16, np.int16), model.rs32(),
                                               model.observed_rescorer, topk)
        assert w.topk_rows.tolist() == sorted(rows)
        assert np.array_equal(w.topk_sizes, sizes)
        for r in range(len(sizes)):
            n = int(sizes[r])
            assert np.array_equal(w.topk_values[r, :n], vals[r, :n]), f"heap of row {w.topk_rows[r]}"
            assert np.array_equal(w.topk_scores[r, :n], scores[r, :n], equal_nan=True), f"scores of row {w.topk_rows[r]}"


def _blob_after(pkg, kind, mode, cut):
    """the blob of a fresh context of that kind and mode after windows 0..cut of the log"""
    windows = _log(KINDS[kind][1])
    with _core(pkg, kind, mode) as core:
        for wi in range(cut + 1):
            _fire(core, wi, windows[wi])
        return core.snapshot_sampled()


def _check_state(core, model):
    """what cooc_sampling_counters and cooc_copy_user_history read back of a restored state"""
    assert core.sampling_counters() == model.counters()
    for u, t in model.total.items():
        items, total = core.user_history(u)
        assert items.tolist() == model.H.get(u, []) and total == t, f"user {u}"


# ---- 1. resume equals uninterrupted ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("target", ["host", "device"])
@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_resume_equals_uninterrupted(pkg, oracle, kind, source, target, cut):
    n_items, spread, _ = KINDS[kind]
    windows = _log(spread)
    blob = _blob_after(pkg, kind, source, cut)
    model = _model_at(kind, cut + 1)
    info = pkg.CooccurrenceCore.sampled_snapshot_info(blob)
    assert info["format"] == 2 and info["item_cut"] == ITEM_CUT and info["seed"] == SEED
    assert info["total_users"] == len(model.total) and info["n_users"] == sum(1 for h in model.H.values() if h)
    assert info["counted_items"] == sum(1 for v in model.item_count.values() if v)
    assert info["global_entries"] == len(model.G)  # no key whose count went back to 0
    c = model.counters()
    assert (info["rejected"], info["fills"], info["replacements"], info["feedbacks"]) == (
        c["item_cut_rejections"], c["fills"], c["replacements"], c["feedbacks"])
    with _core(pkg, kind, target) as core:
        assert core.restore_sampled(blob) == {k: info[k] for k in INFO_KEYS}
        _check_state(core, model)
        assert core.snapshot_sampled() == blob, "a blob taken straight after the restore differs from the one restored"
        for wi in range(cut + 1, len(windows)):
            w = _fire(core, wi, windows[wi])
            mw = model.window(list(windows[wi]))
            _check_window(core, model, w, mw, oracle, TOPK, rows_to_read=None if n_items == 24 else [0, n_items - 1])


# ---- 2. canonical ---------------------------------------------------------------------------------------------------
def test_blob_is_canonical_across_modes_and_representations(pkg):
    """At each cut point: host-decided and device-decided contexts give the same bytes, and so do the dense matrix
    and the row slabs at the same n_items (the slabs hold zero-count entries by then, which the pack must drop)."""
    _log(1)
    cores = {(kind, mode): _core(pkg, kind, mode) for kind in ("dense", "slabs") for mode in ("host", "device")}
    try:
        for wi, recs in enumerate(_log(1)):
            for core in cores.values():
                _fire(core, wi, recs)
            if wi not in CUTS:
                continue
            blobs = {key: core.snapshot_sampled() for key, core in cores.items()}
            first = blobs[("dense", "host")]
            for key, blob in blobs.items():
                assert blob == first, f"the blob of {key} after window {wi} differs from the dense host-mode one"
            model = _model_at("dense", wi + 1)
            fields, s = f2.parse(first)
            assert fields == dict(n_items=24, user_cut=USER_CUT, window_size_ms=1000, rank=0, world=1)
            assert len(s[f1.ROW_COLS]) == len(model.G) and s[f1.ROW_CNTS].min() > 0
            assert s[f2.SMP_USER_IDS].tolist() == sorted(model.total)
            assert s[f2.SMP_TOTALS].tolist() == [model.total[u] for u in sorted(model.total)]
            counted = sorted(i for i, v in model.item_count.items() if v)
            assert s[f2.SMP_ITEM_IDS].tolist() == counted
            assert s[f2.SMP_ITEM_CNTS].tolist() == [model.item_count[i] for i in counted]
            assert f2.build(fields, s) == first  # the format's own statement gives the same bytes
            # the slab contexts do hold dead entries by now: more entries live in their arenas than the blob has keys
            assert cores[("slabs", "host")].global_slab_stats()[2] > len(model.G)
    finally:
        for core in cores.values():
            core.close()


def test_blob_is_canonical_large_universe(pkg):
    blobs = [_blob_after(pkg, "large", mode, 4) for mode in ("host", "device")]
    assert blobs[0] == blobs[1]
    model = _model_at("large", 5)
    _, s = f2.parse(blobs[0])
    assert len(s[f1.ROW_COLS]) == len(model.G) and LONER in s[f2.SMP_USER_IDS] and LONER not in s[f1.USER_IDS]


# ---- 3. slot growth -------------------------------------------------------------------------------------------------
def test_restore_grows_the_device_samplers_slots(pkg, oracle):
    """1,100 users (more than the device sampler's first 1,024 slots) saved in host mode, restored in device mode"""
    n_items, n_users = 64, 1100
    rng = np.random.default_rng(5)
    users = (np.arange(n_users) * 3 + 1).tolist()
    windows = [list(zip(users, np.minimum(rng.zipf(1.3, n_users) - 1, n_items - 1).tolist())) for _ in range(2)]
    model = sm.SampledModel(n_items, 200, USER_CUT, SEED)
    kw = dict(n_items=n_items, topk=TOPK, user_cut=USER_CUT, item_cut=200, sample_seed=SEED)
    with pkg.CooccurrenceCore(sample_on="host", **kw) as core:
        _fire(core, 0, windows[0])
        blob = core.snapshot_sampled()
    mw = model.window(windows[0])
    assert "r" in mw.decisions and "f" in mw.decisions  # users with and without a reservoir
    info = pkg.CooccurrenceCore.sampled_snapshot_info(blob)
    assert info["total_users"] == n_users and 0 < info["n_users"] < n_users
    with pkg.CooccurrenceCore(sample_on="device", **kw) as core:
        core.restore_sampled(blob)
        _check_state(core, model)
        w = _fire(core, 1, windows[1])
        mw = model.window(windows[1])
        _check_window(core, model, w, mw, oracle, TOPK)


# ---- 4. pending windows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source,target", [("host", "device"), ("device", "host")])
def test_buffered_windows_travel(pkg, oracle, source, target):
    windows = _log(1)
    model = _model_at("dense", 5)
    with _core(pkg, "dense", source) as core:
        for wi in range(5):
            _fire(core, wi, windows[wi])
        _feed(core, 5, windows[5])  # buffered: no watermark yet
        _feed(core, 6, windows[6][:7])
        blob = core.snapshot_sampled()
    info = pkg.CooccurrenceCore.sampled_snapshot_info(blob)
    assert (info["pending_windows"], info["pending_records"]) == (2, len(windows[5]) + 7)
    with _core(pkg, "dense", target) as core:
        core.restore_sampled(blob)
        out = core.op_process_watermark(5999)
        assert len(out) == 1 and out[0].ts == 5999
        _check_window(core, model, out[0], model.window(list(windows[5])), oracle, TOPK)
        _feed(core, 6, windows[6][7:])
        out = core.op_process_watermark(6999)
        assert len(out) == 1 and out[0].ts == 6999
        _check_window(core, model, out[0], model.window(list(windows[6])), oracle, TOPK)


# ---- 5. untrusted bytes on the device -------------------------------------------------------------------------------
PHASE_B_TOTALS = "a user with a history has no total, a total below its history's length, or a history longer than"


def _mutations(fields, good):
    """(name, sections, why): one bad content each, laid out and sealed as a valid blob, and a fragment of the
    message of the check that refuses it -- a phase-A bit, or phase B's sentence about the totals"""
    def edit(kind, fn):
        s = dict(good)
        s[kind] = good[kind].copy()
        fn(s[kind])
        return s

    def put(i, v):
        def fn(a):
            a[i] = v
        return fn

    def swap(a):
        a[0], a[1] = a[1], a[0]

    uids, hp = good[f1.USER_IDS], good[f1.HIST_PTR]
    tids = good[f2.SMP_USER_IDS].tolist()
    j = int(np.argmax(np.diff(hp)))            # a user with the longest history
    assert hp[j + 1] - hp[j] == USER_CUT >= 2
    at = tids.index(int(uids[j]))
    loner = tids.index(LONER)
    out = [
        ("a counter of 0", edit(f2.SMP_ITEM_CNTS, put(0, 0)), "(checks failed: 512;"),
        ("a counter of item_cut + 1", edit(f2.SMP_ITEM_CNTS, put(0, ITEM_CUT + 1)), "(checks failed: 512;"),
        ("counted items out of order", edit(f2.SMP_ITEM_IDS, swap), "(checks failed: 256;"),
        ("a counted item = n_items", edit(f2.SMP_ITEM_IDS, put(-1, fields["n_items"])), "(checks failed: 256;"),
        ("a total of 0", edit(f2.SMP_TOTALS, put(loner, 0)), "(checks failed: 2048;"),
        ("a total below the history's length", edit(f2.SMP_TOTALS, put(at, USER_CUT - 1)), PHASE_B_TOTALS),
    ]
    s = dict(good)                              # a user with a history missing from the users with a total
    s[f2.SMP_USER_IDS] = np.delete(good[f2.SMP_USER_IDS], at)
    s[f2.SMP_TOTALS] = np.delete(good[f2.SMP_TOTALS], at)
    assert len(s[f2.SMP_USER_IDS]) >= len(uids)  # (the directory's relation still holds)
    out.append(("a history's user without a total", s, PHASE_B_TOTALS))
    s = dict(good)                              # a history of user_cut + 1 items, its total large enough
    s[f1.HIST_ITEMS] = np.insert(good[f1.HIST_ITEMS], int(hp[j + 1]), 1)
    s[f1.HIST_PTR] = hp.copy()
    s[f1.HIST_PTR][j + 1:] += 1
    s[f2.SMP_TOTALS] = good[f2.SMP_TOTALS].copy()
    s[f2.SMP_TOTALS][at] = max(int(good[f2.SMP_TOTALS][at]), USER_CUT + 1)
    out.append(("a history longer than user_cut", s, PHASE_B_TOTALS))
    return out


@pytest.mark.parametrize("target", ["host", "device"])
def test_device_validation_refuses_bad_contents(pkg, oracle, target):
    windows = _log(1)
    good_blob = _blob_after(pkg, "dense", "host", 4)
    fields, good = f2.parse(good_blob)
    assert f2.build(fields, good) == good_blob
    base = _model_at("dense", 5)
    assert len(good[f2.SMP_ITEM_IDS]) >= 2
    with _core(pkg, "dense", target) as core:
        for name, sections, why in _mutations(fields, good):
            bad = f2.build(fields, sections)
            pkg.CooccurrenceCore.sampled_snapshot_info(bad)  # header, directory and scalars are fine
            with pytest.raises(pkg.IllegalArgumentException) as e:
                core.restore_sampled(bad)
            print(f"refused ({name}): {e.value}")
            assert why in str(e.value), name
            # the context is empty, sampled and usable
            assert core.sampling_counters() == dict.fromkeys(base.counters(), 0), name
            assert core.user_history(LONER)[1] == 0 and core.op_counters()["rescorer_observed"] == 0
        core.restore_sampled(good_blob)
        model = _model_at("dense", 5)
        _check_state(core, model)
        w = _fire(core, 5, windows[5])
        _check_window(core, model, w, model.window(list(windows[5])), oracle, TOPK)
    # after a refusal a context also runs from empty
    with _core(pkg, "dense", target) as core:
        with pytest.raises(pkg.IllegalArgumentException):
            core.restore_sampled(f2.build(fields, _mutations(fields, good)[0][1]))
        model = _model_at("dense", 0)
        w = _fire(core, 0, windows[0])
        _check_window(core, model, w, model.window(list(windows[0])), oracle, TOPK)


# ---- 6. boundaries of the interface ---------------------------------------------------------------------------------
def test_interface_boundaries(pkg):
    windows = _log(1)
    blob = _blob_after(pkg, "dense", "host", 1)
    with pkg.CooccurrenceCore(n_items=24, topk=TOPK, user_cut=USER_CUT) as plain:  # unsampled
        with pytest.raises(pkg.IllegalStateException):
            plain.snapshot_sampled()
        with pytest.raises(pkg.IllegalStateException):
            plain.restore_sampled(blob)
        with pytest.raises(pkg.IllegalArgumentException):  # the format-1 family: an unknown magic
            plain.restore(blob)
        with pytest.raises(pkg.IllegalArgumentException):
            pkg.CooccurrenceCore.snapshot_info(blob)
        plain.submit_batch(0, [1, 2], [0, 2, 3], [3, 4, 5])
        plain.finish_window(0)
        plain_blob = plain.snapshot()
    assert pkg.CooccurrenceCore.snapshot_info(plain_blob)["format"] == 1
    for kw in (dict(item_cut=ITEM_CUT + 1), dict(sample_seed=SEED + 1), dict(user_cut=USER_CUT + 1), dict(n_items=25),
               dict(window_size_ms=2000)):
        for mode in ("host", "device"):
            with _core(pkg, "dense", mode, **kw) as core:
                with pytest.raises(pkg.IllegalArgumentException):
                    core.restore_sampled(blob)
                assert core.sampling_counters()["fills"] == 0
    for mode in ("host", "device"):
        with _core(pkg, "dense", mode) as core:
            with pytest.raises(pkg.IllegalArgumentException):  # a format-1 blob
                core.restore_sampled(plain_blob)
            with pytest.raises(pkg.IllegalArgumentException):  # truncated
                core.restore_sampled(blob[:-8])
            core.restore_sampled(blob)
            with pytest.raises(pkg.IllegalStateException):  # streaming state now
                core.restore_sampled(blob)
        with _core(pkg, "dense", mode) as core:
            core.submit_batch(0, [1], [0, 1], [2])
            with pytest.raises(pkg.IllegalStateException):  # after a submit
                core.restore_sampled(blob)
            with pytest.raises(pkg.IllegalStateException):  # a window is staged
                core.snapshot_sampled()
            core.finish_window(0)
            assert pkg.CooccurrenceCore.sampled_snapshot_info(core.snapshot_sampled())["total_users"] == 1
        with _core(pkg, "dense", mode) as core:  # an empty sampled context has a blob too, and takes it back
            empty = core.snapshot_sampled()
            assert len(empty) == f2.HEADER_BYTES + (16 + 1 + 1 + 1 + 8) * 8
        with _core(pkg, "dense", mode) as core:
            core.restore_sampled(empty)
            _fire(core, 0, windows[0])
            assert core.snapshot_sampled() == _blob_after(pkg, "dense", "host", 0)
