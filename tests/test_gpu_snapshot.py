"""Checkpoint and restore of the streaming state (cooc_snapshot_prepare .. cooc_restore_finish).

The resume cases share one check: a C1-shaped log goes to operator A up to the middle of the stream, A's blob is
taken (the watermark rule leaves the current window buffered, so the operator's pending windows are in it), A is
closed, a new operator B restores the blob and gets the rest; A's windows followed by B's must equal an
uninterrupted oracle.OracleStream's window by window, and B's final accumulators, sampled global rows and global
row sums the oracle's.  The oracle runs once per item universe and is shared.  All comparisons are exact.
Needs an MI355X.
"""
import ctypes
import functools
import struct

import numpy as np
import pytest

from tests._helpers import (INT64_MAX, as_int_keys, assert_windows_equal, micro_events, micro_logs, run_events,
                            window_rows)

pytestmark = pytest.mark.gpu

CHUNK = 5000
HEADER = 64
N_SECTIONS = 15
# section kinds (cooc_snapshot.h)
SCALARS, USER_IDS, HIST_PTR, HIST_ITEMS, ROW_IDS, ROW_PTR, ROW_COLS, ROW_CNTS, ROW_SUMS = range(1, 10)
XSUM_IDS, XSUM_VALS, PEND_TS, PEND_PTR, PEND_USERS, PEND_ITEMS = range(10, 16)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _operator(pkg, M, planner="auto", top_k=10, **kw):
    return pkg.NonSampledUserInteractionCounterOneInputStreamOperator(1, "SECONDS", n_items=M, top_k=top_k,
                                                                      planner=planner, **kw)


@functools.lru_cache(maxsize=None)
def _reference(M):
    """The C1-shaped log over M items and what an uninterrupted oracle makes of it (computed once)."""
    from flink_cooccurrence_amd import datagen
    from oracle import oracle

    d = datagen.config_c1(seed=5, U=1500, M=M, mean=20.0)
    users, items, ts = datagen.to_records(d["user_ptr"], d["items"], d["ts"])
    ref = oracle.OracleStream(1000, topk=10)
    n_chunks = (len(users) + CHUNK - 1) // CHUNK
    want, upto = [], []
    for c in range(n_chunks):
        sl = slice(c * CHUNK, (c + 1) * CHUNK)
        ref.process_elements(users[sl], items[sl], ts[sl])
        want += ref.process_watermark(int(ts[sl][-1]) - 1)
        upto.append(len(want))  # windows fired through chunk c
    want += ref.process_watermark(INT64_MAX)
    return dict(M=M, users=users, items=items, ts=ts, n_chunks=n_chunks, mid=n_chunks // 2, want=want, upto=upto,
                counters=ref.counters(), global_rows=ref.global_rows(), global_rowsums=ref.global_rowsums())


def _feed(op, R, c0, c1, final=False):
    got = []
    for c in range(c0, c1):
        sl = slice(c * CHUNK, (c + 1) * CHUNK)
        op.process_elements(R["users"][sl], R["items"][sl], R["ts"][sl])
        got += op.process_watermark(int(R["ts"][sl][-1]) - 1)
    if final:
        got += op.process_watermark(INT64_MAX)
    return got


def _check_windows(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert_windows_equal(g, w)


def _check_final(op, R):
    """Accumulators, sampled global rows and global row sums, as test_streaming_sparse_global_rows_vs_oracle."""
    assert op.accumulators() == R["counters"]
    rows, rp, cols, exact, v16 = R["global_rows"]
    for r in list(range(0, len(rows), max(1, len(rows) // 200))) + [len(rows) - 1]:
        a = int(rows[r])
        c, n, n16 = op.core.global_row(a)
        assert np.array_equal(c, cols[rp[r]:rp[r + 1]]), f"global row {a}"
        assert np.array_equal(n.astype(np.int64), exact[rp[r]:rp[r + 1]])
        assert np.array_equal(n16, v16[rp[r]:rp[r + 1]])
    gi, gv32, gex = R["global_rowsums"]
    ex, v32 = op.core.global_rowsums()
    assert np.array_equal(ex[gi], gex) and np.array_equal(v32[gi], gv32)


def _prefix(pkg, R, planner="auto"):
    """Operator A fed to the middle -> (its windows, its blob, the blob's info); A closed."""
    A = _operator(pkg, R["M"], planner)
    got = _feed(A, R, 0, R["mid"])
    blob = A.snapshot()
    info = A.core.last_snapshot_info
    A.close()
    assert info["pending_records"] > 0 and info["pending_windows"] >= 1  # the buffered window is in the blob
    assert info["bytes"] == len(blob) and info["format"] == 1 and (info["rank"], info["world"]) == (0, 1)
    return got, blob, info


def _resume(op, R, got_before):
    """B (restored) gets the rest of the stream; everything against the uninterrupted oracle."""
    got = got_before + _feed(op, R, R["mid"], R["n_chunks"], final=True)
    _check_windows(got, R["want"])
    _check_final(op, R)


@functools.lru_cache(maxsize=None)
def _good(pkg, M=1003, planner="auto"):
    return _prefix(pkg, _reference(M), planner)


# ---- the blob, read by hand -------------------------------------------------------
def _sections(blob):
    """{kind: (offset, bytes, count, checksum, directory offset)}"""
    out = {}
    for k in range(N_SECTIONS):
        at = HEADER + 40 * k
        kind, elem, off, nbytes, count, cs = struct.unpack_from("<iiqqqQ", blob, at)
        out[kind] = (off, nbytes, count, cs, at)
    return out


def _splitmix64(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _checksum(words):
    """sum over the 8-byte words w_i of splitmix64(w_i ^ i), mod 2^64"""
    w = np.frombuffer(words, "<u8")
    with np.errstate(over="ignore"):
        return int(_splitmix64(w ^ np.arange(len(w), dtype=np.uint64)).sum(dtype=np.uint64))


def _reseal(blob, kind):
    """Recompute section `kind`'s checksum and the header's own after an edit of the payload."""
    b = bytearray(blob)
    off, nbytes, _, _, at = _sections(blob)[kind]
    struct.pack_into("<Q", b, at + 32, _checksum(bytes(b[off:off + (nbytes + 7) // 8 * 8])))
    struct.pack_into("<Q", b, 48, 0)
    struct.pack_into("<Q", b, 48, _checksum(bytes(b[:HEADER + 40 * N_SECTIONS])))
    return bytes(b)


def test_checksums_are_the_documented_ones(pkg, torch_cuda):
    """Every section's checksum and the header's, recomputed on the host from the documented formula."""
    _, blob, _ = _good(pkg)
    for kind, (off, nbytes, count, cs, _) in _sections(blob).items():
        assert off % 8 == 0 and cs == _checksum(blob[off:off + (nbytes + 7) // 8 * 8]), f"section {kind}"
    assert _reseal(blob, ROW_COLS) == blob


# ---- resume ---------------------------------------------------------------------------------------
def test_resume_dense_unaligned_rows(pkg, torch_cuda):
    """M = 1003: no multiple of 4 or 64, so the matrix rows start unaligned and end in a ragged tail."""
    R = _reference(1003)
    got, blob, info = _good(pkg)
    B = _operator(pkg, 1003)
    assert B.restore(blob) == info == B.snapshot_info(blob)
    assert B.snapshot() == blob  # canonical: B right after the restore gives A's bytes
    _resume(B, R, got)
    B.close()


def test_resume_slabs(pkg, torch_cuda):
    """M = 40,500: the global rows are slabs that moved and were compacted before the snapshot."""
    R = _reference(40_500)
    got, blob, info = _prefix(pkg, R)
    assert len(got) >= 5
    B = _operator(pkg, 40_500)
    assert B.restore(blob) == info
    assert B.snapshot() == blob
    _resume(B, R, got)
    B.close()


def test_cross_representation(pkg, torch_cuda):
    """The same prefix through the dense matrix (planner auto) and through row slabs (planner large) gives
    byte-identical blobs, and each restores into the other representation."""
    R = _reference(1003)
    got_d, blob_d, _ = _good(pkg)
    got_s, blob_s, _ = _prefix(pkg, R, planner="large")
    assert blob_d == blob_s
    _check_windows(got_s, R["want"][:len(got_s)])
    for planner, blob, got in (("large", blob_d, got_d), ("auto", blob_s, got_s)):
        B = _operator(pkg, 1003, planner)
        B.restore(blob)
        assert B.snapshot() == blob
        _resume(B, R, got)
        B.close()


def test_ranges(pkg, torch_cuda):
    """The blob copied out in 4,093-byte ranges equals the one-shot copy; a restore written in 4,093-byte ranges
    in descending offset order succeeds; prepare, restore_finish and snapshot_info agree."""
    from flink_cooccurrence_amd import _lib

    L = _lib.load()
    R = _reference(1003)
    A = _operator(pkg, 1003)
    got = _feed(A, R, 0, R["mid"])
    one_shot = A.snapshot()
    assert A.core.snapshot(range_bytes=4093) == one_shot
    info = A.core.last_snapshot_info
    A.close()
    B = _operator(pkg, 1003)
    h = B.core._h
    buf = np.frombuffer(one_shot, np.uint8)
    _lib.check(L.cooc_restore_begin(h, len(buf)), h)
    n_ranges = 0
    for off in reversed(range(0, len(buf), 4093)):
        n = min(4093, len(buf) - off)
        _lib.check(L.cooc_restore_write(h, off, n, ctypes.c_void_p(buf.ctypes.data + off)), h)
        n_ranges += 1
    assert n_ranges > 10
    rinfo = _lib.CoocSnapshotInfo()
    _lib.check(L.cooc_restore_finish(h, ctypes.byref(rinfo)), h)
    assert rinfo.as_dict() == info == pkg.CooccurrenceCore.snapshot_info(one_shot)
    _resume(B, R, got)
    B.close()


# ---- compaction shapes ------------------------------------------------------------------------------
def _all_rows(core, M):
    return {a: tuple(x.tolist() for x in core.global_row(a)[:2]) for a in range(M)}


@pytest.mark.parametrize("M", [1, 65, 1003])
def test_compaction_shapes(pkg, torch_cuda, M):
    """Lane, wave and row boundaries of the dense compaction, through the public path.  A full row cannot sit
    beside a never-seen item (the matrix is symmetric), so the state is checked twice.  After window 1: an item
    in the middle never seen (an empty row between full ones), and at M = 1003 a row of exactly 65 entries (item 10
    held twice by a user with 64 other items) and rows of exactly 64.  After window 2, where one user holds item
    0 twice and every other item once: item 0's row is full, itself included (at M = 65 exactly 65 entries, the
    other rows exactly 64).  Each time every item's global_row after a restore equals the row before the snapshot,
    and the row-slab representation gives the same bytes."""
    windows = []
    if M == 65:
        windows.append([(1, [0, 0] + [b for b in range(1, M) if b != 32])])
    elif M == 1003:
        windows.append([(1, [10, 10] + list(range(11, 75))), (2, [900, 901, 1002])])
    windows.append([(3, [0, 0] + list(range(1, M)))])
    cores = {p: pkg.CooccurrenceCore(n_items=M, topk=0, planner=p) for p in (("auto", "large") if M > 1 else ("auto",))}
    for w, users in enumerate(windows):
        ts = 1000 * (w + 1) - 1
        up = np.concatenate([[0], np.cumsum([len(it) for _, it in users])]).astype(np.int64)
        blobs = {}
        for p, core in cores.items():
            core.submit_batch(ts, [u for u, _ in users], up, np.concatenate([it for _, it in users]).astype(np.int32))
            core.finish_window(ts)
            blobs[p] = core.snapshot()
        core = cores["auto"]
        before = _all_rows(core, M)
        lens = {a: len(r[0]) for a, r in before.items()}
        if w == len(windows) - 1:
            assert before[0][0] == list(range(M)) and before[0][1][0] >= 2  # the full row, item 0 with itself
            if M == 65:
                assert lens[0] == 65 and all(lens[a] == 64 for a in range(1, M))
        else:
            assert 0 in lens.values() and any(lens[a] == 0 and a not in (0, M - 1) for a in lens)  # an unseen item
            assert 64 in lens.values()
            if M == 1003:
                assert lens[10] == 65 and lens[11] == 64 and lens[74] == 64 and lens[75] == 0 and lens[1002] == 2
        assert core.last_snapshot_info["global_rows"] == sum(1 for n in lens.values() if n)
        assert core.last_snapshot_info["global_entries"] == sum(lens.values())
        if M > 1:
            assert blobs["auto"] == blobs["large"]
        for p in cores:
            with pkg.CooccurrenceCore(n_items=M, topk=0, planner=p) as fresh:
                fresh.restore(blobs["auto"])
                assert _all_rows(fresh, M) == before, f"planner {p}"
                assert np.array_equal(fresh.global_rowsums()[0], core.global_rowsums()[0])
                assert fresh.global_observed() == core.global_observed()
                assert fresh.snapshot() == blobs["auto"]
    for core in cores.values():
        core.close()


# ---- user table -------------------------------------------------------------------------------------
def test_user_table_and_long_history(pkg, oracle, torch_cuda):
    """User ids -5 and 2^26 + 3 live in the hash map, 7 in the dense table; one history has 1 item, one 5,000
    (copied in pieces).  After the restore a window touching all of them equals the oracle's."""
    M = 1003
    rng = np.random.default_rng(11)
    big = 2**26 + 3
    first = [(-5, [17])] + [(7, rng.integers(0, M, 5000).tolist())] + [(big, rng.integers(0, M, 12).tolist())]
    second = [(-5, [3, 17]), (7, [1, 2, 1002]), (big, [0]), (8, [5, 6])]
    ev = []
    for t0, users in ((100, first), (1100, second)):
        rec = [(u, it) for u, items in users for it in items]
        order = rng.permutation(len(rec)).tolist()  # the users' records interleaved, 50 per millisecond
        ev += [("e", rec[i][0], rec[i][1], t0 + k // 50) for k, i in enumerate(order)]
        ev.append(("w", t0 + 899))
    cut = 1 + next(i for i, e in enumerate(ev) if e[0] == "w")
    ref = oracle.OracleStream(1000, topk=10)
    want = run_events(ev + [("w", INT64_MAX)], ref.process_elements, ref.process_watermark)
    A = _operator(pkg, M)
    got = run_events(ev[:cut], A.process_elements, A.process_watermark)
    blob = A.snapshot()
    info = A.core.last_snapshot_info
    A.close()
    assert info["n_users"] == 3 and info["history_items"] == 5013 and info["pending_records"] == 0
    ids = np.frombuffer(blob, "<i4", 3, _sections(blob)[USER_IDS][0])
    assert ids.tolist() == [-5, 7, big]  # ascending ids
    B = _operator(pkg, M)
    B.restore(blob)
    assert B.snapshot() == blob
    got += run_events(ev[cut:] + [("w", INT64_MAX)], B.process_elements, B.process_watermark)
    assert len(want) == 2
    _check_windows(got, want)
    assert B.accumulators() == ref.counters()
    B.close()


# ---- user_cut ---------------------------------------------------------------------------------------
def test_user_cut_across_restore(pkg, oracle, torch_cuda):
    """user_cut = 3: a user who reached the cap before the snapshot adds nothing after it, a user at 2 exactly one
    more (as test_streaming_user_cut_vs_oracle: against OracleStream with the same cut); a context with another
    user_cut refuses the blob."""
    M = 50
    ev = [("e", 1, 4, 10), ("e", 1, 5, 11), ("e", 1, 6, 12), ("e", 2, 7, 13), ("e", 2, 8, 14), ("e", 3, 4, 15),
          ("w", 999)]
    rest = [("e", 1, 9, 1010), ("e", 1, 10, 1011), ("e", 2, 11, 1012), ("e", 2, 12, 1013), ("e", 3, 13, 1014),
            ("w", INT64_MAX)]
    ref = oracle.OracleStream(1000, topk=5, user_cut=3)
    want = run_events(ev + rest, ref.process_elements, ref.process_watermark)
    A = _operator(pkg, M, top_k=5, user_cut=3)
    got = run_events(ev, A.process_elements, A.process_watermark)
    blob = A.snapshot()
    A.close()
    other = _operator(pkg, M, top_k=5, user_cut=4)
    with pytest.raises(pkg.IllegalArgumentException):
        other.restore(blob)
    other.close()
    B = _operator(pkg, M, top_k=5, user_cut=3)
    B.restore(blob)
    got += run_events(rest, B.process_elements, B.process_watermark)
    assert len(want) == 2
    _check_windows(got, want)
    rows = window_rows(got[1])
    assert 9 not in rows and 10 not in rows and 12 not in rows  # user 1 capped; user 2's second item dropped
    assert rows[11] == {7: 1, 8: 1} and rows[13] == {4: 1}     # user 2 exactly one more; user 3 free
    assert B.accumulators() == ref.counters()
    B.close()


# ---- empty ------------------------------------------------------------------------------------------
def test_empty_blob_then_micro_log(pkg, oracle, torch_cuda):
    """A fresh context's blob restores; a golden micro-log then runs to its golden windows."""
    log = max((l for l in micro_logs() if not l.get("closed_form_only")), key=lambda l: len(l["windows"]))
    ev = micro_events(log)
    M = 1 + max(e[2] for e in ev if e[0] == "e")
    A = pkg.NonSampledUserInteractionCounterOneInputStreamOperator(log["window_ms"], n_items=M, top_k=3)
    blob = A.snapshot()
    info = A.core.last_snapshot_info
    A.close()
    assert (info["n_users"], info["global_rows"], info["pending_records"]) == (0, 0, 0)
    op = pkg.NonSampledUserInteractionCounterOneInputStreamOperator(log["window_ms"], n_items=M, top_k=3)
    assert op.restore(blob) == info
    got = run_events(ev, op.process_elements, op.process_watermark)
    ref = oracle.OracleStream(log["window_ms"], topk=3)
    want = run_events(ev, ref.process_elements, ref.process_watermark)
    assert len(got) == len(want) == len(log["windows"])
    for g, w, gold in zip(got, want, log["windows"]):
        assert_windows_equal(g, w)
        assert window_rows(g) == as_int_keys(gold["rows"])
    assert op.accumulators() == ref.counters()
    op.close()


# ---- refusals ---------------------------------------------------------------------------------------
def _refused_then_good(pkg, bad, exc, why):
    """`bad` is refused with exc by the check whose message holds `why`; the same context then restores the good
    blob and resumes correctly."""
    R = _reference(1003)
    got, good, _ = _good(pkg)
    B = _operator(pkg, 1003)
    with pytest.raises(exc) as e:
        B.restore(bad)
    print(f"refused: {e.value}")
    assert e.value.status == 1 and why in str(e.value)
    B.restore(good)
    _resume(B, R, got)
    B.close()
    return str(e.value)


def test_refuses_staged_window_and_used_context(pkg, torch_cuda):
    _, good, _ = _good(pkg)
    with pkg.CooccurrenceCore(n_items=1003, topk=10) as core:
        core.submit_batch(999, [1], [0, 2], [3, 4])
        with pytest.raises(pkg.IllegalStateException) as e:  # a staged, unfinished window
            core.snapshot()
        assert e.value.status == 2
        core.finish_window(999)
        assert pkg.CooccurrenceCore.snapshot_info(core.snapshot())["n_users"] == 1
        with pytest.raises(pkg.IllegalStateException):  # the context has state
            core.restore(good)
    op = _operator(pkg, 1003)
    op.process_element(1, 2, 500)  # an element processed
    with pytest.raises(pkg.IllegalStateException) as e:
        op.restore(good)
    assert e.value.status == 2
    op.close()


@pytest.mark.parametrize("what", ["n_items", "window_size_ms"])
def test_refuses_other_configuration(pkg, torch_cuda, what):
    _, good, _ = _good(pkg)
    if what == "n_items":
        op = _operator(pkg, 1004)
    else:
        op = pkg.NonSampledUserInteractionCounterOneInputStreamOperator(2, "SECONDS", n_items=1003, top_k=10)
    with pytest.raises(pkg.IllegalArgumentException) as e:
        op.restore(good)
    print(f"refused: {e.value}")
    assert e.value.status == 1 and "taken with n_items" in str(e.value)  # (the one message names all three settings)
    assert op.process_watermark(INT64_MAX) == []  # still empty and usable
    op.close()


def test_refuses_truncated_blob(pkg, torch_cuda):
    _, good, _ = _good(pkg)
    _refused_then_good(pkg, good[:-1], pkg.IllegalArgumentException, "its length is not the length it announces")


@pytest.mark.parametrize("kind", [k for k in range(1, N_SECTIONS + 1) if k not in (XSUM_IDS, XSUM_VALS)])
def test_refuses_flipped_payload_bit(pkg, torch_cuda, kind):
    """One flipped bit in a section's payload: the section's checksum catches it."""
    _, good, _ = _good(pkg)
    off, nbytes, _, _, _ = _sections(good)[kind]
    assert nbytes > 0
    b = bytearray(good)
    b[off + nbytes // 2] ^= 0x10
    msg = _refused_then_good(pkg, bytes(b), pkg.IllegalArgumentException, "checksum mismatch in section")
    assert msg.endswith(f"checksum mismatch in section {kind}")  # (the message names the kind, 1-based like `kind`)


# the check that refuses each edit: a phase-A bit (by position), or phase B (the rows through their offsets)
PHASE_B_ROWS = "not strictly ascending or its counts do not sum"
BAD_CONTENTS = {
    "column_out_of_range": "invalid contents (checks failed: 32;",
    "columns_swapped": PHASE_B_ROWS,  # (both columns stay in range: phase A passes)
    "count_zero": "invalid contents (checks failed: 64;",
    "row_sum_off": PHASE_B_ROWS,
    "item_out_of_range": "invalid contents (checks failed: 4;",
}


@pytest.mark.parametrize("edit", list(BAD_CONTENTS))
def test_refuses_bad_contents_behind_good_checksums(pkg, torch_cuda, edit):
    """Edits with the checksums recomputed: only the device validation pass can catch them."""
    _, good, _ = _good(pkg)
    S = _sections(good)
    b = bytearray(good)
    rp = np.frombuffer(good, "<i8", S[ROW_PTR][2], S[ROW_PTR][0])
    r = next(i for i in range(len(rp) - 1) if rp[i + 1] - rp[i] >= 2)
    at_col = S[ROW_COLS][0] + 4 * int(rp[r])
    c0, c1 = struct.unpack_from("<ii", good, at_col)
    if edit == "column_out_of_range":
        struct.pack_into("<i", b, at_col + 4 * int(rp[r + 1] - rp[r] - 1), 1003)  # the row's last column: still ascending
        kind = ROW_COLS
    elif edit == "columns_swapped":
        struct.pack_into("<ii", b, at_col, c1, c0)
        kind = ROW_COLS
    elif edit == "count_zero":
        struct.pack_into("<I", b, S[ROW_CNTS][0] + 4 * int(rp[r]), 0)
        kind = ROW_CNTS
    elif edit == "row_sum_off":
        at = S[ROW_SUMS][0] + 8 * r
        struct.pack_into("<q", b, at, struct.unpack_from("<q", good, at)[0] + 1)
        kind = ROW_SUMS
    else:
        struct.pack_into("<i", b, S[HIST_ITEMS][0], -1)
        kind = HIST_ITEMS
    bad = _reseal(bytes(b), kind)
    assert bad != good and pkg.CooccurrenceCore.snapshot_info(bad) == pkg.CooccurrenceCore.snapshot_info(good)
    _refused_then_good(pkg, bad, pkg.IllegalArgumentException, BAD_CONTENTS[edit])


# ---- the JNI call sequence ----------------------------------------------------------------------------
def test_jni_snapshot_sequence_replayed(pkg, oracle, torch_cuda):
    """What the Java operators' snapshotState / initializeState do through cooc_jni.c, call for call
    (the pattern of tests/test_boundary_sequence.py): prepare, ranged copies into separately allocated arrays,
    release; in a new handle begin, ranged writes, finish; then the operator's usual per-watermark sequence."""
    from flink_cooccurrence_amd import _lib, datagen
    from tests.test_boundary_sequence import JniReplay, _ref_records

    L = pkg.load_library()
    M, max_array = 300, 8191  # (the Java side: Integer.MAX_VALUE - 8 bytes per array)
    d = datagen.config_c1(seed=13, U=600, M=M, mean=12.0)
    users, items, ts = datagen.to_records(d["user_ptr"], d["items"], d["ts"])
    ref = oracle.OracleStream(1000)
    step, half = 700, (len(users) // 1400) * 700
    want, got = [], []
    A = JniReplay(L, M, 1000, [0], 0, 997)
    for lo in range(0, half, step):
        sl = slice(lo, lo + step)
        ref.process_elements(users[sl], items[sl], ts[sl])
        want += ref.process_watermark(int(ts[sl][-1]) - 1)
        got += A.process_watermark(users[sl], items[sl], ts[sl], int(ts[sl][-1]) - 1)[0]
    # snapshotState
    info = _lib.CoocSnapshotInfo()
    _lib.check(L.cooc_snapshot_prepare(A.h, ctypes.byref(info)), A.h)
    arrays = []
    for off in range(0, info.bytes, max_array):
        arr = np.zeros(min(max_array, info.bytes - off), np.uint8)  # one Java byte[] per range
        _lib.check(L.cooc_snapshot_copy(A.h, off, len(arr), ctypes.c_void_p(arr.ctypes.data)), A.h)
        arrays.append(arr)
    _lib.check(L.cooc_snapshot_release(A.h), A.h)
    assert L.cooc_snapshot_copy(A.h, 0, 1, ctypes.c_void_p(arrays[0].ctypes.data)) == _lib.COOC_ERR_STATE  # released
    A.close()
    assert len(arrays) > 3 and info.pending_records > 0
    # initializeState
    B = JniReplay(L, M, 1000, [0], 0, 997)
    _lib.check(L.cooc_restore_begin(B.h, sum(len(a) for a in arrays)), B.h)
    off = 0
    for arr in arrays:
        _lib.check(L.cooc_restore_write(B.h, off, len(arr), ctypes.c_void_p(arr.ctypes.data)), B.h)
        off += len(arr)
    rinfo = _lib.CoocSnapshotInfo()
    _lib.check(L.cooc_restore_finish(B.h, ctypes.byref(rinfo)), B.h)
    assert rinfo.as_dict() == info.as_dict()
    for lo in range(half, len(users), step):
        sl = slice(lo, lo + step)
        ref.process_elements(users[sl], items[sl], ts[sl])
        want += ref.process_watermark(int(ts[sl][-1]) - 1)
        got += B.process_watermark(users[sl], items[sl], ts[sl], int(ts[sl][-1]) - 1)[0]
    want += ref.process_watermark(INT64_MAX)
    got += B.process_watermark([], [], [], INT64_MAX)[0]
    assert len(got) == len(want) > 4
    for g, w in zip(got, want):
        assert g[:3] == _ref_records(w) and g[3] == w.observed
    B.close()
