"""Rescaling: all blobs of one checkpoint restored into another parallelism (cooc_restore_begin_parts ..
cooc_restore_finish_parts), single process, world-1 destination.  The expected bytes come from tests/_snapblob.py,
numpy over sections with no library code.

Rows of a blob have at most n_items entries (columns strictly ascending), so at M = 300 the dictated row lengths
stop at the full row of 300; the lengths 2,047 .. 4,097 reach the dense destination at M = 4,200 and the slabs at
M = 40,500.  Needs an MI355X.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import _snapblob as sb
from tests._helpers import INT64_MAX

pytestmark = pytest.mark.gpu

CHUNK = 5000
BIG_USER = 2**26 + 3


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _operator(pkg, M, planner="auto"):
    return pkg.NonSampledUserInteractionCounterOneInputStreamOperator(1, "SECONDS", n_items=M, top_k=10, planner=planner)


@functools.lru_cache(maxsize=None)
def _log(M):
    from flink_cooccurrence_amd import datagen

    d = datagen.config_c1(seed=5, U=2000, M=M, mean=20.0)
    users, items, ts = datagen.to_records(d["user_ptr"], d["items"], d["ts"])
    n_chunks = (len(users) + CHUNK - 1) // CHUNK
    return dict(users=users, items=items, ts=ts, n_chunks=n_chunks, mid=n_chunks // 2)


def _feed(op, R, c0, c1, final=False):
    got = []
    for c in range(c0, c1):
        sl = slice(c * CHUNK, (c + 1) * CHUNK)
        op.process_elements(R["users"][sl], R["items"][sl], R["ts"][sl])
        got += op.process_watermark(int(R["ts"][sl][-1]) - 1)
    if final:
        got += op.process_watermark(INT64_MAX)
    return got


@functools.lru_cache(maxsize=None)
def _half(pkg, M, planner="auto"):
    """The blob of a world-1 operator after the first half of the log, records pending."""
    A = _operator(pkg, M, planner)
    _feed(A, _log(M), 0, _log(M)["mid"])
    blob = A.snapshot()
    info = A.core.last_snapshot_info
    A.close()
    assert info["pending_records"] > 0 and info["n_users"] > 100 and info["global_rows"] > 100
    return blob


def _hash_part(W):
    """an arbitrary old routing: a hash of the id, not mod"""
    def part_of(u):
        h = (np.asarray(u, np.int64).astype(np.uint64) * np.uint64(2654435761)) >> np.uint64(7)
        return (h % np.uint64(W)).astype(np.int64)
    return part_of


def _restored(pkg, M, parts, route=None, planner="auto", **kw):
    op = _operator(pkg, M, planner)
    info = op.restore_parts(parts, route, **kw)
    return op, info


def _snapshot_of(pkg, M, parts, route=None, planner="auto"):
    op, info = _restored(pkg, M, parts, route, planner)
    blob = op.snapshot()
    assert info == op.core.last_snapshot_info == pkg.CooccurrenceCore.snapshot_info(blob)
    op.close()
    return blob


# ---- 0. the helper is pinned to the library ------------------------------------------------------------
@pytest.mark.parametrize("M", [300, 40_500])
def test_helper_rebuilds_real_blobs(pkg, torch_cuda, M):
    b = _half(pkg, M)
    f, s = sb.parse(b)
    assert sb.build(f, s) == b
    assert (f["n_items"], f["rank"], f["world"]) == (M, 0, 1) and len(s[sb.ROW_IDS]) > 0 and len(s[sb.PEND_USERS]) > 0


# ---- 1. split and merge --------------------------------------------------------------------------------
def _per_window_sorted(s):
    """the pending records of every window, stably sorted by user: the order across users removed, the order of one
    user's records kept"""
    out = []
    for k in range(len(s[sb.PEND_TS])):
        sl = slice(int(s[sb.PEND_PTR][k]), int(s[sb.PEND_PTR][k + 1]))
        o = np.argsort(s[sb.PEND_USERS][sl], kind="stable")
        out.append((s[sb.PEND_USERS][sl][o].tolist(), s[sb.PEND_ITEMS][sl][o].tolist()))
    return out


@pytest.mark.parametrize("W", [2, 3, 5])
@pytest.mark.parametrize("M", [300, 40_500])
def test_split_and_merge(pkg, torch_cuda, M, W):
    b = _half(pkg, M)
    parts = sb.split(b, W, _hash_part(W))
    heads = [sb.parse(p) for p in parts]
    assert all(len(s[sb.USER_IDS]) > 0 and len(s[sb.ROW_IDS]) > 0 for _, s in heads)
    assert len({int(s[sb.SCALARS][sb.OBSERVED_EXACT]) for _, s in heads}) == W  # the accumulators split unevenly
    assert all(s[sb.SCALARS][sb.AGREED] == s[sb.SCALARS][sb.WATERMARK] for _, s in heads)
    want = sb.expected_part(parts, 0, 1, sb.keep_all)
    got = _snapshot_of(pkg, M, parts)
    assert got == want
    # against b: only the order of records within pending windows may differ
    (fb, s_b), (fg, s_g) = sb.parse(b), sb.parse(got)
    assert fb == fg
    for kind in range(1, sb.N_SECTIONS + 1):
        if kind not in (sb.PEND_USERS, sb.PEND_ITEMS):
            assert np.array_equal(s_b[kind], s_g[kind]), f"section {kind}"
    assert _per_window_sorted(s_b) == _per_window_sorted(s_g)
    # idempotence: the result split again and merged gives the same bytes
    assert _snapshot_of(pkg, M, sb.split(got, W, _hash_part(W))) == got


def test_one_part_is_the_plain_restore(pkg, torch_cuda):
    b = _half(pkg, 300)
    assert _snapshot_of(pkg, 300, [b]) == b
    assert _snapshot_of(pkg, 300, [b], planner="large") == b


def test_ranged_part_writes(pkg, torch_cuda):
    """parts written in 4,093-byte ranges"""
    b = _half(pkg, 300)
    parts = sb.split(b, 3, _hash_part(3))
    op, _ = _restored(pkg, 300, parts, range_bytes=4093)
    assert op.snapshot() == sb.expected_part(parts, 0, 1, sb.keep_all)
    op.close()


# ---- 2. continue the stream ----------------------------------------------------------------------------
def _assert_same_window(g, w):
    for name in ("ts", "observed"):
        assert getattr(g, name) == getattr(w, name)
    for name in ("rows", "row_ptr", "cols", "exact", "v16", "rs_items", "rs_exact", "rs_v32", "topk_rows", "topk_sizes"):
        assert np.array_equal(getattr(g, name), getattr(w, name)), name
    for r in range(len(w.topk_rows)):
        n = int(w.topk_sizes[r])
        assert np.array_equal(g.topk_values[r, :n], w.topk_values[r, :n])
        assert np.array_equal(g.topk_scores[r, :n], w.topk_scores[r, :n], equal_nan=True)


@pytest.mark.parametrize("M,src,dst", [(300, "auto", "auto"), (40_500, "auto", "auto"), (300, "auto", "large"),
                                       (300, "large", "auto")])
def test_continue_the_stream(pkg, torch_cuda, M, src, dst):
    """The rest of the stream to the rescaled context and to a twin restored plainly from b: every window, the
    accumulators and the global row sums are equal.  (300, auto -> large) is dense -> slabs, (300, large -> auto)
    slabs -> dense."""
    R = _log(M)
    b = _half(pkg, M, src)
    twin = _operator(pkg, M, dst)
    twin.restore(b)
    op, _ = _restored(pkg, M, sb.split(b, 3, _hash_part(3)), planner=dst)
    want = _feed(twin, R, R["mid"], R["n_chunks"], final=True)
    got = _feed(op, R, R["mid"], R["n_chunks"], final=True)
    assert len(got) == len(want) >= 5
    for g, w in zip(got, want):
        _assert_same_window(g, w)
    assert op.accumulators() == twin.accumulators()
    for x, y in zip(op.core.global_rowsums(), twin.core.global_rowsums()):
        assert np.array_equal(x, y)
    assert op.snapshot() == twin.snapshot()
    op.close()
    twin.close()


# ---- 3. dictated shapes --------------------------------------------------------------------------------
HIST_LENS = {-5: 1, 3: 15, 63: 16, 64: 17, 100: 2047, 199: 2048, 200: 2049, BIG_USER: 5000}
USER_PART = {-5: 0, 63: 0, 100: 0, 200: 0, 3: 1, 64: 1, 199: 1, BIG_USER: 1, 7: 1}
WATERMARK = 999
T1, T2, T3 = 1999, 2999, 3999


def _row_lens(M):
    if M == 300:
        return [1, 63, 64, 65, 299, 300]
    return [1, 2047, 2048, 2049] + ([4097] if M >= 4200 else [])


@functools.lru_cache(maxsize=None)
def _synthetic(M):
    """Four parts built by hand: part 0 has rows and users, part 1 users but no rows, part 2 rows but no users,
    part 3 is wholly empty (but for the other parts' row sums).  Rows of the dictated lengths alternate between
    parts 0 and 2, counts reach past 65,536; histories of the dictated lengths, user ids negative, across the
    bitmap's word boundary and outside the dense table; window T1 is pending in part 0 only, T2 in parts 0 and 1,
    T3 holds only users that the bitmap of test_bitmap_route drops."""
    W = 4
    rng = np.random.default_rng(3)
    rows = {}  # a -> (cols, cnts)
    for j, n in enumerate(_row_lens(M)):
        a = 8 * j + (0 if j % 2 == 0 else 2) + 16  # a mod 4 is 0 or 2
        cols = np.sort(rng.choice(M, n, replace=False)).astype(np.int32)
        cnts = (1 + (np.arange(n, dtype=np.int64) * 7919 + j) % 100_000).astype(np.uint32)
        rows[a] = (cols, cnts)
    assert max(int(c.max()) for _, c in rows.values()) >= 65_536
    hist = {u: rng.integers(0, M, n).astype(np.int32) for u, n in HIST_LENS.items()}
    pend = {0: {T1: ([63, 100, 63], [1, 2, 3]), T2: ([63, -5], [4, 5]), T3: ([100, 200, -5], [6, 7, 8])},
            1: {T2: ([64, 3, 7], [9, 10, 11]), T3: ([BIG_USER], [12])}}
    all_ids = np.array(sorted(rows), np.int32)
    all_sums = np.array([int(rows[a][1].sum(dtype=np.int64)) for a in sorted(rows)], np.int64)
    parts = []
    for r in range(W):
        s = sb.empty_sections()
        sc = s[sb.SCALARS]
        sc[sb.OBSERVED_EXACT], sc[sb.ROWSUM_ACC], sc[sb.RESCORED_ITEMS], sc[sb.LATE_ELEMENTS] = 1000 + r, 77 * r, 5 + r, r
        sc[sb.OBSERVED_REF], sc[sb.SCAL2], sc[sb.SCAL3] = 4242, 4242, 99_999
        sc[sb.WATERMARK] = sc[sb.AGREED] = WATERMARK
        users = sorted(u for u in HIST_LENS if USER_PART[u] == r)
        s[sb.USER_IDS] = np.array(users, np.int32)
        s[sb.HIST_PTR] = np.concatenate([[0], np.cumsum([HIST_LENS[u] for u in users])]).astype(np.int64)
        s[sb.HIST_ITEMS] = np.concatenate([hist[u] for u in users]) if users else np.zeros(0, np.int32)
        own = all_ids % W == r
        mine = [int(a) for a in all_ids[own]]
        s[sb.ROW_IDS], s[sb.ROW_SUMS] = all_ids[own], all_sums[own]
        s[sb.ROW_PTR] = np.concatenate([[0], np.cumsum([len(rows[a][0]) for a in mine])]).astype(np.int64)
        s[sb.ROW_COLS] = np.concatenate([rows[a][0] for a in mine]) if mine else np.zeros(0, np.int32)
        s[sb.ROW_CNTS] = np.concatenate([rows[a][1] for a in mine]) if mine else np.zeros(0, np.uint32)
        s[sb.XSUM_IDS], s[sb.XSUM_VALS] = all_ids[~own], all_sums[~own]
        wins = pend.get(r, {})
        ts = sorted(wins)
        s[sb.PEND_TS] = np.array(ts, np.int64)
        s[sb.PEND_PTR] = np.concatenate([[0], np.cumsum([len(wins[t][0]) for t in ts])]).astype(np.int64)
        s[sb.PEND_USERS] = np.array([u for t in ts for u in wins[t][0]], np.int32)
        s[sb.PEND_ITEMS] = np.array([i for t in ts for i in wins[t][1]], np.int32)
        parts.append(sb.build(dict(n_items=M, user_cut=0, window_size_ms=1000, rank=r, world=W), s))
    return tuple(parts), rows, hist


@pytest.mark.parametrize("M", [300, 4200, 40_500])
def test_dictated_shapes(pkg, torch_cuda, M):
    parts, rows, _ = _synthetic(M)
    infos = [pkg.CooccurrenceCore.snapshot_info(p) for p in parts]
    assert [i["global_rows"] > 0 for i in infos] == [True, False, True, False]
    assert [i["n_users"] > 0 for i in infos] == [True, True, False, False]
    want = sb.expected_part(parts, 0, 1, sb.keep_all)
    op, info = _restored(pkg, M, list(parts))
    assert info == pkg.CooccurrenceCore.snapshot_info(want)
    assert info["n_users"] == sum(i["n_users"] for i in infos)
    assert info["history_items"] == sum(i["history_items"] for i in infos)
    assert info["pending_windows"] == 3  # T1 from part 0 alone, T2 and T3 from both
    for a, (cols, cnts) in rows.items():  # the installed rows, read back one by one
        c, n, _ = op.core.global_row(a)
        assert np.array_equal(c, cols) and np.array_equal(n, cnts), f"row {a}"
    assert len(op.core.global_row(17)[0]) == 0
    assert op.snapshot() == want
    f, s = sb.parse(want)
    k = s[sb.PEND_TS].tolist().index(T2)
    assert s[sb.PEND_USERS][s[sb.PEND_PTR][k]:s[sb.PEND_PTR][k + 1]].tolist() == [63, -5, 64, 3, 7]  # part 0, then part 1
    assert op.accumulators()["rescorer_observed"] == 4242
    op.close()


# ---- 4. the bitmap route -------------------------------------------------------------------------------
N_BITS = 200
KEPT = (3, 7, 63, 64, 199)  # 199 = n_bits - 1; users 200 = n_bits, 100, -5 and 2^26 + 3 are dropped


@pytest.mark.parametrize("M", [300, 40_500])
def test_bitmap_route(pkg, torch_cuda, M):
    from flink_cooccurrence_amd import _lib

    parts, _, hist = _synthetic(M)
    bitmap = np.zeros(N_BITS, bool)
    bitmap[list(KEPT)] = True
    keep = lambda u: np.isin(np.asarray(u), KEPT)
    want = sb.expected_part(parts, 0, 1, keep)
    # a route whose words go on past n_bits with every bit set (bit 200 = n_bits and bit 2^26 + 3 among them):
    # only the u < n_bits test can drop users 200 and 2^26 + 3
    words = np.full(BIG_USER // 64 + 2, np.uint64(2**64 - 1))
    words[:(N_BITS + 63) // 64] = np.frombuffer(np.packbits(np.concatenate([bitmap, np.ones(56, bool)]),
                                                            bitorder="little").tobytes(), "<u8")
    assert (int(words[N_BITS // 64]) >> (N_BITS % 64)) & 1 == 1 and (int(words[100 // 64]) >> (100 % 64)) & 1 == 0
    raw = _lib.CoocUserRoute(_lib.COOC_ROUTE_BITMAP, 0, N_BITS, ctypes.c_void_p(words.ctypes.data))
    for route in (bitmap, bitmap.astype(np.uint8), raw):
        op, info = _restored(pkg, M, list(parts), route)
        assert op.snapshot() == want
        op.close()
    f, s = sb.parse(want)
    assert s[sb.USER_IDS].tolist() == [3, 63, 64, 199]  # (7 has pending records only)
    assert info["history_items"] == 15 + 16 + 17 + 2048
    assert np.array_equal(s[sb.HIST_ITEMS][-2048:], hist[199])
    assert s[sb.PEND_TS].tolist() == [T1, T2]  # every record of T3 is dropped by the route, and so is the window
    assert s[sb.PEND_USERS].tolist() == [63, 63, 63, 64, 3, 7]


# ---- 5. refusals ---------------------------------------------------------------------------------------
def _edit_last(parts, edit, fields=None):
    """the last part with its sections edited by edit(sections) and its header fields updated, rebuilt and resealed"""
    f, s = sb.parse(parts[-1])
    if edit:
        edit(s)
    return list(parts[:-1]) + [sb.build(dict(f, **(fields or {})), s)]


def _add_user(s):
    s[sb.USER_IDS] = np.array([63], np.int32)
    s[sb.HIST_PTR] = np.array([0, 1], np.int64)
    s[sb.HIST_ITEMS] = np.array([5], np.int32)


def _add_pending_at_watermark(s):
    s[sb.PEND_TS] = np.array([WATERMARK], np.int64)
    s[sb.PEND_PTR] = np.array([0, 1], np.int64)
    s[sb.PEND_USERS] = np.array([1], np.int32)
    s[sb.PEND_ITEMS] = np.array([1], np.int32)


def _scalar(k, delta, also=None):
    def edit(s):
        s[sb.SCALARS][k] += delta
        if also is not None:
            s[sb.SCALARS][also] += delta
    return edit


def _row_in_wrong_part(parts):
    """row 5 (5 mod 4 = 1) in part 3, and known to every other part's row sums: only its place is wrong"""
    out = []
    for i, p in enumerate(parts):
        f, s = sb.parse(p)
        if i == len(parts) - 1:
            s[sb.ROW_IDS], s[sb.ROW_PTR] = np.array([5], np.int32), np.array([0, 1], np.int64)
            s[sb.ROW_COLS], s[sb.ROW_CNTS], s[sb.ROW_SUMS] = np.array([1], np.int32), np.array([2], np.uint32), np.array([2], np.int64)
        else:
            s[sb.XSUM_IDS] = np.concatenate([[5], s[sb.XSUM_IDS]]).astype(np.int32)
            s[sb.XSUM_VALS] = np.concatenate([[2], s[sb.XSUM_VALS]]).astype(np.int64)
        out.append(sb.build(f, s))
    return out


def _xsum_value_off(s):
    s[sb.XSUM_VALS][0] += 1


def _xsum_missing(s):
    s[sb.XSUM_IDS], s[sb.XSUM_VALS] = s[sb.XSUM_IDS][1:], s[sb.XSUM_VALS][1:]


def _xsum_unowned(s):
    s[sb.XSUM_IDS][-1] = 290  # an item without a row anywhere, in place of a row's: the number of entries stays


def _flip_payload(parts):
    f, s = sb.parse(parts[-1])
    b = bytearray(parts[-1])
    b[sb.HEADER + sb.ENTRY * sb.N_SECTIONS + 3] ^= 0x40  # in the scalars' payload
    return list(parts[:-1]) + [bytes(b)]


FAULTS = {
    "duplicate_user": lambda p: _edit_last(p, _add_user),
    "row_in_wrong_part": _row_in_wrong_part,
    "rank_twice": lambda p: _edit_last(p, None, dict(rank=0)),
    "world_not_n_parts": lambda p: _edit_last(p, None, dict(world=5)),
    "other_n_items": lambda p: _edit_last(p, None, dict(n_items=301)),
    "job_wide_scalar": lambda p: _edit_last(p, _scalar(sb.SCAL2, 1)),
    "watermark": lambda p: _edit_last(p, _scalar(sb.WATERMARK, -1, also=sb.AGREED)),
    "regather": lambda p: _edit_last(p, _scalar(sb.REGATHER, 1)),
    "pending_at_watermark": lambda p: _edit_last(p, _add_pending_at_watermark),
    "xsum_value_off_by_one": lambda p: _edit_last(p, _xsum_value_off),
    "xsum_entry_missing": lambda p: _edit_last(p, _xsum_missing),
    "xsum_entry_unowned": lambda p: _edit_last(p, _xsum_unowned),
    "flipped_payload_byte": _flip_payload,
}


# A fragment of the message of the check that refuses each fault (the last part is part 3).
# row_in_wrong_part sets bit 1 (its place) and with it always bit 2: the misplaced row gets no owner, so the entry
# that the other parts' row sums must hold for it (their number is checked on the host) finds no row.
# xsum_entry_missing never reaches the device: the host check of the entries' number refuses it, which is the check
# meant for a missing entry (k_snap_parts_xsums relies on it); with the number kept it is xsum_entry_unowned.
REFUSED_BY = {
    "duplicate_user": "snapshot parts: a user id in more than one part",
    "row_in_wrong_part": "invalid across parts (checks failed: 3;",
    "rank_twice": "part 3: not taken by the rank of its position",
    "world_not_n_parts": "part 3: its world is not the number of parts",
    "other_n_items": "part 3: snapshot blob: taken with n_items 301",
    "job_wide_scalar": "part 3: a job-wide total differs from part 0's",
    "watermark": "part 3: its watermark is not the job's agreed one",
    "regather": "part 3: taken with a collective step outstanding",
    "pending_at_watermark": "part 3: a window pending at or below its watermark",
    "xsum_value_off_by_one": "invalid across parts (checks failed: 2;",
    "xsum_entry_missing": "part 3: its row sums of other ranks are not as many as the other parts' rows",
    "xsum_entry_unowned": "invalid across parts (checks failed: 2;",
    "flipped_payload_byte": "part 3: snapshot blob: checksum mismatch in section 1",
    "bad_route_kind": "user route: unknown kind",
    "null_bits": "user route: a bitmap of n_bits > 0 needs bits",
}
assert set(REFUSED_BY) == set(FAULTS) | {"bad_route_kind", "null_bits"}


@pytest.mark.parametrize("fault", list(FAULTS) + ["bad_route_kind", "null_bits"])
def test_refusals(pkg, torch_cuda, fault):
    from flink_cooccurrence_amd import _lib

    M = 300
    parts, _, _ = _synthetic(M)
    parts = list(parts)
    op = _operator(pkg, M)
    with pytest.raises(pkg.IllegalArgumentException) as e:
        if fault == "bad_route_kind":
            op.restore_parts(parts, _lib.CoocUserRoute(2, 0, 0, None))
        elif fault == "null_bits":
            op.restore_parts(parts, _lib.CoocUserRoute(_lib.COOC_ROUTE_BITMAP, 0, 10, None))
        else:
            bad = FAULTS[fault](parts)
            assert bad != parts and all(pkg.CooccurrenceCore.snapshot_info(b)["bytes"] == len(b) for b in bad)
            op.restore_parts(bad)
    print(f"refused: {e.value}")
    assert e.value.status == 1 and REFUSED_BY[fault] in str(e.value)
    # the context is empty and usable: the valid parts restore, and the snapshot is the expected one
    op.restore_parts(parts)
    assert op.snapshot() == sb.expected_part(parts, 0, 1, sb.keep_all)
    op.close()


def test_reserved_route_field(pkg, torch_cuda):
    from flink_cooccurrence_amd import _lib

    parts, _, _ = _synthetic(300)
    op = _operator(pkg, 300)
    with pytest.raises(pkg.IllegalArgumentException):
        op.restore_parts(list(parts), _lib.CoocUserRoute(_lib.COOC_ROUTE_MOD, 1, 0, None))
    op.close()


def test_begin_parts_on_used_context(pkg, torch_cuda):
    parts, _, _ = _synthetic(300)
    op = _operator(pkg, 300)
    op.process_element(1, 2, 500)
    with pytest.raises(pkg.IllegalStateException) as e:
        op.restore_parts(list(parts))
    assert e.value.status == 2
    op.close()
    with pkg.CooccurrenceCore(n_items=300, topk=10) as core:
        core.restore_parts(list(parts))
        with pytest.raises(pkg.IllegalStateException):  # the context has state now
            core.restore_parts(list(parts))
        assert core.snapshot() == sb.expected_part(parts, 0, 1, sb.keep_all)
