"""The snapshot blob restated in numpy, for the rescaling tests: parse / build with the documented
layout and checksums (per section the sum over its 8-byte words w_i of splitmix64(w_i ^ i) mod 2^64; the header's
sum over the 664 header + directory bytes with its own word taken as 0), and the rescaling rule itself as numpy
over sections: split() cuts a world-1 blob into the blobs W subtasks would have taken, expected_part() is what
cooc_restore_finish_parts followed by a snapshot must give for one rank of a new world, byte for byte.  No
library code is involved, so the tests compare the library against an independent statement of the rule."""
import struct

import numpy as np

HEADER, ENTRY, N_SECTIONS = 64, 40, 15
MAGIC, FORMAT = 0x31504E53434F4F43, 1
INT64_MIN = -(2**63)
SCALARS, USER_IDS, HIST_PTR, HIST_ITEMS, ROW_IDS, ROW_PTR, ROW_COLS, ROW_CNTS, ROW_SUMS = range(1, 10)
XSUM_IDS, XSUM_VALS, PEND_TS, PEND_PTR, PEND_USERS, PEND_ITEMS = range(10, 16)
DTYPES = {SCALARS: "<i8", USER_IDS: "<i4", HIST_PTR: "<i8", HIST_ITEMS: "<i4", ROW_IDS: "<i4", ROW_PTR: "<i8",
          ROW_COLS: "<i4", ROW_CNTS: "<u4", ROW_SUMS: "<i8", XSUM_IDS: "<i4", XSUM_VALS: "<i8", PEND_TS: "<i8",
          PEND_PTR: "<i8", PEND_USERS: "<i4", PEND_ITEMS: "<i4"}
# the scalar section's words
OBSERVED_EXACT, OBSERVED_REF, ROWSUM_ACC, RESCORED_ITEMS, LATE_ELEMENTS, WATERMARK, AGREED, REGATHER, SCAL2, SCAL3 = range(10)
SCALAR_WORDS = 16
ADDITIVE = (OBSERVED_EXACT, ROWSUM_ACC, RESCORED_ITEMS, LATE_ELEMENTS)
JOB_WIDE = (OBSERVED_REF, SCAL2, SCAL3)
FIELDS = ("n_items", "user_cut", "window_size_ms", "rank", "world")


def _splitmix64(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def checksum(data: bytes) -> int:
    w = np.frombuffer(data, "<u8")
    with np.errstate(over="ignore"):
        return int(_splitmix64(w ^ np.arange(len(w), dtype=np.uint64)).sum(dtype=np.uint64))


def parse(blob: bytes):
    """-> (fields, sections): fields = {n_items, user_cut, window_size_ms, rank, world}, sections = {kind: array}"""
    magic, fmt, n_sec, total, n_items, user_cut, window, rank, world, _, reserved = struct.unpack_from("<QiiqiiqiiQQ", blob, 0)
    assert (magic, fmt, n_sec, total, reserved) == (MAGIC, FORMAT, N_SECTIONS, len(blob), 0)
    fields = dict(n_items=n_items, user_cut=user_cut, window_size_ms=window, rank=rank, world=world)
    sections = {}
    for k in range(N_SECTIONS):
        kind, elem, off, nbytes, count, _ = struct.unpack_from("<iiqqqQ", blob, HEADER + ENTRY * k)
        assert kind == k + 1 and elem == np.dtype(DTYPES[kind]).itemsize and nbytes == count * elem
        sections[kind] = np.frombuffer(blob, DTYPES[kind], count, off).copy()
    return fields, sections


def build(fields, sections) -> bytes:
    """The canonical blob of these header fields and 15 sections: back to back in kind order, each 8-byte aligned
    and zero-padded, checksummed, the header sealed last."""
    body, entries, off = [], [], HEADER + ENTRY * N_SECTIONS
    for kind in range(1, N_SECTIONS + 1):
        a = np.ascontiguousarray(sections[kind], DTYPES[kind])
        raw = a.tobytes()
        raw += bytes(-len(raw) % 8)
        entries.append((kind, a.dtype.itemsize, off, a.nbytes, len(a), checksum(raw)))
        body.append(raw)
        off += len(raw)
    head = bytearray(HEADER + ENTRY * N_SECTIONS)
    struct.pack_into("<QiiqiiqiiQQ", head, 0, MAGIC, FORMAT, N_SECTIONS, off, fields["n_items"], fields["user_cut"],
                     fields["window_size_ms"], fields["rank"], fields["world"], 0, 0)
    for k, e in enumerate(entries):
        struct.pack_into("<iiqqqQ", head, HEADER + ENTRY * k, *e)
    struct.pack_into("<Q", head, 48, checksum(bytes(head)))
    return bytes(head) + b"".join(body)


def empty_sections():
    s = {k: np.zeros(0, DTYPES[k]) for k in DTYPES}
    s[SCALARS] = np.zeros(SCALAR_WORDS, "<i8")
    s[SCALARS][WATERMARK] = s[SCALARS][AGREED] = INT64_MIN
    for k in (HIST_PTR, ROW_PTR, PEND_PTR):
        s[k] = np.zeros(1, "<i8")
    return s


def take_lists(ptr, datas, idx):
    """Lists idx (in that order) of the lists ptr over the parallel arrays datas -> (new ptr, new arrays)."""
    ptr = np.asarray(ptr, np.int64)
    idx = np.asarray(idx, np.int64)
    lens = ptr[idx + 1] - ptr[idx]
    new_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pos = np.repeat(ptr[idx] - new_ptr[:-1], lens) + np.arange(new_ptr[-1], dtype=np.int64)
    return new_ptr, [np.asarray(d)[pos] for d in datas]


def _pending(windows):
    """{ts: (users, items)} -> sections 12..15, windows without a record dropped"""
    ts = sorted(t for t, (u, _) in windows.items() if len(u))
    ptr = np.concatenate([[0], np.cumsum([len(windows[t][0]) for t in ts])]).astype(np.int64)
    cat = lambda j: np.concatenate([windows[t][j] for t in ts]).astype(np.int32) if ts else np.zeros(0, np.int32)
    return {PEND_TS: np.array(ts, np.int64), PEND_PTR: ptr, PEND_USERS: cat(0), PEND_ITEMS: cat(1)}


def _windows(s):
    return [(int(t), s[PEND_USERS][s[PEND_PTR][k]:s[PEND_PTR][k + 1]], s[PEND_ITEMS][s[PEND_PTR][k]:s[PEND_PTR][k + 1]])
            for k, t in enumerate(s[PEND_TS])]


def uneven_shares(v, W):
    """v >= 0 as W non-negative shares that differ: v // 3, v // 9, ..., the rest on the last part"""
    shares = [int(v) // 3 ** (i + 1) for i in range(W - 1)]
    return shares + [int(v) - sum(shares)]


def split(blob1, W, user_part_of):
    """The world-1 blob as the W blobs a job of W subtasks would have taken in the same logical state: rows by
    a mod W, users by user_part_of (ids array -> parts array; the old routing is arbitrary), every part with every
    other part's row sums in sections 10 / 11, the additive accumulators split unevenly, the job-wide scalars and
    the watermark everywhere, agreed = the watermark when W > 1.  -> list of W blobs"""
    f, s = parse(blob1)
    assert (f["rank"], f["world"]) == (0, 1)
    upart = np.asarray(user_part_of(s[USER_IDS]), np.int64) if len(s[USER_IDS]) else np.zeros(0, np.int64)
    ppart = np.asarray(user_part_of(s[PEND_USERS]), np.int64) if len(s[PEND_USERS]) else np.zeros(0, np.int64)
    shares = {k: uneven_shares(s[SCALARS][k], W) for k in ADDITIVE}
    out = []
    for r in range(W):
        p = empty_sections()
        sc = s[SCALARS].copy()
        for k in ADDITIVE:
            sc[k] = shares[k][r]
        if W > 1:
            sc[AGREED] = sc[WATERMARK]
        sc[REGATHER] = 0
        p[SCALARS] = sc
        ui = np.flatnonzero(upart == r)
        p[USER_IDS] = s[USER_IDS][ui]
        p[HIST_PTR], (p[HIST_ITEMS],) = take_lists(s[HIST_PTR], [s[HIST_ITEMS]], ui)
        own = s[ROW_IDS] % W == r
        ri = np.flatnonzero(own)
        p[ROW_IDS], p[ROW_SUMS] = s[ROW_IDS][ri], s[ROW_SUMS][ri]
        p[ROW_PTR], (p[ROW_COLS], p[ROW_CNTS]) = take_lists(s[ROW_PTR], [s[ROW_COLS], s[ROW_CNTS]], ri)
        if W > 1:
            p[XSUM_IDS], p[XSUM_VALS] = s[ROW_IDS][~own], s[ROW_SUMS][~own]
        windows = {}
        for k, t in enumerate(s[PEND_TS]):
            sl = slice(int(s[PEND_PTR][k]), int(s[PEND_PTR][k + 1]))
            m = ppart[sl] == r
            windows[int(t)] = (s[PEND_USERS][sl][m], s[PEND_ITEMS][sl][m])
        p.update(_pending(windows))
        out.append(build(dict(f, rank=r, world=W), p))
    return out


def expected_part(parts, rank, world, keep):
    """What rank `rank` of a new job of `world` subtasks holds after cooc_restore_finish_parts of these blobs (ALL
    blobs of one checkpoint, in rank order), as the blob its snapshot gives.  keep: user ids array -> bool array,
    the users this rank keeps."""
    parsed = [parse(b) for b in parts]
    f0, s0 = parsed[0]
    out = empty_sections()
    # histories: the kept users of all parts in ascending id order
    ids = np.concatenate([s[USER_IDS] for _, s in parsed])
    lens = np.concatenate([np.diff(s[HIST_PTR]) for _, s in parsed])
    items = np.concatenate([s[HIST_ITEMS] for _, s in parsed])
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert len(np.unique(ids)) == len(ids)
    order = np.argsort(ids, kind="stable")
    order = order[np.asarray(keep(ids[order]), bool)] if len(order) else order
    out[USER_IDS] = ids[order]
    out[HIST_PTR], (out[HIST_ITEMS],) = take_lists(ptr, [items], order)
    # rows a with a mod world == rank from whichever part holds them; the others' row sums when world > 1
    rids = np.concatenate([s[ROW_IDS] for _, s in parsed])
    rsum = np.concatenate([s[ROW_SUMS] for _, s in parsed])
    rlen = np.concatenate([np.diff(s[ROW_PTR]) for _, s in parsed])
    rptr = np.concatenate([[0], np.cumsum(rlen)]).astype(np.int64)
    cols = np.concatenate([s[ROW_COLS] for _, s in parsed])
    cnts = np.concatenate([s[ROW_CNTS] for _, s in parsed])
    rorder = np.argsort(rids, kind="stable")
    mine = rids[rorder] % world == rank
    out[ROW_IDS], out[ROW_SUMS] = rids[rorder][mine], rsum[rorder][mine]
    out[ROW_PTR], (out[ROW_COLS], out[ROW_CNTS]) = take_lists(rptr, [cols, cnts], rorder[mine])
    if world > 1:
        out[XSUM_IDS], out[XSUM_VALS] = rids[rorder][~mine], rsum[rorder][~mine]
    # pending windows: the union by maxTimestamp, the kept records of part 0, then part 1, ...
    windows = {}
    for _, s in parsed:
        for t, u, it in _windows(s):
            m = np.asarray(keep(u), bool)
            pu, pi = windows.get(t, (np.zeros(0, np.int32), np.zeros(0, np.int32)))
            windows[t] = (np.concatenate([pu, u[m]]), np.concatenate([pi, it[m]]))
    out.update(_pending(windows))
    sc = np.zeros(SCALAR_WORDS, np.int64)
    for k in JOB_WIDE:
        sc[k] = s0[SCALARS][k]
    if rank == 0:
        for k in ADDITIVE:
            sc[k] = sum(int(s[SCALARS][k]) for _, s in parsed)
    sc[WATERMARK] = s0[SCALARS][WATERMARK]
    sc[AGREED] = sc[WATERMARK] if world > 1 else INT64_MIN
    out[SCALARS] = sc
    return build(dict(f0, rank=rank, world=world), out)


def keep_all(u):
    return np.ones(len(u), bool)


def keep_mod(world, rank):
    return lambda u: np.asarray(u, np.int64) % world == rank
