"""numpy restatement of cooc_log_prepare_device, written from its contract in include/cooc.h, and the text
fixtures of the device-ingest tests (built here so that the CPU tests can assert what they hold and the GPU tests
use the same bytes)."""
from __future__ import annotations

import numpy as np

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
INT64_MIN, INT64_MAX = -2**63, 2**63 - 1


class BadRecord(Exception):
    def __init__(self, index: int):
        super().__init__(f"record {index}")
        self.index = index


def late_flags(ts: np.ndarray, W: int) -> np.ndarray:
    """Record i of block b = i // W is late iff ts[i] = Long.MIN_VALUE, or b >= 1 and ts[i] < m_b, the largest
    timestamp of the blocks before b (late records included).  W = 0: the first rule only."""
    ts = np.asarray(ts, np.int64)
    late = ts == INT64_MIN
    if W > 0 and len(ts):
        starts = np.arange(0, len(ts), W)
        bmax = np.maximum.reduceat(ts, starts)
        m = np.maximum.accumulate(bmax)  # through block b
        b = np.arange(len(ts)) // W
        has = b >= 1
        late[has] |= ts[has] < m[b[has] - 1]
    return late


def window_end(ts: np.ndarray, size: int) -> np.ndarray:
    """maxTimestamp = ts - (ts + size) % size + size - 1 with Java's remainder (the sign of the dividend)."""
    ts = np.asarray(ts, np.int64)
    return ts - np.fmod(ts + size, size) + size - 1


def prepare(users, items, ts, W: int, size: int, n_items: int) -> dict:
    users = np.asarray(users, np.int32)
    items = np.asarray(items, np.int32)
    ts = np.asarray(ts, np.int64)
    n = len(ts)
    assert W >= 0 and len(users) == n and len(items) == n
    late = late_flags(ts, W)
    kept = np.flatnonzero(~late)
    lo, hi = INT64_MIN + 2 * size, INT64_MAX - 2 * size
    bad = [int(i) for i in kept if not (0 <= items[i] < n_items) or not (lo <= int(ts[i]) <= hi)]
    if bad:
        raise BadRecord(bad[0])
    we = window_end(ts[kept], size)
    fire = kept[np.argsort(we, kind="stable")]  # ascending window end, arrival order within a window
    wts, first = np.unique(window_end(ts[fire], size), return_index=True)
    user_ids, rec_user = np.unique(users[fire], return_inverse=True)  # ascending as signed int32
    csr = np.argsort(rec_user, kind="stable")  # by user, then firing order
    return {
        "n_kept": len(kept), "n_late": int(late.sum()), "n_users": len(user_ids), "n_windows": len(wts),
        "late": late, "fire": fire,
        "rec_user": rec_user.astype(np.int32), "rec_item": items[fire],
        "user_ids": user_ids.astype(np.int32),
        "user_ptr": np.concatenate([[0], np.cumsum(np.bincount(rec_user, minlength=len(user_ids)))]).astype(np.int64),
        "user_items": items[fire][csr],
        "window_ptr": np.concatenate([first, [len(kept)]]).astype(np.int64),
        "window_ts": wts.astype(np.int64),
    }


def pair_counts(user_ptr, user_items, cut: int = 0) -> dict:
    """{(a, b): count} over every ordered pair of distinct positions of every user's (first `cut`) items."""
    out: dict = {}
    for u in range(len(user_ptr) - 1):
        h = [int(x) for x in user_items[user_ptr[u]:user_ptr[u + 1]]]
        if cut:
            h = h[:cut]
        for p, a in enumerate(h):
            for q, b in enumerate(h):
                if p != q:
                    out[(a, b)] = out.get((a, b), 0) + 1
    return out


# ---- the hand-written log: window 1000 ms, W = 4, n_items = 10; every output stated by hand --------------------
HAND_SIZE, HAND_W, HAND_ITEMS = 1000, 4, 10
HAND_LOG = [  # (user, item, ts)
    (7, 3, 100), (-2, 1, 1500), (7, 4, 900), (5, 0, 1200),     # block 0: nothing before it, all kept; m_1 = 1500
    (7, 2, 1500), (5, 9, 1499), (9, 5, 3200), (-2, 6, 3100),   # block 1: 1500 = m_1 kept, 1499 late; m_2 = 3200
    (9, 7, 3199), (5, 8, 3200), (7, 1, 3999), (9, 0, 3500),    # block 2: 3199 late, 3200 = m_2 kept
]
HAND_WANT = {
    "n_kept": 10, "n_late": 2, "n_users": 4, "n_windows": 3,
    "fire": [0, 2, 1, 3, 4, 6, 7, 9, 10, 11],  # windows 999 | 1999 | 3999 (none ends at 2999: a gap)
    "rec_item": [3, 4, 1, 0, 2, 5, 6, 8, 1, 0],
    "user_ids": [-2, 5, 7, 9],
    "rec_user": [2, 2, 0, 1, 2, 3, 0, 1, 2, 3],
    "window_ptr": [0, 2, 5, 10],
    "window_ts": [999, 1999, 3999],
    "user_ptr": [0, 2, 4, 8, 10],
    "user_items": [1, 6, 0, 8, 3, 4, 2, 1, 5, 0],  # user 7 has records in all three windows
}


# ---- logs of the end-to-end tests ------------------------------------------------------------------------------
def jitter_log(seed: int, n: int, n_users: int, n_items: int, spread: int = 1, negative_users: bool = True):
    """An ascending log (3 ms per record) in which 30% of the records are up to 3 s behind: with blocks of 500
    records about a fifth of it is late.  Users +-, items zipf-like times `spread`."""
    rng = np.random.default_rng(seed)
    users = rng.integers(0, n_users, n).astype(np.int32) * 7 - (3 * n_users if negative_users else 0)
    items = (np.minimum(rng.zipf(1.2, n) - 1, n_items // spread - 1) * spread).astype(np.int32)
    behind = np.where(rng.random(n) < 0.3, rng.integers(0, 3000, n), 0)
    ts = (10_000 + 3 * np.arange(n) - behind).astype(np.int64)
    return users.astype(np.int32), items, ts


def to_text(users, items, ts, eol: str = "\n") -> bytes:
    return "".join(f"{u},{i},{t}{eol}" for u, i, t in zip(users, items, ts)).encode()


# ---- text fixtures of the device parser ------------------------------------------------------------------------
BOUNDARIES = (256, 1024, 4096, 16384)


def _side(j: int) -> int:
    """which side of the boundary 256 j gets the line break: 1 = its last byte before, 0 = its first byte after"""
    return bin(j).count("1") & 1


def cycling_text(total: int = 70_000) -> bytes:
    """Valid lines whose lengths cycle, steered (by ignored fourth fields) so that every multiple m of 256 has a
    '\\n' at m - 1 or at m, the side chosen by the parity of the bits of m / 256: both sides occur for the multiples
    of 256, 1,024, 4,096 and 16,384."""
    out, pos, k = [], 0, 0
    while pos < total:
        base = f"{(k * 7919) % 100_000 - 50_000},{k % 300},{1_000_000 + 37 * k}"
        j = pos // 256 + 1
        target = 256 * j - _side(j)
        d = target - pos  # the line's length that puts its '\n' on the target
        assert d >= len(base)
        c = d if d <= 70 else len(base) + k % 17
        pad = c - len(base)
        line = base + ("," + "9" * (pad - 1) if pad else "")
        out.append(line + "\n")
        pos += c + 1
        k += 1
    return "".join(out).encode()


SPECIAL_TEXT = (b"1,2,3\r\n+5,-0,7,extra,fields\r\n-2147483648,2147483647,-9223372036854775808\r\n"
                b"2147483647,0,9223372036854775807\r\n0005,007,+0009\r\n1,2,3,,,\r\n7,8,9")  # no final newline
SPECIAL_WANT = ([1, 5, INT32_MIN, INT32_MAX, 5, 1, 7], [2, 0, INT32_MAX, 0, 7, 2, 8],
                [3, 7, INT64_MIN, INT64_MAX, 9, 3, 9])
LONG_LINE_TEXT = b"1,2,3\n" + b"4,5,6," + b"x," * 9_997 + b"\n7,8,9\n"  # one 20,000-byte line of ignored fields
LONG_LINE_WANT = ([1, 4, 7], [2, 5, 8], [3, 6, 9])

REJECTS = {  # the dictated rejects: each is one line the host parser refuses
    "int_overflow": b"2147483648,1,1",
    "int_underflow": b"1,-2147483649,1",
    "long_overflow": b"1,1,9223372036854775808",
    "long_underflow": b"1,1,-9223372036854775809",
    "empty_field": b"1,,3",
    "two_fields": b"1,2",
    "space": b"1, 2,3",
    "lone_sign": b"1,-,3",
    "letter": b"1,2,3a",
    "empty_line": b"",
}
N_VALID = 9  # lines of a reject text


def reject_text(bad: bytes, at: int, bad2: bytes | None = None, at2: int = -1) -> bytes:
    lines = [f"{k},{k + 1},{k + 2}".encode() for k in range(N_VALID)]
    lines[at] = bad
    if bad2 is not None:
        lines[at2] = bad2
    return b"\n".join(lines) + b"\n"
