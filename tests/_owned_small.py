"""cooc_count_owned below 40,320 items (include/cooc.h, "small universes"), for the tests of it: the logs, built
here on the CPU, their split over the ranks, a spawn whose children run under a time limit, and the comparisons
against oracle.closed_form / oracle.rows_topk.  No library code."""
from __future__ import annotations

import time

import numpy as np

M_A, USERS_A, TOPK = 301, 200, 5
CHILD_TIMEOUT_S = 240  # every child of a spawn; a hang fails the test instead of stalling the suite


def _csr(lists):
    up = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    items = np.concatenate([np.asarray(x, np.int32) for x in lists] + [np.zeros(0, np.int32)]).astype(np.int32)
    return up, items


def log_a():
    """M = 301 (divisible by neither 2 nor 3), 200 users, list lengths 0..40 from a Zipf item law over 260 of the
    items in a shuffled order (so some items have no record), a fixed seed; users 0..3 hold 0, 1, 0 and 2 items"""
    rng = np.random.default_rng(20_240_521)
    ids = rng.permutation(M_A)[:260]
    p = 1.0 / np.arange(1, len(ids) + 1) ** 1.1
    p /= p.sum()
    lens = rng.integers(0, 41, USERS_A)
    lens[:4] = [0, 1, 0, 2]
    return _csr([ids[rng.choice(len(ids), size=int(n), p=p)] for n in lens]) + (M_A,)


def log_b(M):
    """M = 2 at three ranks leaves rank 2 without a row (R = 0); M = 7 gives the ranks 3, 2 and 2 rows"""
    if M == 2:
        return _csr([[0, 1], [1, 0, 1], [], [1], [0, 1, 0, 1]]) + (2,)
    rng = np.random.default_rng(77)
    return _csr([rng.integers(0, M, int(n)) for n in rng.integers(0, 6, 23)]) + (M,)


def log_70000():
    """the control at n_items = 70,000 (the large-universe exchange): 300 users, lists of 2..30 Zipf items"""
    rng = np.random.default_rng(4242)
    M = 70_000
    return _csr([np.minimum(rng.zipf(1.3, int(n)) - 1, M - 1) for n in rng.integers(2, 31, 300)]) + (M,)


SPLIT_M, SPLIT_USERS, SPLIT_ITEMS = 2003, 2200, 2000


def log_split():
    """2,200 users, each holding the same 2,000 items of M = 2,003 (every user a rotation of 0..1999): every row
    has 2,200 x 1,999 pairs, above the batch planner's 2^22-pair chunk, so the owner splits it"""
    base = np.arange(SPLIT_ITEMS, dtype=np.int32)
    items = np.concatenate([np.roll(base, u) for u in range(SPLIT_USERS)])
    return np.arange(SPLIT_USERS + 1, dtype=np.int64) * SPLIT_ITEMS, items, SPLIT_M


def shard(up, items, world, rank, ranks_with_users=None):
    """rank's users of a log: user u on rank u mod ranks_with_users (default world; fewer leaves the last ranks
    without users) -> (user_ptr, items)"""
    k = ranks_with_users or world
    lists = [items[up[u]:up[u + 1]] for u in range(len(up) - 1) if u % k == rank]
    return _csr(lists)


def capped(up, items, cut):
    return _csr([items[up[u]:up[u + 1]][:cut] for u in range(len(up) - 1)])


def spawn(worker, args, world, what):
    """torch.multiprocessing.spawn with a time limit over the children: past it they are killed and the test fails"""
    import pytest
    import torch.multiprocessing as mp

    ctx = mp.spawn(worker, args=args, nprocs=world, join=False)
    deadline = time.monotonic() + CHILD_TIMEOUT_S
    while not ctx.join(timeout=2.0):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                if p.is_alive():
                    p.kill()
            pytest.fail(f"{what}: a child ran longer than {CHILD_TIMEOUT_S} s")


def views(data):
    """the reference's views of exact counts / row sums: int16 counts, int32 row sums"""
    d = np.asarray(data, np.int64)
    return d.astype(np.uint64).astype(np.uint16).view(np.int16), d.astype(np.uint64).astype(np.uint32).view(np.int32)


def expected_heaps(oracle, rp, cols, data, rowsums, rows, topk=TOPK):
    """oracle.rows_topk of the given rows, fed the closed form's counts in ascending column order and the whole
    log's row sums -> {row: (values, scores)} in heap order"""
    rows = np.asarray(rows, np.int32)
    hp = np.concatenate([[0], np.cumsum([rp[a + 1] - rp[a] for a in rows])]).astype(np.int64)
    hc = np.concatenate([cols[rp[a]:rp[a + 1]] for a in rows] + [np.zeros(0, np.int32)])
    hv = np.concatenate([views(data[rp[a]:rp[a + 1]])[0] for a in rows] + [np.zeros(0, np.int16)])
    rs32 = views(rowsums)[1]
    sz, v, sc = oracle.rows_topk(rows, hp, hc, hv, rs32, int(rs32.astype(np.int64).sum()), topk)
    return {int(a): (v[j, :sz[j]].copy(), sc[j, :sz[j]].copy()) for j, a in enumerate(rows)}


def assert_union(parts, world, want, key="a"):
    """the ranks' owned results against the closed form `want` = (rp, cols, data, rowsums, observed): rank r's
    non-empty rows are exactly the non-empty rows a with a mod world == r, columns ascending, counts, int64 row sums
    and the cnt16 view equal; every other row empty"""
    rp, cols, data, rowsums, observed = want
    M = len(rp) - 1
    w_nnz = np.diff(rp)
    owner = np.arange(M) % world
    for r, p in enumerate(parts):
        e = p[key]
        mine = owner == r
        nnz = np.diff(e["rp"])
        assert np.all(nnz[~mine] == 0), f"rank {r}: a row owned elsewhere has entries"
        assert np.array_equal(nnz[mine], w_nnz[mine]), f"rank {r}: row lengths"
        assert np.array_equal(e["rowsum"][mine], rowsums[mine]) and np.all(e["rowsum"][~mine] == 0), f"rank {r}"
        for a in np.flatnonzero(mine & (w_nnz > 0)):
            sl, ws = slice(e["rp"][a], e["rp"][a + 1]), slice(rp[a], rp[a + 1])
            assert np.array_equal(e["cols"][sl], cols[ws]), f"row {a}: columns"
            assert np.array_equal(e["cnt"][sl].astype(np.int64), data[ws]), f"row {a}: counts"
            assert np.array_equal(e["cnt16"][sl], views(data[ws])[0]), f"row {a}: cnt16"
        assert e["observed"] == observed, f"rank {r}: info.observed"
        assert e["local_observed"] == int(rowsums[mine].sum()), f"rank {r}: info.local_observed"
    assert sum(p[key]["local_observed"] for p in parts) == observed


def assert_heaps(parts, world, want_heaps, key="a_topk"):
    """every owned row's heap (size, values in heap order, scores) equals the oracle's; rows owned elsewhere and
    rows without entries have size 0"""
    for r, p in enumerate(parts):
        t = p[key]
        for a in range(len(t["sizes"])):
            v, sc = want_heaps.get(a, (np.zeros(0, np.int32), np.zeros(0))) if a % world == r else (
                np.zeros(0, np.int32), np.zeros(0))
            n = int(t["sizes"][a])
            assert n == len(v), f"rank {r}, row {a}: heap size {n} != {len(v)}"
            assert np.array_equal(t["values"][a, :n], v), f"rank {r}, row {a}: heap values"
            assert np.array_equal(t["scores"][a, :n], sc, equal_nan=True), f"rank {r}, row {a}: scores"
