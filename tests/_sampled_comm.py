"""The sampled mode across ranks (include/cooc.h, "sampled mode at world > 1"), for the tests of it: the contract's
data-parallel form restated in pure Python (RankParallel), the dictated log that walks the multi-rank branches, and
the check, made on the model's run alone, that a log reaches each of them (reached).  No library code."""
from __future__ import annotations

from collections import Counter

import numpy as np

import _sampled_model as sm

SEED = 0xC0FFEE
ITEM_CUT, USER_CUT = 5, 2
BRANCHES = "abcdefgh"


class RankParallel:
    """The contract's data-parallel form: h_q[i] records of item i on rank q, base_r[i] = sum_{q<r} h_q[i]; a record
    of i on rank r with rank rho among rank r's records of i is sampled iff count[i] + base_r[i] + rho < item_cut;
    the user stage is local; every rank ends with count[i] += min(sum_q h_q[i], max(0, item_cut - count[i])) -
    sum_q f_q[i].  The counters are kept once per rank, as the ranks keep them."""

    def __init__(self, world: int, item_cut: int, user_cut: int, seed: int):
        self.world, self.item_cut, self.user_cut, self.seed = world, item_cut, user_cut, seed
        self.count = [dict() for _ in range(world)]
        self.H: dict = {}
        self.total: dict = {}
        self.ctr = [Counter() for _ in range(world)]  # rejected, fills, replacements, feedbacks per rank

    def window(self, per_rank):
        W = self.world
        h = [Counter(i for _, i in R) for R in per_rank]
        f = [Counter() for _ in range(W)]
        decisions = []
        for r, R in enumerate(per_rank):
            cnt, rho, ctr = self.count[r], Counter(), self.ctr[r]
            for u, i in R:
                base = sum(h[q][i] for q in range(r))
                sample = cnt.get(i, 0) + base + rho[i] < self.item_cut
                rho[i] += 1
                self.total[u] = self.total.get(u, 0) + 1
                if not sample:
                    ctr["rejected"] += 1
                    decisions.append("r")
                    continue
                H = self.H.setdefault(u, [])
                if len(H) < self.user_cut:
                    H.append(i)
                    ctr["fills"] += 1
                    decisions.append("f")
                    continue
                k = sm.draw(self.seed, u, self.total[u])
                if k < self.user_cut:
                    H[k] = i
                    ctr["replacements"] += 1
                    decisions.append(f"k{k}")
                else:
                    f[r][i] += 1
                    ctr["feedbacks"] += 1
                    decisions.append("b")
        union = set().union(*[set(x) for x in h])
        for cnt in self.count:
            for i in union:
                c = cnt.get(i, 0)
                cnt[i] = c + min(sum(x[i] for x in h), max(0, self.item_cut - c)) - sum(x[i] for x in f)
                assert cnt[i] >= 0
        return decisions


def serial(per_rank):
    """the job's arrival order of a window: R_0 || R_1 || ... (rank-major)"""
    return [rec for R in per_rank for rec in R]


def item_id(idx: int, n_items: int) -> int:
    """item index [0, 300) -> an id spread over the universe: a step coprime to 2 and 3, so that the rows fall on
    every owner (row a on rank a mod world); index 299 is the last item"""
    if idx == 299:
        return n_items - 1
    step = max(1, n_items // 300)
    while step % 6 != 1:
        step -= 1
    return idx * step


def dictated_log(world: int, n_items: int):
    """8 windows, per window one record list per rank (user u on rank u mod world), 130 users, about 2,000 records:
    a random background (users 0..89, item indices 0..189 and 299, replacements, feedbacks, rejections on every
    rank) and, on users and items of their own, the records that walk branches (a)-(h) of the multi-rank window.
    Returns (windows, marks); marks names the dictated users and items of (h)."""
    rng = np.random.default_rng(23)
    last = world - 1
    it = lambda idx: item_id(idx, n_items)  # noqa: E731
    fresh_next = [1002 + r for r in range(world)]  # (1002 = 6 * 167: rank r's ids are 1002 + r + k * world)

    def fresh(rank):  # a user id never used before, on `rank`
        u = fresh_next[rank]
        fresh_next[rank] += world
        return u

    def find(rank, total, want, lo=5000):  # a user on `rank` whose draw at `total` satisfies want
        u = lo
        while True:
            u = sm.find_user_total(SEED, total, want, u)
            if u % world == rank:
                return u
            u += 1

    ia, ic, idd, iq, x, y, z = (it(k) for k in range(200, 207))
    F = find(1, 3, lambda k: k >= USER_CUT)           # full after w0; its third record feeds back
    F2 = find(last, 3, lambda k: k >= USER_CUT, F + 1)
    B = find(1, 3, lambda k: k == 1, F2 + 1)          # full with [x, y]; its third record replaces slot 1
    A = fresh(0)

    def background(n, ranks=None):
        users = rng.integers(0, 90, n)
        idx = np.where(rng.random(n) < 0.6, rng.integers(0, 190, n), np.minimum(rng.zipf(1.3, n) - 1, 49))
        idx = np.where(rng.random(n) < 0.03, 299, idx)
        out = [[] for _ in range(world)]
        for u, k in zip(users.tolist(), idx.tolist()):
            if ranks is None or u % world in ranks:
                out[u % world].append((u, it(k)))
        return out

    W = []
    w = background(350)
    w[1] += [(F, it(207)), (F, it(208)), (B, x), (B, y)]
    w[last] += [(F2, it(209)), (F2, it(210))]
    W.append(w)
    w = background(350)  # (a), (b): the cut of ia falls inside rank 1's records; (c): ic on the last rank only
    w[0] += [(fresh(0), ia) for _ in range(2)]
    w[1] += [(fresh(1), ia) for _ in range(5)]
    w[last] += [(fresh(last), ic) for _ in range(ITEM_CUT)]
    W.append(w)
    w = background(350)  # (c): ic binds on rank 0; (d): idd reaches the cut with a feedback from rank 1
    w[0] += [(fresh(0), ic)] + [(fresh(0), idd) for _ in range(ITEM_CUT - 1)]
    w[1] += [(F, idd)]
    W.append(w)
    w = background(350)  # (d): the feedback reopened the cut of idd for rank 0
    w[0] = [(fresh(0), idd)] + w[0]
    W.append(w)
    W.append(background(200, ranks={0}))  # (e): records on rank 0 only
    w = [[] for _ in range(world)]  # (f): rejections and a feedback, no slot changes
    for r in range(world):
        w[r] += [(fresh(r), ic), (fresh(r), ic)]
    w[last] += [(F2, iq)]
    W.append(w)
    w = [[] for _ in range(world)]  # (g), (h): A fills (x, y) on rank 0, B replaces y on rank 1
    w[0] += [(A, x), (A, y)]
    w[1] += [(B, z)]
    W.append(w)
    W.append(background(350))
    return W, dict(A=A, B=B, x=x, y=y, z=z, window=6)


def reached(world: int, windows, n_items: int, marks=None, item_cut=ITEM_CUT, user_cut=USER_CUT, seed=SEED):
    """Which of the branches (a)-(h) the log reaches, found from SampledModel's run over the serialised windows
    (and nothing else).  Returns (set of letters, the model after the log, its ModelWindow per window)."""
    model = sm.SampledModel(n_items, item_cut, user_cut, seed)
    got = set()
    last_only: Counter = Counter()  # item -> what windows with its records on the last rank only added to its counter
    fb_hi_prev: Counter = Counter()
    mws = []
    for wi, per_rank in enumerate(windows):
        start = dict(model.item_count)
        len_before = {u: len(model.H.get(u, [])) for R in per_rank for u, _ in R}
        H_before = {u: list(model.H.get(u, [])) for R in per_rank for u, _ in R}
        recs = serial(per_rank)
        mw = model.window(recs)
        mws.append(mw)
        h = [Counter(i for _, i in R) for R in per_rank]
        dec, at = [], 0
        for R in per_rank:
            dec.append(mw.decisions[at:at + len(R)])
            at += len(R)
        for r in range(1, world):
            for i, n in h[r].items():
                room = item_cut - start.get(i, 0) - sum(h[q][i] for q in range(r))
                if 0 < room < n:
                    got.add("a")
        fb_hi: Counter = Counter()
        minus_ranks = 0
        for r, R in enumerate(per_rank):
            rho: Counter = Counter()
            minus = False
            for (u, i), d in zip(R, dec[r]):
                alone = start.get(i, 0) + rho[i]
                if r >= 1 and d == "r" and alone < item_cut:
                    got.add("b")
                if r == 0 and d == "r" and last_only[i] > 0 and alone - last_only[i] < item_cut:
                    got.add("c")
                if r == 0 and d != "r" and fb_hi_prev[i] > 0 and alone + fb_hi_prev[i] >= item_cut:
                    got.add("d")
                if r >= 1 and d == "b":
                    fb_hi[i] += 1
                if d.startswith("k") and int(d[1:]) < len_before[u]:
                    minus = True
                rho[i] += 1
            minus_ranks += minus
        if recs and any(not R for R in per_rank):
            got.add("e")
        if recs and set(mw.decisions) <= {"r", "b"}:
            assert not mw.delta
            got.add("f")
        if minus_ranks == 1:
            got.add("g")
        if marks and wi == marks["window"]:
            A, B, x, y = marks["A"], marks["B"], marks["x"], marks["y"]
            da = [d for (u, _), d in zip(per_rank[0], dec[0]) if u == A]
            db = [d for (u, _), d in zip(per_rank[1], dec[1]) if u == B]
            if (A % world == 0 and B % world == 1 and da == ["f", "f"] and db == ["k1"] and H_before[B] == [x, y]
                    and model.H[A] == [x, y] and mw.delta.get((x, y), None) == 0 and mw.delta.get((y, x), None) == 0):
                got.add("h")
        for i in set().union(*[set(c) for c in h]):
            if h[world - 1][i] > 0 and all(h[q][i] == 0 for q in range(world - 1)):
                last_only[i] += min(h[world - 1][i], max(0, item_cut - start.get(i, 0)))
        fb_hi_prev = fb_hi
    return got, model, mws
