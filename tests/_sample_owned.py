"""cooc_sample_owned (include/cooc.h, "device-side sampler across GPUs"), for the tests of it: the wide log, the
ranks' shards of a log as the entry point takes them, the expected outputs of a rank from the pure-Python model, and
a numpy double of the exchange -- every rank's window restated over arrays with the all-gathers as list
concatenations, the way the library runs it (histograms sorted by item, base and totals by binary search, the
feedback lists subtracted by the peers).  No library code."""
from __future__ import annotations

import numpy as np

import _sampled_comm as sc
import _sampled_model as sm

WIDE_ITEMS, WIDE_ITEM_CUT, WIDE_USER_CUT = 24, 300, 4


def wide_log(world: int):
    """4 windows of 700 records per rank (none for the last rank in window 2), 40 users per rank (u mod world),
    Zipf items over 24: block and wave boundaries of the feedback list's append, a rank with no record in a window"""
    rng = np.random.default_rng(7)
    windows = []
    for w in range(4):
        per_rank = []
        for r in range(world):
            n = 0 if (w == 2 and r == world - 1) else 700
            users = rng.integers(0, 40, n) * world + r
            items = np.minimum(rng.zipf(1.2, n) - 1, WIDE_ITEMS - 1)
            per_rank.append([(int(u), int(i)) for u, i in zip(users, items)])
        windows.append(per_rank)
    return windows


def rank_users(windows, rank: int):
    """the sorted job-wide ids of the users with a record on `rank`: the local index is the position"""
    return sorted({u for w in windows for u, _ in w[rank]})


def shard(windows, rank: int):
    """rank's arguments: (local user indices, items, keys, window_ptr) as numpy arrays"""
    keys = rank_users(windows, rank)
    local = {u: j for j, u in enumerate(keys)}
    recs = [rec for w in windows for rec in w[rank]]
    wp = np.concatenate([[0], np.cumsum([len(w[rank]) for w in windows])]).astype(np.int64)
    return (np.array([local[u] for u, _ in recs], np.int32), np.array([i for _, i in recs], np.int32),
            np.array(keys, np.int32), wp)


def serial_log(windows):
    """the job's log: every window R_0 || R_1 || ..., and its window_ptr"""
    flat = [sc.serial(w) for w in windows]
    wp = np.concatenate([[0], np.cumsum([len(w) for w in flat])]).astype(np.int64)
    recs = [rec for w in flat for rec in w]
    return np.array([u for u, _ in recs], np.int32), np.array([i for _, i in recs], np.int32), wp


def model_of(windows, n_items, item_cut, user_cut, seed):
    """SampledModel after the serialised windows, and its decisions per window and rank"""
    model = sm.SampledModel(n_items, item_cut, user_cut, seed)
    decisions = []
    for per_rank in windows:
        mw = model.window(sc.serial(per_rank))
        at, by_rank = 0, []
        for R in per_rank:
            by_rank.append(mw.decisions[at:at + len(R)])
            at += len(R)
        decisions.append(by_rank)
    return model, decisions


def expected_rank(model, decisions, keys, rank: int, n_items: int):
    """what rank's call returns, from the model: (res_ptr, res_items, total, item_count, info)"""
    lens = np.array([len(model.H.get(u, [])) for u in keys], np.int64)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    items = np.array([i for u in keys for i in model.H.get(u, [])], np.int32)
    total = np.array([model.total[u] for u in keys], np.int32)
    count = np.zeros(n_items, np.int16)
    for i, c in model.item_count.items():
        count[i] = c
    mine = [d for by_rank in decisions for d in by_rank[rank]]
    info = {"rejected": sum(d == "r" for d in mine), "fills": sum(d == "f" for d in mine),
            "replacements": sum(d[0] == "k" for d in mine), "feedbacks": sum(d == "b" for d in mine),
            "users": int(np.count_nonzero(lens)), "item_counter_sum": int(sum(model.item_count.values())),
            "reservoir_items": int(ptr[-1])}
    return ptr, items, total, count, info


class ExchangeDouble:
    """numpy double of cooc_sample_owned's windows: rank r holds count_r[n_items] (a replica), and by local user
    index its reservoirs and totals; a window is, per rank, the sort by item into a histogram list, the gather of
    the lists, base and the job's totals by binary search in the peers' lists, the cut at rho + base, the commit by
    each item's lowest listing rank, the local user stage with the draw keyed by keys_r[j], and the gathered
    feedback lists subtracted by the peers."""

    def __init__(self, world, n_items, item_cut, user_cut, seed, keys):
        self.world, self.n_items, self.item_cut, self.user_cut, self.seed = world, n_items, item_cut, user_cut, seed
        self.keys = [np.asarray(k, np.int64) for k in keys]
        self.count = [np.zeros(n_items, np.int32) for _ in range(world)]
        self.H = [[[] for _ in k] for k in keys]
        self.total = [np.zeros(len(k), np.int32) for k in keys]
        self.ctr = [dict(rejected=0, fills=0, replacements=0, feedbacks=0) for _ in range(world)]
        self.gathers = []  # per window: (histogram words gathered, feedback words gathered)

    @staticmethod
    def _find(lst, item):
        """the records of `item` in a histogram list of (item << 32 | records) words sorted by item"""
        at = int(np.searchsorted(lst >> np.uint64(32), np.uint64(item)))
        return int(lst[at] & np.uint64(0xFFFFFFFF)) if at < len(lst) and int(lst[at] >> np.uint64(32)) == item else 0

    def window(self, per_rank_local):
        """per_rank_local[r] = (local user indices, items) of rank r's records; returns the decisions per rank"""
        W = self.world
        hist = []
        for users, items in per_rank_local:  # k_icx_pack: the runs of the by-item order
            ids, n = np.unique(np.asarray(items, np.int64), return_counts=True)
            hist.append((ids.astype(np.uint64) << np.uint64(32)) | n.astype(np.uint64))
        decisions, fb = [], []
        for r, (users, items) in enumerate(per_rank_local):
            users, items = np.asarray(users, np.int64), np.asarray(items, np.int64)
            order = np.argsort(items, kind="stable")
            rho = np.empty(len(items), np.int64)
            if len(items):
                sorted_items = items[order]
                head = np.flatnonzero(np.concatenate([[True], sorted_items[1:] != sorted_items[:-1]]))
                run = np.cumsum(np.concatenate([[True], sorted_items[1:] != sorted_items[:-1]])) - 1
                rho[order] = np.arange(len(items)) - head[run]
            base = {int(w >> np.uint64(32)): sum(self._find(hist[q], int(w >> np.uint64(32))) for q in range(r))
                    for w in hist[r]}
            samp = np.array([rho[p] + base[int(items[p])] < self.item_cut - self.count[r][items[p]]
                             for p in range(len(items))], bool)
            dec, mine = [], []
            seen: dict = {}
            for p in range(len(items)):  # the user stage, local
                u, i = int(users[p]), int(items[p])
                j = seen.get(u, 0)
                seen[u] = j + 1
                t = int(self.total[r][u]) + j + 1
                if not samp[p]:
                    self.ctr[r]["rejected"] += 1
                    dec.append("r")
                    continue
                H = self.H[r][u]
                if len(H) < self.user_cut:
                    H.append(i)
                    self.ctr[r]["fills"] += 1
                    dec.append("f")
                    continue
                k = sm.draw(self.seed, int(self.keys[r][u]), t)
                if k < self.user_cut:
                    H[k] = i
                    self.ctr[r]["replacements"] += 1
                    dec.append(f"k{k}")
                else:
                    mine.append(i)
                    self.ctr[r]["feedbacks"] += 1
                    dec.append("b")
            for u, n in seen.items():
                self.total[r][u] += n
            decisions.append(dec)
            fb.append(mine)
        for r in range(W):  # the commit over the gathered union (each item by its lowest listing rank), the feedback
            for q in range(W):
                for w in hist[q]:
                    item = int(w >> np.uint64(32))
                    if any(self._find(hist[o], item) for o in range(q)):
                        continue
                    tot = sum(self._find(hist[o], item) for o in range(W))
                    self.count[r][item] += min(tot, max(0, self.item_cut - int(self.count[r][item])))
            for q in range(W):
                for i in fb[q]:
                    self.count[r][i] -= 1
            assert int(self.count[r].min(initial=0)) >= 0
        self.gathers.append((sum(len(h) for h in hist), sum(len(f) for f in fb)))
        return decisions
