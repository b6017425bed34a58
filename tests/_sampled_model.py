"""Pure-Python model of the sampled streaming mode (include/cooc.h, "sampled mode"): the item cut, the per-user
reservoir with its counter-based draw and the end-of-window feedback, record by record, with the per-event +-1
records as the reference writes them (UserInteractionCounterOneInputStreamOperator.java:167-250) and the window
outputs by the header's rule.  No library code: the tests compare the library against this restatement."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

MASK = (1 << 64) - 1


def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def draw(seed: int, user: int, total: int) -> int:
    key = ((user & 0xFFFFFFFF) << 32) | (total & 0xFFFFFFFF)
    return ((splitmix64((seed & MASK) ^ key) >> 32) * total) >> 32


def i16(x: int) -> int:
    x &= 0xFFFF
    return x - 0x10000 if x & 0x8000 else x


def i32(x: int) -> int:
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x & 0x80000000 else x


@dataclass
class ModelWindow:
    delta: dict            # {(a, b): signed net}, zero nets kept
    rowsum: dict           # {a: signed row sum of the nets}, one per delta row
    observed: int          # fills only: sum |H'|(|H'|-1) - |H|(|H|-1)
    decisions: list        # per record: "r" rejected, "f" fill, "k<slot>" replacement, "b" feedback
    events: dict = field(default_factory=dict)  # {(a, b): sum of the reference's emitted +-1 records}
    twice: int = 0         # slots changed more than once within the window
    zero_nets: int = 0

    def rows(self) -> dict:
        out: dict = {}
        for (a, b), v in self.delta.items():
            out.setdefault(a, {})[b] = v
        return {a: dict(sorted(r.items())) for a, r in sorted(out.items())}


class SampledModel:
    def __init__(self, n_items: int, item_cut: int, user_cut: int, seed: int):
        self.n_items, self.item_cut, self.user_cut, self.seed = n_items, item_cut, user_cut, seed
        self.item_count: dict = {}
        self.H: dict = {}       # user -> reservoir (slot order)
        self.total: dict = {}   # user -> userInteractionsTotal
        self.G: dict = {}       # (a, b) -> exact global count (zero counts removed)
        self.rs: dict = {}      # a -> exact global row sum
        self.rejected = self.fills = self.replacements = self.feedbacks = 0
        self.observed_exact = 0      # ObservedCooccurrences accumulator (fills)
        self.observed_rescorer = 0   # the rescorer's long: += the int view of every row-sum delta
        self.rowsum_acc = 0
        self.rescored = 0

    def window(self, records) -> ModelWindow:
        before: dict = {}
        changed: dict = {}
        events: dict = {}
        feedback = []
        decisions = []
        twice = 0

        def emit(a, b, v):
            events[(a, b)] = events.get((a, b), 0) + v

        for u, i in records:
            sample = self.item_count.get(i, 0) < self.item_cut
            if sample:
                self.item_count[i] = self.item_count.get(i, 0) + 1
            else:
                self.rejected += 1
            self.total[u] = self.total.get(u, 0) + 1
            if not sample:
                decisions.append("r")
                continue
            H = self.H.setdefault(u, [])
            if u not in before:
                before[u] = list(H)
                changed[u] = set()
            if len(H) < self.user_cut:
                for h in H:
                    emit(i, h, 1)
                    emit(h, i, 1)
                changed[u].add(len(H))
                H.append(i)
                self.fills += 1
                decisions.append("f")
                continue
            k = draw(self.seed, u, self.total[u])
            assert 0 <= k < self.total[u]
            if k < self.user_cut:
                prev = H[k]
                for s, h in enumerate(H):
                    if s != k:
                        emit(i, h, 1)
                        emit(prev, h, -1)
                        emit(h, i, 1)
                        emit(h, prev, -1)
                if k in changed[u]:
                    twice += 1
                changed[u].add(k)
                H[k] = i
                self.replacements += 1
                decisions.append(f"k{k}")
            else:
                feedback.append(i)
                decisions.append("b")
        for i in feedback:
            self.item_count[i] -= 1
            assert self.item_count[i] >= 0
        self.feedbacks += len(feedback)

        delta: dict = {}
        observed = 0
        for u, ch in changed.items():
            if not ch:
                continue
            Hb, Ha = before[u], self.H[u]
            observed += len(Ha) * (len(Ha) - 1) - len(Hb) * (len(Hb) - 1)
            for H_, sign in ((Ha, 1), (Hb, -1)):
                n = len(H_)
                for p in ch:  # every ordered pair of two distinct slots with at least one of them changed
                    if p >= n:
                        continue
                    a = H_[p]
                    for q in range(n):
                        if q == p:
                            continue
                        delta[(a, H_[q])] = delta.get((a, H_[q]), 0) + sign
                        if q not in ch:
                            delta[(H_[q], a)] = delta.get((H_[q], a), 0) + sign
        # the reference's records telescope to the same nets; its key set may be larger
        for key, v in events.items():
            assert delta.get(key, 0) == v, (key, v, delta.get(key))
        assert set(delta) <= set(events)
        rowsum: dict = {}
        for (a, b), v in delta.items():
            rowsum[a] = rowsum.get(a, 0) + v
            g = self.G.get((a, b), 0) + v
            assert g >= 0
            if g:
                self.G[(a, b)] = g
            else:
                self.G.pop((a, b), None)
        for a, v in rowsum.items():
            self.rs[a] = self.rs.get(a, 0) + v
            self.observed_rescorer += i32(v)
            self.rowsum_acc += i32(v)
        self.observed_exact += observed
        self.rescored += len(rowsum)
        return ModelWindow(delta, rowsum, observed, decisions, events, twice,
                           sum(1 for v in delta.values() if v == 0))

    def counters(self) -> dict:
        return {"item_cut_rejections": self.rejected, "fills": self.fills, "replacements": self.replacements,
                "feedbacks": self.feedbacks, "users": sum(1 for h in self.H.values() if h),
                "item_counter_sum": sum(self.item_count.values())}

    def global_rows(self) -> dict:
        out: dict = {}
        for (a, b), v in self.G.items():
            out.setdefault(a, {})[b] = v
        return {a: dict(sorted(r.items())) for a, r in sorted(out.items())}

    def rs32(self) -> np.ndarray:
        out = np.zeros(self.n_items, np.int32)
        for a, v in self.rs.items():
            out[a] = i32(v)
        return out


def reference_log(n_items: int = 24, spread: int = 1):
    """The reference log of the sampled mode's tests: 8 windows of 60 records, users integers(0, 12), items min(zipf(1.3) - 1, 23)
    (times `spread`, to reach a large universe), numpy.random.default_rng(7)."""
    rng = np.random.default_rng(7)
    windows = []
    for _ in range(8):
        users = rng.integers(0, 12, 60)
        items = np.minimum(rng.zipf(1.3, 60) - 1, 23)
        windows.append([(int(u), int(i) * spread) for u, i in zip(users, items)])
    return windows


def find_user_total(seed: int, total: int, want, user_lo: int = 0, user_hi: int = 1 << 20) -> int:
    """The first user id in [user_lo, user_hi) whose draw at `total` satisfies want(k)."""
    for u in range(user_lo, user_hi):
        if want(draw(seed, u, total)):
            return u
    raise LookupError("no user id gives the wanted draw")
