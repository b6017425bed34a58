"""The contract of the sampled mode across ranks (include/cooc.h, "sampled mode at world > 1"), pinned on the CPU: the
data-parallel form it gives -- per-rank histograms h_q, base_r = sum over lower ranks, the cut at count + base +
rho, the commit count += min(sum h, max(0, item_cut - count)) - sum f on every rank -- equals SampledModel fed
every window in the serialised order R_0 || R_1 || ... || R_{W-1}, on random 3-rank logs; and the dictated log of
the multi-process GPU test reaches each branch it is written for.  No library code runs here."""
import numpy as np
import pytest

import _sampled_comm as sc
import _sampled_model as sm


def _random_log(seed, world=3, n_windows=6, n=150, n_users=60, n_items=30):
    rng = np.random.default_rng(seed)
    out = []
    for wi in range(n_windows):
        users = rng.integers(0, n_users, n)
        items = np.minimum(rng.zipf(1.3, n) - 1, n_items - 1)
        quiet = int(rng.integers(0, world)) if wi % 2 else -1  # every other window one rank has no record
        per_rank = [[] for _ in range(world)]
        for u, i in zip(users.tolist(), items.tolist()):
            if u % world != quiet:
                per_rank[u % world].append((u, i))
        out.append(per_rank)
    return out


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("cuts", [(8, 3), (3, 1), (40, 2)])
def test_data_parallel_form_equals_the_serialised_model(seed, cuts):
    item_cut, user_cut = cuts
    world, M = 3, 30
    model = sm.SampledModel(M, item_cut, user_cut, sc.SEED)
    par = sc.RankParallel(world, item_cut, user_cut, sc.SEED)
    seen = set()
    for per_rank in _random_log(seed):
        mw = model.window(sc.serial(per_rank))
        assert par.window(per_rank) == mw.decisions
        seen |= {d[0] for d in mw.decisions}
        want = {i: c for i, c in model.item_count.items() if c}
        for r in range(world):  # replicated: identical on every rank, also for items the rank saw no record of
            assert {i: c for i, c in par.count[r].items() if c} == want, f"rank {r}"
        assert par.H == model.H and par.total == model.total
    ctr = sum(par.ctr, start=type(par.ctr[0])())
    assert (ctr["rejected"], ctr["fills"], ctr["replacements"], ctr["feedbacks"]) == (
        model.rejected, model.fills, model.replacements, model.feedbacks)
    assert seen >= ({"r", "f", "k"} if user_cut * 30 >= 60 else {"r", "f"})


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("n_items", [300, 40_500, 1_000_000])
def test_dictated_log_reaches_every_branch(world, n_items):
    windows, marks = sc.dictated_log(world, n_items)
    got, model, mws = sc.reached(world, windows, n_items, marks)
    assert got == set(sc.BRANCHES), f"not reached: {sorted(set(sc.BRANCHES) - got)}"
    users = {u for w in windows for R in w for u, _ in R}
    assert len(windows) <= 8 and len(users) <= 300 and sum(len(R) for w in windows for R in w) <= 4000
    assert all(u % world == r for w in windows for r, R in enumerate(w) for u, _ in R)
    assert max(i for w in windows for R in w for _, i in R) == n_items - 1
    # the log is more than its dictated records: replacements and feedbacks on every rank, zero nets, a window
    # whose minus runs are on more than one rank
    par = sc.RankParallel(world, sc.ITEM_CUT, sc.USER_CUT, sc.SEED)
    for w in windows:
        par.window(w)
    assert all(min(c["rejected"], c["fills"], c["replacements"], c["feedbacks"]) >= 10 for c in par.ctr)
    assert sum(mw.zero_nets for mw in mws) >= 2
