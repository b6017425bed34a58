"""cooc_sample_owned without a GPU: the symbol is declared, exported and bound and leaves the ABI version alone; the
numpy double of its exchange (tests/_sample_owned.ExchangeDouble: histogram lists, base and totals by search in the
peers' lists, the feedback lists) equals the contract's data-parallel form (_sampled_comm.RankParallel) and the
serial model (_sampled_model.SampledModel over R_0 || R_1 || ...) on the logs the GPU tests run."""
import numpy as np
import pytest

import _sample_owned as so
import _sampled_comm as sc


def test_symbol_binding_and_abi(pkg):
    from flink_cooccurrence_amd import _lib, sharding

    L = pkg.load_library()
    assert "cooc_sample_owned" in pkg.header_symbols()
    assert L.cooc_sample_owned.argtypes is not None
    assert len(L.cooc_sample_owned.argtypes) == len(L.cooc_sample_device.argtypes) + 1 == 18
    assert L.cooc_sample_owned.argtypes[-1] == L.cooc_sample_device.argtypes[-1]  # the same cooc_sample_info
    assert L.cooc_abi_version() == 7
    assert hasattr(pkg.CooccurrenceCore, "sample_owned") and callable(sharding.sample_owned)
    assert L.cooc_sample_owned(None, 0, None, None, 1, None, 1, None, 5, 2, 0, None, None, 0, None, None, None,
                               None) == _lib.COOC_ERR_ARG  # no context: refused, nothing touched


def _logs(world):
    yield "dictated-300", sc.dictated_log(world, 300)[0], 300, sc.ITEM_CUT, sc.USER_CUT
    yield "dictated-70000", sc.dictated_log(world, 70_000)[0], 70_000, sc.ITEM_CUT, sc.USER_CUT
    yield "wide", so.wide_log(world), so.WIDE_ITEMS, so.WIDE_ITEM_CUT, so.WIDE_USER_CUT


@pytest.mark.parametrize("world", [2, 3])
def test_exchange_double_equals_both_models(world):
    for name, windows, n_items, item_cut, user_cut in _logs(world):
        shards = [so.shard(windows, r) for r in range(world)]
        double = so.ExchangeDouble(world, n_items, item_cut, user_cut, sc.SEED, [s[2] for s in shards])
        par = sc.RankParallel(world, item_cut, user_cut, sc.SEED)
        model, serial_dec = so.model_of(windows, n_items, item_cut, user_cut, sc.SEED)
        for wi, per_rank in enumerate(windows):
            local = [(s[0][s[3][wi]:s[3][wi + 1]], s[1][s[3][wi]:s[3][wi + 1]]) for s in shards]
            got = double.window(local)
            flat = par.window(per_rank)
            assert [d for ds in got for d in ds] == flat, f"{name}: window {wi} against RankParallel"
            assert got == serial_dec[wi], f"{name}: window {wi} against the serial model"
            for r in range(world):  # the replicated counters after every window
                assert {i: int(c) for i, c in enumerate(double.count[r]) if c} == \
                    {i: c for i, c in par.count[r].items() if c}, f"{name}: window {wi}, rank {r}"
        for r, (_, _, keys, _) in enumerate(shards):
            ptr, items, total, count, info = so.expected_rank(model, serial_dec, keys.tolist(), r, n_items)
            assert [i for h in double.H[r] for i in h] == items.tolist(), f"{name}: rank {r}"
            assert [len(h) for h in double.H[r]] == np.diff(ptr).tolist()
            assert double.total[r].tolist() == total.tolist()
            assert np.array_equal(double.count[r].astype(np.int16), count)
            assert {k: double.ctr[r][k] for k in ("rejected", "fills", "replacements", "feedbacks")} == \
                {k: info[k] for k in ("rejected", "fills", "replacements", "feedbacks")}
            assert dict(par.ctr[r]) == {k: v for k, v in double.ctr[r].items() if v}
        if name == "dictated-300":  # the "no list gathered" branch: a window without a feedback on any rank
            assert double.gathers[6][1] == 0 and double.gathers[6][0] > 0
            assert all(144 <= n for _, n in double.gathers[1:4])


@pytest.mark.parametrize("world", [2, 3])
def test_logs_reach_what_the_gpu_tests_rely_on(world):
    """from the models alone: the dictated log walks (a)-(f) in both universes; the wide log has a rank-window above
    one block with more than a wave of feedbacks, replacements, an empty rank-window and the cut inside a higher
    rank's records"""
    for n_items in (300, 70_000):
        windows, marks = sc.dictated_log(world, n_items)
        assert sc.reached(world, windows, n_items, marks)[0] >= set("abcdef")
    windows = so.wide_log(world)
    got, _, _ = sc.reached(world, windows, so.WIDE_ITEMS, None, so.WIDE_ITEM_CUT, so.WIDE_USER_CUT, sc.SEED)
    assert {"a", "b", "d", "e"} <= got
    _, dec = so.model_of(windows, so.WIDE_ITEMS, so.WIDE_ITEM_CUT, so.WIDE_USER_CUT, sc.SEED)
    for by_rank in dec:  # (every non-empty rank-window: 83 to 436 feedbacks, 19 to 203 replacements)
        for ds in by_rank:
            if ds:
                assert sum(d == "b" for d in ds) >= 65 and sum(d[0] == "k" for d in ds) >= 1
    assert any(len(ds) > 256 and sum(d == "b" for d in ds) >= 65 for by_rank in dec for ds in by_rank)
    assert any(not ds for by_rank in dec for ds in by_rank)
