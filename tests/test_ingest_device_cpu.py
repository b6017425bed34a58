"""Device ingest without a GPU: the symbol contract of cooc_parse_interactions_device / cooc_log_prepare_device, the
numpy model of the log preparation (tests/_log_model.py) pinned by hand and against the oracle, and the text
fixtures of the GPU tests checked for what they claim to hold."""
import ctypes

import numpy as np
import pytest

import _log_model as lm
import _sampled_model as sm

INT64_MAX = 2**63 - 1


def test_symbols_bound_and_abi(pkg):
    from flink_cooccurrence_amd import _lib

    L = _lib.load()
    for name in ("cooc_parse_interactions_device", "cooc_log_prepare_device"):
        assert name in _lib.header_symbols()
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == len(_lib._SIGS[name][1])
    assert L.cooc_abi_version() == 7
    assert ctypes.sizeof(_lib.CoocLogInfo) == 64
    assert callable(pkg.CooccurrenceCore.parse_interactions_device) and callable(pkg.CooccurrenceCore.prepare_log)


def test_model_on_the_hand_written_log():
    u, i, t = (np.array(c) for c in zip(*lm.HAND_LOG))
    got = lm.prepare(u, i, t, lm.HAND_W, lm.HAND_SIZE, lm.HAND_ITEMS)
    assert np.flatnonzero(got["late"]).tolist() == [5, 8]
    for key, want in lm.HAND_WANT.items():
        g = got[key]
        assert (g.tolist() if isinstance(g, np.ndarray) else g) == want, key
    # the log has what the issue asks of it
    assert got["n_late"] == 2 and t[4] == t[:4].max() and not got["late"][4]
    assert np.diff(got["window_ts"]).tolist() == [1000, 2000] and got["user_ids"][0] < 0
    assert len({int(w) for w, r in zip(np.repeat(np.arange(3), np.diff(got["window_ptr"])), got["rec_user"]) if r == 2}) > 1


def _feed_oracle(oracle, users, items, ts, W, size, user_cut=0):
    s = oracle.OracleStream(size, user_cut=user_cut)
    late, fired, hi = 0, [], None
    for lo in range(0, len(users), W):
        sl = slice(lo, lo + W)
        late += s.process_elements(users[sl], items[sl], ts[sl])
        hi = int(ts[sl].max()) if hi is None else max(hi, int(ts[sl].max()))
        fired += s.process_watermark(hi - 1)
    fired += s.process_watermark(INT64_MAX)
    return s, late, fired


def _oracle_rows(s):
    rows, row_ptr, cols, exact, _ = s.global_rows()
    return {(int(a), int(cols[e])): int(exact[e]) for r, a in enumerate(rows) for e in range(row_ptr[r], row_ptr[r + 1])
            if exact[e]}


@pytest.mark.parametrize("cut", [0, 2])
def test_model_vs_oracle_hand_log(oracle, cut):
    u, i, t = (np.array(c) for c in zip(*lm.HAND_LOG))
    m = lm.prepare(u, i, t, lm.HAND_W, lm.HAND_SIZE, lm.HAND_ITEMS)
    s, late, fired = _feed_oracle(oracle, u.astype(np.int32), i.astype(np.int32), t.astype(np.int64), lm.HAND_W,
                                  lm.HAND_SIZE, cut)
    assert late == m["n_late"] == s.counters()["UserInteractionCounterLateElements"]
    assert [w.ts for w in fired] == m["window_ts"].tolist()
    # the user histories after the whole log: the oracle's global rows are the pair counts over the model's CSR
    assert _oracle_rows(s) == lm.pair_counts(m["user_ptr"], m["user_items"], cut)


E2E = dict(seed=11, n=6000, n_users=400, n_items=300, W=500, size=1000)
SAMPLED = dict(seed=12, n=2000, n_users=30, n_items=40, W=250, size=1000, item_cut=5, user_cut=4, draw_seed=0x5EED)


def _conditions(m, n):
    assert m["n_windows"] >= 3
    assert 0.05 * n <= m["n_late"] <= 0.5 * n
    win_of = np.repeat(np.arange(m["n_windows"]), np.diff(m["window_ptr"]))
    first = {}
    assert any(first.setdefault(int(u), int(w)) != int(w) for u, w in zip(m["rec_user"], win_of))


def test_end_to_end_log_is_not_vacuous(oracle):
    c = E2E
    u, i, t = lm.jitter_log(c["seed"], c["n"], c["n_users"], c["n_items"])
    m = lm.prepare(u, i, t, c["W"], c["size"], c["n_items"])
    _conditions(m, c["n"])
    assert m["user_ids"][0] < 0 < m["user_ids"][-1]
    s, late, fired = _feed_oracle(oracle, u, i, t, c["W"], c["size"])
    assert late == m["n_late"] and [w.ts for w in fired] == m["window_ts"].tolist()
    assert _oracle_rows(s) == lm.pair_counts(m["user_ptr"], m["user_items"])
    # the text round trip the GPU test starts from
    assert lm.to_text(u, i, t).count(b"\n") == c["n"] and len(lm.to_text(u, i, t)) <= 120_000


def test_sampled_log_is_not_vacuous():
    c = SAMPLED
    u, i, t = lm.jitter_log(c["seed"], c["n"], c["n_users"], c["n_items"], negative_users=False)
    m = lm.prepare(u, i, t, c["W"], c["size"], c["n_items"])
    _conditions(m, c["n"])
    assert m["user_ids"][0] >= 0  # the ids serve as the draw keys
    model = sm.SampledModel(c["n_items"], c["item_cut"], c["user_cut"], c["draw_seed"])
    ids = m["user_ids"][m["rec_user"]]
    for w in range(m["n_windows"]):
        a, b = m["window_ptr"][w], m["window_ptr"][w + 1]
        model.window([(int(x), int(y)) for x, y in zip(ids[a:b], m["rec_item"][a:b])])
    assert model.replacements >= 1 and model.feedbacks >= 1


def test_model_rejects_and_ignores():
    u = np.zeros(6, np.int32)
    t = np.array([100, 200, 150, 50, 300, 400], np.int64)  # W = 3: record 3 (50 < 200) is late
    i = np.array([1, 2, 3, 99, 4, 5], np.int32)
    assert lm.prepare(u, i, t, 3, 1000, 10)["n_late"] == 1  # the out-of-range item of a late record is ignored
    i[4] = i[5] = 99
    with pytest.raises(lm.BadRecord) as e:
        lm.prepare(u, i, t, 3, 1000, 10)
    assert e.value.index == 4
    t2 = t.copy()
    t2[5] = INT64_MAX - 1999
    with pytest.raises(lm.BadRecord) as e:
        lm.prepare(u, np.ones(6, np.int32), t2, 3, 1000, 10)
    assert e.value.index == 5
    t2[5] = INT64_MAX - 2000  # the last timestamp the operator's expression takes
    assert lm.prepare(u, np.ones(6, np.int32), t2, 3, 1000, 10)["window_ts"][-1] == lm.window_end(t2[5:], 1000)[0]
    # W = 0: no watermark before the end; only Long.MIN_VALUE is late
    t3 = np.array([5, 4, -2**63, 3], np.int64)
    assert lm.late_flags(t3, 0).tolist() == [False, False, True, False]
    assert lm.late_flags(t3, 1).tolist() == [False, True, True, True]


def test_window_end_is_the_operators(oracle):
    for t in (0, 999, 1000, -1, -1000, -1001, 123456789, -987654321):
        assert int(lm.window_end(np.array([t]), 1000)[0]) == oracle.window_max_ts(t, 1000)


# ---- the text fixtures ------------------------------------------------------------------------------------------
def test_cycling_text_holds_its_breaks(pkg):
    text = lm.cycling_text()
    assert 69_000 <= len(text) <= 71_000
    nl = np.flatnonzero(np.frombuffer(text, np.uint8) == 10)
    assert set((nl % 64).tolist()) == set(range(64))
    at = set(nl.tolist())
    for K in lm.BOUNDARIES:
        sides = set()
        for m in range(K, len(text) - 64, K):
            assert (m - 1 in at) != (m in at), (K, m)  # a break right before or right after every multiple
            sides.add(m in at)
        assert sides == {True, False}, K  # and both sides occur
    users, items, ts = pkg.parse_interactions(text)
    assert len(users) == len(nl) and users.min() < 0 < users.max()


def test_special_and_long_line_texts(pkg):
    for text, want in ((lm.SPECIAL_TEXT, lm.SPECIAL_WANT), (lm.LONG_LINE_TEXT, lm.LONG_LINE_WANT)):
        got = pkg.parse_interactions(text)
        for g, w in zip(got, want):
            assert g.tolist() == w
    assert not lm.SPECIAL_TEXT.endswith(b"\n") and lm.SPECIAL_TEXT.count(b"\r\n") == 6
    assert max(len(x) for x in lm.LONG_LINE_TEXT.split(b"\n")) == 20_000


@pytest.mark.parametrize("name", sorted(lm.REJECTS))
def test_host_verdict_on_every_reject(pkg, name):
    from flink_cooccurrence_amd import _lib

    for at in (0, lm.N_VALID // 2, lm.N_VALID - 1):
        with pytest.raises(_lib.IllegalArgumentException, match=f"line {at} "):
            pkg.parse_interactions(lm.reject_text(lm.REJECTS[name], at))
    # alone, every dictated line is refused, and the valid lines around it are not
    assert len(pkg.parse_interactions(lm.reject_text(b"1,2,3", 0))[0]) == lm.N_VALID
