"""Rescoring with topk > 1024 (flink-cooccurrence_amd/csrc/cooc_rescore.hip, k_rescore: one wave per workgroup,
its heap too large for the four-wave kernels): a universe of 1,300 items whose longest rows hold more than 1,025
entries, so that a full heap of 1,025 takes replacements (score > least) and is not only filled.  Batch results in
both layouts (k_rescore<DenseRows> and k_rescore<CsrRows>, every item a row) and two streaming windows over dense
global rows (k_rescore<DenseRows> over the touched-rows list), every heap against the oracle's rescorer
(ItemRowRescorer...java:195-241, via OracleStream) as in test_batch_topk_vs_rescorer; and the largest topK the
configuration accepts (32,767, a Java short), which no LDS heap holds: the call fails and the context stays usable.
Needs an MI355X."""
import numpy as np
import pytest

from tests._helpers import assert_topk_equal, assert_windows_equal

pytestmark = pytest.mark.gpu

INT64_MAX = np.iinfo(np.int64).max
M, K = 1300, 1025


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def wide_log():
    """250 users of about 100 distinct items each: the head items' rows reach nearly every column, and no count
    leaves the int16 range (the heaps are numeric)."""
    from flink_cooccurrence_amd import datagen

    return datagen.small_log(41, 250, M, 100.0, replacement=False)


def _one_window(oracle, up, it, k):
    lens = np.diff(up)
    ref = oracle.OracleStream(1000, topk=k)
    ref.process_elements(np.repeat(np.arange(len(lens), dtype=np.int32), lens), it, np.zeros(len(it), np.int64))
    (w,) = ref.process_watermark(INT64_MAX)
    return w


@pytest.fixture(scope="module")
def wide_ref(oracle, wide_log):
    return _one_window(oracle, *wide_log, K)


def _assert_batch_equals(sizes, vals, scores, w, n_items):
    rows = w.topk_rows
    assert np.all(sizes[np.setdiff1d(np.arange(n_items), rows)] == 0)

    class G:
        pass

    g = G()
    g.topk_rows, g.topk_sizes, g.topk_values, g.topk_scores = rows, sizes[rows], vals[rows], scores[rows]
    assert_topk_equal(g, w)


@pytest.mark.parametrize("output", ["dense", "csr"])
def test_batch_topk_1025_vs_rescorer(pkg, wide_log, wide_ref, torch_cuda, output):
    up, it = wide_log
    with pkg.CooccurrenceCore(n_items=M, output=output) as core:
        got = core.count(up, it)
        sizes, vals, scores = core.topk_batch(K)
    assert np.diff(got.row_ptr).max() > K  # a row longer than the heap: replacements, not only the fill
    assert sizes.max() == K
    _assert_batch_equals(sizes, vals, scores, wide_ref, M)


def test_streaming_topk_1025_vs_oracle(pkg, oracle, wide_log, torch_cuda):
    """Two windows (each user's items halved between them) over dense global rows."""
    from flink_cooccurrence_amd import datagen

    up, it = wide_log
    lens = np.diff(up)
    pos = np.arange(len(it)) - np.repeat(up[:-1], lens)
    ts = np.where(pos < np.repeat(lens // 2, lens), 500, 1500).astype(np.int64)
    users, items, ts = datagen.to_records(up, it, ts)
    op = pkg.NonSampledUserInteractionCounterOneInputStreamOperator(1, "SECONDS", n_items=M, top_k=K)
    ref = oracle.OracleStream(1000, topk=K)
    op.process_elements(users, items, ts)
    ref.process_elements(users, items, ts)
    got = op.process_watermark(INT64_MAX)
    want = ref.process_watermark(INT64_MAX)
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert_windows_equal(g, w)
    rows, rp, _, _, _ = ref.global_rows()
    longest = int(rows[np.argmax(np.diff(rp))])
    assert np.diff(rp).max() > K and longest in want[-1].topk_rows.tolist()
    assert want[-1].topk_sizes.max() == K
    op.close()


def test_batch_topk_32767_fails_and_context_survives(pkg, oracle, torch_cuda):
    from flink_cooccurrence_amd import datagen

    up, it = datagen.small_log(13, 800, 150, 18.0)
    with pkg.CooccurrenceCore(n_items=150) as core:
        core.count(up, it)
        with pytest.raises(pkg.IllegalArgumentException, match="topk too large for the LDS heaps"):
            core.topk_batch(32767)
        sizes, vals, scores = core.topk_batch(7)
    _assert_batch_equals(sizes, vals, scores, _one_window(oracle, up, it, 7), 150)
