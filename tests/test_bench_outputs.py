"""bench.py --dump-outputs: the helpers that turn a result into the float arrays it writes.  The row sample is a
function of the row lengths alone (fixed ladder + seeded order, within the entry cap); a window's arrays keep the leading
rows and zero the unset heap slots; the files are float32 / float64 within the size limit."""
import numpy as np
import pytest

import bench


def test_sample_rows_fixed_seeded_and_capped():
    rng = np.random.default_rng(5)
    nnz = rng.integers(0, 300, 200_000).astype(np.int32)
    nnz[0], nnz[10] = 150_000, 600_000  # row 10 alone is past the ladder's half of the cap
    cap = 1_000_000
    rows = bench.sample_rows(nnz, cap)
    assert np.array_equal(rows, bench.sample_rows(nnz.copy(), cap))
    assert len(np.unique(rows)) == len(rows) and rows.min() >= 0 and rows.max() < len(nnz)
    assert list(rows[:5]) == [0, 100, 1000, 10_000, 100_000]
    total = int(nnz[rows].sum())
    assert cap - 300 < total <= cap
    # a small result is sampled whole
    small = np.full(97, 40, np.int32)
    assert sorted(bench.sample_rows(small, cap)) == list(range(97))
    assert len(bench.sample_rows(np.zeros(0, np.int32), cap)) == 0


def test_window_arrays_prefix_and_unset_slots():
    class W:
        rows = np.arange(3, dtype=np.int32)
        row_ptr = np.array([0, 2, 5, 9], np.int64)
        cols = np.arange(9, dtype=np.int32)
        exact = np.arange(1, 10, dtype=np.int64)
        rs_items = np.arange(3, dtype=np.int32)
        rs_exact = np.array([3, 12, 30], np.int64)
        observed = 45
        topk_rows = np.arange(3, dtype=np.int32)
        topk_sizes = np.array([1, 2, 0], np.int32)
        topk_values = np.full((3, 2), 7, np.int32)
        topk_scores = np.full((3, 2), np.nan)

    a = bench.window_arrays(W)
    assert np.array_equal(a["row_ptr"], [0, 2, 5, 9]) and np.array_equal(a["cnt"], np.arange(1, 10))
    assert np.array_equal(a["topk_values"], [[7, 0], [7, 7], [0, 0]])
    assert np.isnan(a["topk_scores"][0, 0]) and a["topk_scores"][0, 1] == 0 and not a["topk_scores"][2].any()
    assert np.array_equal(a["totals"], [9, 45])
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())


def test_write_outputs_types_and_limit(tmp_path):
    arrays = {"a": np.arange(5, dtype=np.float64), "b": np.ones((2, 3), np.float32)}
    bench.write_outputs(str(tmp_path / "d"), arrays)
    assert sorted(p.name for p in (tmp_path / "d").iterdir()) == ["a.npy", "b.npy"]
    assert np.array_equal(np.load(tmp_path / "d" / "a.npy"), arrays["a"])
    with pytest.raises(AssertionError):
        bench.write_outputs(str(tmp_path / "e"), {"a": np.arange(5)})  # integers are not written
    with pytest.raises(AssertionError):
        bench.write_outputs(str(tmp_path / "f"), {"a": np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1)})
