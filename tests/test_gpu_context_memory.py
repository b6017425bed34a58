"""A context gives back the device memory it took: cycles of open / a few windows / close, free device memory
(torch.cuda.mem_get_info) after cycle 2 against after cycle 6 (the first cycles absorb code-object loading).

Three kinds of cycle, each with topk > 0: a dense sampled context with a window of two counting runs (host and
device sampler), a large-universe context whose row slabs compact (the windows of
test_gpu_global_slabs.py::test_repeated_compaction at n_items = 40,500), and a restore refused for a corrupted
checksum byte (Snapshotter::wipe).

BOUND (bytes of free memory lost between cycle 2 and cycle 6) was measured against the commit before DevBuf owned
its memory, not against the code under test.  This file run three times there gave 0 / 0 / 0 bytes lost for the
dense sampled cycles (both samplers) and for the refused restore, and 2,097,152 / 2,097,152 / 2,097,152 for the
large universe: free memory dropped once, after cycle 3, and stayed there through cycle 6.  (That commit's
Counter::release did not name sp_rank_, sp_rkeys_ and sp_bits_; sp_bits_, about 10 KB, is reserved by every
large-universe run, so each cycle lost less than a step and a new block was taken now and then.  With DevBuf
owning its memory all four kinds read 0.)  The allocator's step (the smallest non-zero difference mem_get_info
showed on that MI355X, under 1-byte hipMallocs) was 2 MiB.
BOUND = the largest reading + one step = 4 MiB.  Since the largest reading is that commit's own leak, the
large-universe case passes there too: a return of exactly that leak (a few KB per context) is below what this
test can see; only a loss of more than 4 MiB over four cycles fails it.

The test only catches gross leaks (a buffer of at least a step lost per cycle); that no buffer can be dropped
without being freed is DevBuf's deleted copy constructor.
"""
import struct

import numpy as np
import pytest

from tests.test_gpu_global_slabs import _log_f, _records

pytestmark = pytest.mark.gpu

BOUND = 4 << 20
CYCLES = 6
SEED = 0xC0FFEE


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _lost(torch_cuda, cycle, kind):
    """free memory after cycle 2 - free memory after cycle 6 of `cycle`"""
    free = []
    for _ in range(CYCLES):
        cycle()
        torch_cuda.cuda.synchronize()
        free.append(torch_cuda.cuda.mem_get_info()[0])
    lost = free[1] - free[-1]
    print(f"{kind}: free after each cycle {free}, lost between cycle 2 and cycle {CYCLES}: {lost} B")
    return lost


def _sampled_windows():
    """5 windows of 200 records: 40 users over 300 items, so every user passes user_cut = 4 in the first window
    and later records replace slots that existed before their window (the minus run)"""
    rng = np.random.default_rng(11)
    return [(rng.integers(0, 40, 200).astype(np.int32), rng.integers(0, 300, 200).astype(np.int32))
            for _ in range(5)]


@pytest.mark.parametrize("sample_on", ["host", "device"])
def test_dense_sampled_context_returns_its_memory(pkg, torch_cuda, sample_on):
    windows = _sampled_windows()
    runs = set()

    def cycle():
        with pkg.CooccurrenceCore(n_items=300, topk=5, user_cut=4, item_cut=20, sample_seed=SEED,
                                  sample_on=sample_on) as core:
            for w, (users, items) in enumerate(windows):
                assert core.op_process_elements(users, items, np.full(len(users), 1000 * w + 1, np.int64)) == 0
                out = core.op_process_watermark(1000 * w + 999)
                assert len(out) == 1
                runs.add(core.last_window_runs())

    lost = _lost(torch_cuda, cycle, f"dense sampled ({sample_on})")
    assert 2 in runs
    assert lost <= BOUND


def test_large_universe_context_returns_its_memory(pkg, torch_cuda):
    M = 40_500
    log = [_records(w, users) for w, users in enumerate(_log_f(M)[:8])]
    seen = []

    def cycle():
        op = pkg.NonSampledUserInteractionCounterOneInputStreamOperator(1, "SECONDS", n_items=M, top_k=10)
        for w, rec in enumerate(log):
            assert op.process_elements(*rec) == 0
            assert len(op.process_watermark(1000 * w + 999)) == 1
        seen.append(op.core.global_slab_stats()[3])
        op.close()

    lost = _lost(torch_cuda, cycle, "large universe")
    print(f"compactions per cycle: {seen}")
    assert min(seen) > 0  # compact_global ran
    assert lost <= BOUND


def test_refused_restore_returns_its_memory(pkg, torch_cuda):
    rng = np.random.default_rng(5)
    with pkg.CooccurrenceCore(n_items=300, topk=5) as core:
        for w in range(3):
            users, items = rng.integers(0, 40, 200).astype(np.int32), rng.integers(0, 300, 200).astype(np.int32)
            core.op_process_elements(users, items, np.full(200, 1000 * w + 1, np.int64))
            assert len(core.op_process_watermark(1000 * w + 999)) == 1
        good = core.snapshot()
    bad = bytearray(good)
    at = 64 + 40 * 6 + 32  # the checksum of the 7th section (the rows' columns) in the directory
    assert struct.unpack_from("<q", good, at - 16)[0] > 0  # (the section has bytes)
    bad[at] ^= 0x01
    bad = bytes(bad)

    def cycle():
        with pkg.CooccurrenceCore(n_items=300, topk=5) as core:
            with pytest.raises(pkg.IllegalArgumentException) as e:
                core.restore(bad)
            assert e.value.status == 1

    lost = _lost(torch_cuda, cycle, "refused restore")
    assert lost <= BOUND
