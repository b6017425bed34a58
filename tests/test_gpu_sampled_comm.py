"""The sampled mode on a context that has a communicator (single process): the call order -- join, then
sampling_enable -- on a world-1 communicator runs the reference log exactly as a context without one, in both
decision modes; after a world > 1 join the checkpoints of a sampled context are refused, with a message that says
so.  The multi-rank windows themselves are in tests/test_sampled_multiproc.py."""
import numpy as np
import pytest

import _sampled_model as sm
from test_gpu_sampled import _check_window, _fire
from test_gpu_sampled_device_mode import _same_state, _same_window

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE


def _never_called_ops(pkg):
    """cooc_comm_ops whose collectives fail: nothing on these tests' paths may reach a collective"""
    from flink_cooccurrence_amd import _lib

    return _lib.CoocCommOps(_lib.ALLREDUCE_FN(lambda *a: 1), _lib.ALLGATHER_FN(lambda *a: 1),
                            _lib.ALLTOALLV_FN(lambda *a: 1))


@pytest.mark.parametrize("on", ["host", "device"])
def test_world_one_communicator_then_sampling(pkg, oracle, on):
    M = 24
    model = sm.SampledModel(M, 20, 4, SEED)
    kw = dict(n_items=M, topk=5, user_cut=4)
    with pkg.CooccurrenceCore(**kw) as joined, \
            pkg.CooccurrenceCore(item_cut=20, sample_seed=SEED, sample_on=on, **kw) as plain:
        joined.comm_init_ops(0, 1, _never_called_ops(pkg))
        assert not joined.sampled
        joined.sampling_enable(20, SEED, on=on)
        assert joined.sampled
        for wi, recs in enumerate(sm.reference_log()):
            w = _fire(joined, wi, recs)
            _same_window(w, _fire(plain, wi, recs))
            _same_state(joined, plain, range(12))
            _check_window(joined, model, w, model.window(recs), oracle, 5)
        c = joined.sampling_counters()
        assert (c["fills"], c["replacements"], c["feedbacks"], c["item_cut_rejections"]) == (48, 55, 137, 240)
        # a world-1 job keeps its checkpoints
        assert joined.snapshot_sampled() == plain.snapshot_sampled()


def test_sampling_enable_arguments_and_order(pkg):
    from flink_cooccurrence_amd import _lib

    with pkg.CooccurrenceCore(n_items=24, topk=3, user_cut=4) as core:
        with pytest.raises(_lib.IllegalArgumentException):
            core.sampling_enable(20, SEED, on="gpu")
        with pytest.raises(_lib.IllegalArgumentException):
            core.sampling_enable(0, SEED)
        assert not core.sampled
        core.sampling_enable(20, SEED)
        with pytest.raises(_lib.IllegalStateException):
            core.sampling_enable(20, SEED)  # already enabled
        with pytest.raises(_lib.IllegalStateException, match="sampled context"):
            core.comm_init_ops(0, 2, _never_called_ops(pkg))  # the order is: join, then enable
    with pkg.CooccurrenceCore(n_items=24, topk=3) as core:  # no reservoir size
        with pytest.raises(_lib.IllegalStateException, match="user_cut"):
            core.sampling_enable(20, SEED)
    op = pkg.NonSampledUserInteractionCounterOneInputStreamOperator(1, "SECONDS", n_items=24, top_k=3, user_cut=4)
    try:
        op.sampling_enable(20, SEED, on="device")
        assert op.core.sampled
        assert op.sampling_counters()["fills"] == 0
    finally:
        op.close()


@pytest.mark.parametrize("on", ["host", "device"])
def test_multi_rank_sampled_context_refuses_checkpoints(pkg, on):
    from flink_cooccurrence_amd import _lib

    with pkg.CooccurrenceCore(n_items=24, topk=3, user_cut=4) as core, \
            pkg.CooccurrenceCore(n_items=24, topk=3, user_cut=4) as donor:
        blob = donor.snapshot()  # an (empty) unsampled checkpoint: what restore_parts would take
        core.comm_init_ops(0, 2, _never_called_ops(pkg))
        core.sampling_enable(20, SEED, on=on)
        for call in (core.snapshot_sampled, lambda: core.restore_parts([blob, blob]),
                     lambda: core.restore_sampled(blob)):
            with pytest.raises(_lib.IllegalStateException, match="world > 1") as e:
                call()
            assert "not built yet" in str(e.value)
        assert core.sampling_counters()["fills"] == 0  # the context is still usable
