"""cooc_count_owned below 40,320 items, the parts a machine without a GPU can check: the ABI did not move (no new
symbol, no struct change), and the header, DESIGN and INTEGRATION state the small-universe exchange.  The GPU side is
tests/test_count_owned_small_multiproc.py, tests/test_sample_owned_small_multiproc.py and tests/test_gpu_owned_small.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _text(name):
    return " ".join(open(os.path.join(ROOT, name)).read().split())


def _header():
    # (comment continuation stars folded away, so that a sentence reads the same wherever its lines break)
    return " ".join(re.sub(r"^\s*\*\s?", "", ln) for ln in open(os.path.join(ROOT, "include", "cooc.h"))).split()


def test_abi_version_stays_7(pkg):
    from flink_cooccurrence_amd import _lib

    assert _lib.load().cooc_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "cooc.h")).read()
    assert re.search(r"#define\s+COOC_ABI_VERSION\s+7\b", header)
    # no new entry point for the small universe: the same four calls
    assert sorted(s for s in pkg.header_symbols() if "owned" in s) == [
        "cooc_count_device_owned", "cooc_count_owned", "cooc_count_owned_host", "cooc_sample_owned", "cooc_topk_owned",
        "cooc_topk_owned_host"]


def test_header_states_the_small_universe_contract():
    h = " ".join(_header())
    assert ("Small universes: below 40,320 items cooc_count_owned runs the records exchange over the communicator, and "
            "row a is complete on rank a mod world.") in h
    assert "always a padded CSR over all n_items rows" in h
    assert "Errors never leave a peer waiting (small universes)." in h
    assert "every rank returns COOC_ERR_ARG before any payload moves or any other collective starts" in h
    # cooc_sample_owned's reservoirs feed cooc_count_owned in both universes
    assert "a valid input of cooc_count_owned in both universes" in h


def test_design_and_integration_state_it():
    design = _text("DESIGN.md")
    assert ("Small universes: `cooc_count_owned` runs the records exchange over the context's communicator, and row a "
            "is complete on rank a mod world.") in design
    assert "The padding reaches the send buffer by a copy" in design and "the choice rests on no measurement" in design
    assert "Any p > 1 time is unmeasured on a one-GPU box." in design
    assert "tests/test_count_owned_small_multiproc.py" in design
    integ = _text("INTEGRATION.md")
    assert "The owned operators work below 40,320 items too" in integ
    assert "records exchange" in _text("README.md")
    # what tests/test_sampled_comm_cpu.py looks for is still there
    for name in ("DESIGN.md", "INTEGRATION.md", "README.md"):
        assert "Not yet: checkpoints of a sampled multi-rank job" in _text(name), name


def test_sharding_names_the_communicator_for_a_small_universe(pkg):
    """the refusal is decided before any collective, from the core alone (no GPU, no process group)"""
    import pytest

    from flink_cooccurrence_amd import sharding

    class Core:  # what sharding.count_owned reads of a CooccurrenceCore without a communicator
        n_items, comm_world, general_planner = 301, 0, False

    with pytest.raises(RuntimeError, match=r"init_comm / init_comm_torch_ops"):
        sharding.count_owned(Core(), None, None)
