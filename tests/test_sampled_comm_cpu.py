"""The sampled mode across ranks, the parts that need no GPU: the Python entry point is there and the ABI version is
unchanged; the host sampler's multi-rank window (cooc_sample.cpp, Sampler::RankCut: the cut at count + base + rho,
the commit from the job's totals, the peers' feedbacks) compiled with AddressSanitizer and
UndefinedBehaviorSanitizer (g++) and driven by the stand-alone tests/sanitize/sample_comm_fuzz.cpp, where W samplers
must decide, rank after rank, what one sampler decides for the serialised window.  Nothing sanitized is loaded
into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flink-cooccurrence_amd", "csrc")


def test_sampling_enable_is_bound_and_the_abi_is_unchanged(pkg):
    from flink_cooccurrence_amd import _lib

    assert _lib.load().cooc_abi_version() == 7
    for cls in (pkg.CooccurrenceCore, pkg.NonSampledUserInteractionCounterOneInputStreamOperator):
        assert callable(getattr(cls, "sampling_enable"))


def test_docs_state_the_contract_and_the_open_end():
    """no "Not yet" for the communicator any more; the checkpoints of a sampled multi-rank job are the open end"""
    for name in ("include/cooc.h", "DESIGN.md", "INTEGRATION.md", "README.md"):
        text = " ".join(open(os.path.join(ROOT, name)).read().split())
        assert "owners across ranks would need the feedback exchanged" not in text, name
        assert "rank-major" in text, name
        assert "Not yet: checkpoints of a sampled multi-rank job" in text, name


def test_host_sampler_ranks_equal_the_serialised_window_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "sample_comm_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-Wall", "-o", exe,
           os.path.join(ROOT, "tests", "sanitize", "sample_comm_fuzz.cpp"), os.path.join(CSRC, "cooc_sample.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    # (verify_asan_link_order=0: the environment may preload a library ahead of the sanitizer runtime)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "sample_comm_fuzz ok" in r.stdout
