"""Sampled mode, the parts that need no GPU: the new entry points are declared, exported and bound; the host side
(cooc_sample.cpp: item cut, reservoir decisions, feedback) compiled with AddressSanitizer and
UndefinedBehaviorSanitizer (g++) and driven by the stand-alone tests/sanitize/sample_fuzz.cpp, whose decisions for
the reference log are compared line by line with the pure-Python model's (tests/_sampled_model.py); the draw's
acceptance rate.  Nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import pytest

import _sampled_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flink-cooccurrence_amd", "csrc")
SEED = 0xC0FFEE


def test_sampled_entry_points_are_bound(pkg):
    """declared in the header, exported by the library, bound in _lib.py; the ABI version is unchanged"""
    from flink_cooccurrence_amd import _lib

    L = _lib.load()
    for name in ("cooc_sampling_enable", "cooc_sampling_counters", "cooc_copy_user_history"):
        assert name in pkg.header_symbols() and getattr(L, name).argtypes is not None
    assert L.cooc_abi_version() == 7
    for cls in (pkg.CooccurrenceCore, pkg.NonSampledUserInteractionCounterOneInputStreamOperator):
        assert hasattr(cls, "user_history") and hasattr(cls, "sampling_counters")


def test_jvm_natives_and_declarations_one_for_one():
    """every native of cooc_jni.c has its declaration in CoocNative.java and the other way round"""
    import re

    jni = open(os.path.join(ROOT, "flink-cooccurrence_amd", "jvm", "jni", "cooc_jni.c")).read()
    java = open(os.path.join(ROOT, "flink-cooccurrence_amd", "jvm", "src", "main", "java", "com", "github", "uce",
                             "flinkcooccurrences", "CoocNative.java")).read()
    natives = set(re.findall(r"Java_com_github_uce_flinkcooccurrences_CoocNative_(\w+)\(", jni))
    declared = set(re.findall(r"\bnative\s+[\w\[\]]+\s+(\w+)\(", java))
    assert natives == declared
    assert "samplingEnable" in natives


@pytest.fixture(scope="module")
def sample_fuzz(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("sample_fuzz") / "sample_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "sanitize", "sample_fuzz.cpp"),
           os.path.join(CSRC, "cooc_sample.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def _run(exe, *args):
    # (verify_asan_link_order=0: the environment may preload a library ahead of the sanitizer runtime)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_host_sampler_random_logs_under_asan_ubsan(sample_fuzz):
    """random logs: k < total, counters >= 0 (and <= item_cut), |H| <= user_cut, replaced slots inside the reservoir"""
    assert "sample_fuzz ok" in _run(sample_fuzz)


def test_host_sampler_decisions_equal_the_models(sample_fuzz, tmp_path):
    """the reference log's decisions, record by record, and the final counters"""
    windows = sm.reference_log()
    path = tmp_path / "log.txt"
    path.write_text("".join("".join(f"{u} {i}\n" for u, i in w) + "w\n" for w in windows))
    got = _run(sample_fuzz, str(path), "20", "4", hex(SEED), "24").split("\n")
    model = sm.SampledModel(24, 20, 4, SEED)
    want = []
    for w in windows:
        want += model.window(w).decisions + ["w"]
    c = model.counters()
    want.append("counters %d %d %d %d %d %d" % (c["item_cut_rejections"], c["fills"], c["replacements"],
                                                 c["feedbacks"], c["users"], c["item_counter_sum"]))
    assert got[: len(want)] == want
    assert (c["fills"], c["replacements"], c["feedbacks"], c["item_cut_rejections"]) == (48, 55, 137, 240)


def test_draw_acceptance():
    """seed 0xC0FFEE, users 0..199,999, total = 1000, user_cut = 100: the draws with k < 100 number 20,000 within
    6 sigma = 6 sqrt(200,000 x 0.1 x 0.9) = 805 (the model gives 20,036)"""
    n = sum(1 for u in range(200_000) if sm.draw(SEED, u, 1000) < 100)
    assert abs(n - 20_000) <= 805, n
