"""The host-only checks across the parts of one checkpoint -- snap_check_parts, the step of cooc_restore_finish_parts
that needs only the parts' headers and scalars (cooc_snapshot.cpp: no device code) -- compiled with AddressSanitizer
and UndefinedBehaviorSanitizer (g++) and driven by the stand-alone tests/sanitize/snapshot_parts_fuzz.cpp:
consistent sets of part heads, every single-field disagreement, permuted and duplicated ranks, n_parts of 0, 1
and 5,000, random heads.  Only the consistent sets may pass, and any out-of-bounds access or undefined operation
aborts the driver.  Nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flink-cooccurrence_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cross_part_checks_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "snapshot_parts_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-Wall", "-o", exe,
           os.path.join(ROOT, "tests", "sanitize", "snapshot_parts_fuzz.cpp"), os.path.join(CSRC, "cooc_snapshot.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    # (verify_asan_link_order=0: the environment may preload a library ahead of the sanitizer runtime)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "snapshot_parts_fuzz ok" in r.stdout


def test_parts_entry_points_are_bound(pkg):
    """declared in the header, exported by the library, bound in _lib.py; the ABI version is unchanged"""
    from flink_cooccurrence_amd import _lib

    L = _lib.load()
    for name in ("cooc_restore_begin_parts", "cooc_restore_write_part", "cooc_restore_finish_parts"):
        assert name in pkg.header_symbols() and getattr(L, name).argtypes is not None
    assert L.cooc_abi_version() == 7
    assert (_lib.COOC_ROUTE_MOD, _lib.COOC_ROUTE_BITMAP) == (0, 1)
    assert hasattr(pkg.CooccurrenceCore, "restore_parts")
