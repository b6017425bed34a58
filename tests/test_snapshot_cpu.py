"""The snapshot blob's header and directory parser -- cooc_snapshot_inspect, which is also the first check of
cooc_restore_finish on untrusted bytes (cooc_snapshot.cpp: host-only, no device code) -- compiled with
AddressSanitizer and UndefinedBehaviorSanitizer (g++) and driven by the stand-alone tests/sanitize/snapshot_fuzz.cpp:
hand-built valid blobs, every truncation, every single-bit flip of the header and directory, random bytes, and
directories with overlapping, misaligned, out-of-range or overflowing (offset, bytes, count).  Only the valid ones
may pass, and any out-of-bounds access or undefined operation aborts the driver.  Nothing sanitized is loaded
into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flink-cooccurrence_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_snapshot_header_parser_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "snapshot_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "sanitize", "snapshot_fuzz.cpp"),
           os.path.join(CSRC, "cooc_snapshot.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    # (verify_asan_link_order=0: the environment may preload a library ahead of the sanitizer runtime)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "snapshot_fuzz ok" in r.stdout


def test_library_inspect_refuses_garbage(pkg):
    """The same parser through the built library and the Python binding: no context, no device."""
    with pytest.raises(pkg.IllegalArgumentException):
        pkg.CooccurrenceCore.snapshot_info(b"")
    with pytest.raises(pkg.IllegalArgumentException) as e:
        pkg.CooccurrenceCore.snapshot_info(b"COOCSNP1" + bytes(1000))
    assert "snapshot blob" in str(e.value)
