"""The host work of the hand-over that several threads share — the check-and-count of a chunk's lists, the claimed staging copy and the
helper pool (openhevc_amd/csrc/handover_host.h) — and the vectorised pack_bs (handover_layout.h) are pure host code:
tests/handover_parallel_check.cpp runs them as a stand-alone program, built once with AddressSanitizer and UBSan and once with
ThreadSanitizer — no GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.parametrize("name, flags", [
    ("asan_ubsan", ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]),
    ("tsan", ["-Xarch_host", "-fsanitize=thread"]),
])
def test_handover_parallel_under_sanitizers(tmp_path, name, flags):
    exe = str(tmp_path / f"handover_parallel_check_{name}")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", *flags,
                    os.path.join(ROOT, "tests", "handover_parallel_check.cpp"), "-o", exe, "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "200 refused chunks" in r.stdout and " ok" in r.stdout
