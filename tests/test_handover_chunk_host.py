"""The arena of a chunk of work lists — the lists of one oh_frames_upload call in one arena, copied parts first — its split binding and
the staging jobs of a group (openhevc_amd/csrc/handover_layout.h) are pure host code: tests/handover_chunk_check.cpp runs them over
small host arrays as a stand-alone program built with AddressSanitizer and UBSan — no GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_handover_chunk_under_sanitizers(tmp_path):
    exe = str(tmp_path / "handover_chunk_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "handover_chunk_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "chunks ok" in r.stdout
