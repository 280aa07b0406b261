"""The host-only functions of the warp service (openhevc_amd/csrc/pics_math.hip: oh_warp_position, oh_warp_cubic, oh_warp_interp,
oh_warp_paths and the map builders): tests/warp_math_check.cpp runs them at the extremes of their domains over heap blocks of exactly
the sizes they may touch, as a stand-alone program built with AddressSanitizer and UBSan — no GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_warp_math_under_sanitizers(tmp_path):
    exe = str(tmp_path / "warp_math_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "warp_math_check.cpp"), os.path.join(ROOT, "openhevc_amd", "csrc", "pics_math.hip"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("warp math ok"), r.stdout + r.stderr
    assert len(r.stdout.splitlines()) == 8                               # one line per group, then the verdict
