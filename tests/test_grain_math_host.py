"""The host-only functions of the film grain service (openhevc_amd/csrc/pics_math.hip: oh_grain_hash, oh_grain_gauss, oh_grain_pattern,
oh_grain_uniform, oh_grain_from_sei, oh_grain_block, oh_grain_mean, oh_grain_value, oh_grain_smooth, oh_grain_blend):
tests/grain_math_check.cpp runs them at the extremes of their domains over heap blocks of exactly the sizes they may touch, as a
stand-alone program built with AddressSanitizer and UBSan — no GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_grain_math_under_sanitizers(tmp_path):
    exe = str(tmp_path / "grain_math_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "grain_math_check.cpp"), os.path.join(ROOT, "openhevc_amd", "csrc", "pics_math.hip"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("grain math ok"), r.stdout + r.stderr
    assert len(r.stdout.splitlines()) == 5                               # one line per group, then the verdict
