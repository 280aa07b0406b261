"""The host arithmetic of the picture services (openhevc_amd/csrc/pics_math.hip: coefficients, colour tables, light-level bins, the SSIM
window, resize taps, the blend, the window in a plane class) writes caller-sized arrays from shift, __int128 and llround arithmetic: tests/pics_math_check.cpp runs it
at the extremes of its domain over heap blocks of exactly the documented sizes, as a stand-alone program built with AddressSanitizer
and UBSan — no GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_pics_math_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pics_math_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "pics_math_check.cpp"), os.path.join(ROOT, "openhevc_amd", "csrc", "pics_math.hip"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("pics math ok"), r.stdout + r.stderr
    assert len(r.stdout.splitlines()) == 8                               # one line per group, then the verdict
