"""The host-only functions of the colour remapping service (openhevc_amd/csrc/pics_math.hip: oh_remap_curve, oh_remap_sample,
oh_remap_from_sei, oh_remap_luts): tests/remap_math_check.cpp runs them at the extremes of their domains over heap blocks of exactly the
sizes they may touch — 33 pivots, pivots at 0 and Mi, a single pivot in the middle, descending targets, 12 -> 8 and 8 -> 12,
all-maximal coefficients with all-maximal samples at d = 0 and d = 15, every refusal — as a stand-alone program built with
AddressSanitizer and UBSan — no GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_remap_math_under_sanitizers(tmp_path):
    exe = str(tmp_path / "remap_math_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "remap_math_check.cpp"), os.path.join(ROOT, "openhevc_amd", "csrc", "pics_math.hip"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("remap math ok"), r.stdout + r.stderr
    assert len(r.stdout.splitlines()) == 5                               # one line per group, then the verdict
