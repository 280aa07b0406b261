"""The engine's switches (openhevc_amd/csrc/engine_tuning.h) and the launch plan of the intra pass (openhevc_amd/csrc/intra_plan.h)
are pure host code: tests/intra_plan_check.cpp runs them against tables written out by hand, as a stand-alone program built with
AddressSanitizer and UBSan — no GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_intra_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "intra_plan_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "intra_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plan ok" in r.stdout
