"""The frame packing SEI reader (openhevc_amd/csrc/annexb.c: oh_sei_frame_packing): tests/frame_packing_sei_check.c runs it over NAL
units in heap blocks of exactly their sizes — every arrangement type with every flag pattern, the longest ids, every truncation of unit
and payload, zero runs that need emulation prevention, two messages in one unit, arbitrary payloads — as a stand-alone program built
with AddressSanitizer and UBSan — no GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CC = os.environ.get("CC", "gcc")


def test_frame_packing_sei_under_sanitizers(tmp_path):
    exe = str(tmp_path / "frame_packing_sei_check")
    subprocess.run([CC, "-std=gnu99", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "frame_packing_sei_check.c"), os.path.join(ROOT, "openhevc_amd", "csrc", "annexb.c"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("frame packing sei ok"), r.stdout + r.stderr
    assert len(r.stdout.splitlines()) == 6                               # one line per group, then the verdict
