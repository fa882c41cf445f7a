"""The paired I4 search's value vector and ranking key (no GPU):
zw_enc_i4pair.h walked on the host by tools/i4_rank_check.cpp -- for extreme
and seeded edge vectors the 55 entries, formed lane by lane as the kernel forms
them, give every pixel of the ten modes through the paired index table exactly
what the ten predictors written plainly from the VP8 rules give, TrueMotion's
sums below 0 and above 255 included; and for extreme and seeded sources and
predictions, ties of two, four and ten modes among them, the ranks by the
byte-dot key equal the ranks by sse << 4 | mode, with the key inside its
bounds.  On the device a wrong entry is a mode predicted from another edge
pixel, a wrong key another set of candidates."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "image-webp_amd", "csrc")
TOOL = os.path.join(ROOT, "tools", "i4_rank_check.cpp")


def test_i4_rank_value_vector_and_key(tmp_path):
    exe = str(tmp_path / "i4_rank_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", CSRC, TOOL, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
