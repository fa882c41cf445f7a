"""The paired I4 search's lane maps and lane-form state (no GPU):
zw_enc_i4pair.h walked on the host by tools/i4_pair_check.cpp -- for ranks
that are permutations of 0..9 per group (the identity, the reversal, seeded
ones), both step forms and K = 3 and 4, lane (g, k, q) receives exactly the
mode of rank k from a lane of its own group, and lanes k >= K are ineligible;
over seeded sequences of winners the state every lane holds, the contexts it
hands the next step and the two exits equal a plain per-MB model of the scalar
form.  On the device a wrong map is a candidate that transforms another
group's mode, a wrong state a search that ends at another block."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "image-webp_amd", "csrc")
TOOL = os.path.join(ROOT, "tools", "i4_pair_check.cpp")


def test_i4_pair_lane_maps_and_state(tmp_path):
    exe = str(tmp_path / "i4_pair_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", CSRC, TOOL, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
