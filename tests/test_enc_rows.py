"""The encode kernels' row schedule (no GPU): image-webp_amd/csrc/zw_enc_rows.h
walked on the host for the shipped shapes -- every MB row owned by exactly one
luma wave and visited once by first_row / next_row (tools/enc_rows_check.cpp).
On the device a wrong schedule is a hang."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_schedule(tmp_path):
    exe = str(tmp_path / "enc_rows_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "image-webp_amd", "csrc"),
                           os.path.join(ROOT, "tools", "enc_rows_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr
