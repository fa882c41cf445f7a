"""The encode pipeline's cross-thread progress counter (no GPU):
image-webp_amd/csrc/zw_progress.h under three producers and a consumer, and
the rules of its stopped state (tools/progress_check.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_progress_counter(tmp_path):
    exe = str(tmp_path / "progress_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "image-webp_amd", "csrc"),
                           os.path.join(ROOT, "tools", "progress_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr
