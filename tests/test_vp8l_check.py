"""The VP8L / ALPH reader over damaged input, on the host (no GPU):
tools/vp8l_check.cpp over csrc/zw_vp8l_dec.cpp alone, built with
-fsanitize=address,undefined as a program of its own.  It decodes every
fixture's ALPH or VP8L payload, then its truncations and seeded single-byte
flips; every call must return ZW_OK or a decoder code, and the sanitizers stop
the run at any access out of bounds.  The reader sees untrusted bytes: on the
library's host threads a fault there would take the caller's process down."""
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "vp8l_check.cpp")
SRC = os.path.join(ROOT, "image-webp_amd", "csrc", "zw_vp8l_dec.cpp")
ALPHA = os.path.join(ROOT, "tests", "golden", "alpha")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("vp8l_check") / "vp8l_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", TOOL, SRC, "-o", path])
    return path


def _run(exe, files):
    assert files
    out = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith(f"ok {len(files)} files"), out.stdout + out.stderr[-4000:]


def test_small_fixtures_every_truncation_and_flips(exe):
    _run(exe, sorted(glob.glob(os.path.join(ALPHA, "alpha_*.webp")) + glob.glob(os.path.join(ALPHA, "ll_*.webp"))))


def test_gallery_fixtures_truncations_and_flips(exe):
    _run(exe, sorted(glob.glob(os.path.join(ALPHA, "gallery_*.webp"))))
