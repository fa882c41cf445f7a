"""The encoder's device-tensor input, walked on the host (no GPU): zw_ingest.h by
tools/ingest_check.cpp -- the pixel rule over all 65 536 f16 bit patterns and over
f32 values around every k + 0.5 tie, the clamps, NaN and +-inf, against an
independent double-precision statement; the vector-run predicate (no accepted run's
load is misaligned or leaves its row, widths 1..40); the argument check against the
span formula of test_gpu_dec_device.py.  On the device a wrong predicate or check is
a load outside the caller's tensor."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "image-webp_amd", "csrc")
TOOL = os.path.join(ROOT, "tools", "ingest_check.cpp")


def _build(tmp_path):
    exe = str(tmp_path / "ingest_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, TOOL, "-o", exe])
    return exe


def test_ingest_rule_predicate_and_span(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr


def test_ingest_rule_matches_numpy(tmp_path):
    """The tool's `rule` mode prints the header's byte for f32 inputs read from stdin;
    numpy's float32 multiply, add, clip and rint (the statement the GPU tests use for
    their expected images) gives the same bytes."""
    exe = _build(tmp_path)
    rng = np.random.default_rng(0x5EED)
    ks = np.arange(-2, 258, dtype=np.float32)
    x = np.concatenate([ks + np.float32(0.5), ks - np.float32(0.49), ks + np.float32(0.49),
                        rng.uniform(-40, 300, 4000).astype(np.float32),
                        np.asarray([np.nan, np.inf, -np.inf, 1e-45, -0.0, 3e38], np.float32)])
    for scale, bias in ((1.0, 0.0), (255.0 * 0.229, 255.0 * 0.485), (0.5, 0.25), (-1.0, 255.0)):
        s, b = np.float32(scale), np.float32(bias)
        with np.errstate(all="ignore"):
            xs = ((x - b) / s).astype(np.float32)
        text = "".join(f"{int(v)}\n" for v in xs.view(np.uint32))
        out = subprocess.run([exe, "rule", str(int(s.view(np.uint32))), str(int(b.view(np.uint32)))], input=text,
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        got = np.array([int(v) for v in out.stdout.split()], np.uint8)
        with np.errstate(all="ignore"):
            t = xs * s
            t = t + b
            want = np.rint(np.clip(t, np.float32(0), np.float32(255)))
        want[np.isnan(t)] = 0
        assert got.shape == want.shape and np.array_equal(got, want.astype(np.uint8)), (scale, bias)
