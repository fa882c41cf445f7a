"""The lossless decode's transform kernels (csrc/zw_vp8l_kernels.hip) through
zw_dbg_vp8l_inverse_device, bit for bit against the plain restatement
tests/vp8l_ref.py on its case list (test_vp8l_inverse.py pins the same list on
the host inverses): the predictor alone over widths, heights, block sizes and
each mode undiluted, cross-colour, subtract-green, colour indexing with every
index width and indices past the table, chains in several orders, and one call
of nine images with different lists.

The cases run in one child process (torch's HIP runtime has to start before the
library loads, as in test_gpu_dec_device.py); each prints a line, and the tests
below look their lines up."""
import os
import subprocess
import sys

import pytest

import vp8l_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "image-webp_amd"), os.path.join(ROOT, "tests")]))

_CASES = r"""
import traceback
import numpy as np
import torch                      # torch's HIP runtime first, then the library (as bench.py does)
torch.zeros(1, device=torch.device("cuda", 0))
import zwebp
import vp8l_ref as V

ctx = zwebp.Context(0)
for name in sorted(V.CASES):
    try:
        w, h, images, want = V.case(name)
        got = zwebp.dbg_vp8l_inverse_device(V.hook_images(images), w, h, ctx=ctx)
        assert got.shape == want.shape, (got.shape, want.shape)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{len(bad)} bytes differ, the first at (image, y, x, c) = {bad[0].tolist()}"
        print("case", name, "ok", flush=True)
    except Exception:
        print("case", name, "FAIL", traceback.format_exc().replace("\n", " | "), flush=True)
print("done", flush=True)
"""


@pytest.fixture(scope="module")
def lines():
    out = subprocess.run([sys.executable, "-c", _CASES], env=ENV, capture_output=True, text=True, timeout=600)
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "done" in out.stdout, text[-6000:]
    return {ln.split(" ok")[0].split(" FAIL")[0]: ln for ln in out.stdout.splitlines() if ln.startswith("case ")}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(V.CASES))
def test_gpu_vp8l_inverse(lines, name):
    assert f"case {name}" in lines, f"case {name} did not run"
    assert lines[f"case {name}"].endswith(" ok"), lines[f"case {name}"]
