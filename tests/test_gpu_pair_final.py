"""The frame-pair kernels' paired final luma transform (final_luma_pair in
image-webp_amd/csrc/zw_enc_kernels.hip): two I16 MBs of a frame pair worked in
one pass of the wave, with the trellis runs of both numbered onto the wave's
lanes (zw_enc_pairfinal.h) -- one trellis call when they are 64 at the most,
one per frame otherwise -- and the per-frame path for everything else (an I4
MB in either frame, the odd last workgroup).  Small frames; every stream is
compared byte for byte with the oracle's, and where it says so the
reconstructed planes too, so that a block that gathered the wrong lane's levels
shows up as a block.  The classes of MB positions a case is chosen for (both
I16 / mixed / both I4 in frames 0 and 1, by the oracle's pass-2 modes) are
counted from the oracle's debug output and asserted.

Every case runs in a fresh child process with ZW_ENC_FP=1 ZW_ENC_ROWS=0 (read
once per process): both passes then run their frame-pair kernels on any batch
of two frames or more."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import json, os, sys
sys.path[:0] = [os.path.join(sys.argv[1], "image-webp_amd"), os.path.join(sys.argv[1], "tests")]
import numpy as np
import oracle_lib as O
import zwebp
from zwebp.shard import frame_seed
from zwebp.synth import synth_rgba
c = json.loads(sys.argv[2])
w, h, q, m, kinds = c["w"], c["h"], c["q"], c["m"], c["kinds"]
n = len(kinds)
mbw, mbh = (w + 15) // 16, (h + 15) // 16
imgs = [synth_rgba(w, h, frame_seed(i), kinds[i]) for i in range(n)]
refs, dbgs = [], []
for im in imgs:
    rc, ref, dbg = O.encode(im, w, h, 3, q, m, debug=True)
    assert rc == 0
    refs.append(ref)
    dbgs.append(dbg)
# the classes of MB positions of frames 0 and 1, by the oracle's pass-2 luma modes
i4 = [np.array([dbgs[f]["p2_info"][k].luma_mode == 4 for k in range(mbw * mbh)]) for f in (0, 1)]
cls = {"both_i16": int((~i4[0] & ~i4[1]).sum()), "mixed": int((i4[0] ^ i4[1]).sum()), "both_i4": int((i4[0] & i4[1]).sum())}
print("classes", cls)
for k, v in c.get("classes_min", {}).items():
    assert cls[k] >= v, (k, cls)
L = zwebp.load_library()
assert L.zwk_encode_fp(1, mbw, n) == 1, "pass 1 does not run in frame pairs"
assert L.zwk_encode_fp(2, mbw, n) == 1, "pass 2 does not run in frame pairs"
ctx = zwebp.Context(0)
out = zwebp.encode_batch(imgs, w, h, zwebp.ColorType.Rgba8, q, m, ctx=ctx)
bad = [i for i in range(n) if out[i] != refs[i]]
if c.get("recon"):
    p = zwebp.Pipeline(n, w, h, zwebp.ColorType.Rgba8, q, m, ctx=ctx)
    for i in range(n):
        p.upload(i, imgs[i])
    p.encode()
    for i in range(n):
        for a, name, mb in zip(p.planes(i, 1), ("recon_y", "recon_u", "recon_v"), (16, 8, 8)):
            A, B = a.reshape(mbh * mb, mbw * mb), dbgs[i][name].reshape(mbh * mb, mbw * mb)
            d = np.argwhere((A != B).reshape(mbh, mb, mbw, mb).any(axis=(1, 3)))
            assert d.size == 0, "frame %d %s: %d MBs differ, first (y, x) %s" % (i, name, len(d), d[0].tolist())
        assert p.output(i) == refs[i], "pipeline stream %d" % i
    p.close()
assert not bad, bad
ctx.close()
print("ok")
"""

N136 = dict(w=136, h=72, q=75, m=4, kinds=["natural", "natural"])  # 9 x 5 MBs, ragged both ways
ALL3 = dict(both_i16=5, mixed=5, both_i4=5)

CASES = {
    # both I16 within one trellis call, and the per-frame path for mixed and I4
    "q75_one_call": dict(N136, recon=True, classes_min=ALL3),
    # no trivially zero block: 80 tasks, one call per frame
    "q90_two_calls": dict(N136, q=90, recon=True, classes_min=ALL3),
    # one MB column and one MB row
    "one_mb_noise_q98": dict(w=16, h=16, q=98, m=4, kinds=["noise", "noise"], classes_min=dict(both_i16=1)),
    # three frames: a pair and the odd last workgroup; the chroma reconstruction too
    "three_frames_q75": dict(w=200, h=120, q=75, m=4, kinds=["natural"] * 3, recon=True, classes_min=ALL3),
    "three_frames_q30": dict(w=200, h=120, q=30, m=4, kinds=["natural"] * 3, recon=True),
    # a pair in which one MB, or both, need no task
    "natural_flat": dict(N136, kinds=["natural", "flat"]),
    "flat_flat": dict(N136, kinds=["flat", "flat"]),
    # the paired form without the trellis in pass 2 (methods below 4), and the other methods
    "method2": dict(N136, m=2),
    "method3": dict(N136, m=3),
    "method5": dict(N136, m=5),
    "method6": dict(N136, m=6),
}


@pytest.mark.parametrize("name", list(CASES))
def test_pair_final_streams_equal_oracle(name):
    env = dict(os.environ, ZW_ENC_FP="1", ZW_ENC_ROWS="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(CASES[name])], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
