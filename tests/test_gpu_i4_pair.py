"""The frame-pair kernels' paired I4 search (i4p_step / pick_i4_pair in
image-webp_amd/csrc/zw_enc_kernels.hip): the candidate modes of the four
(MB, slot) groups from the inverse-rank permute, and the search's running
state held in lanes (zw_enc_i4pair.h).  Small frames at the shapes where a
step can go wrong: one MB (the one-block steps only, no top-right), one MB row
and one MB column (the top-right and left borders), K = 3 and 4, K = 10 (the
single form, untouched), pairs in which one MB or both are never searched, the
odd last workgroup, and both ends of the quantiser.  Every stream is compared
byte for byte with the oracle's, and the reconstructed Y plane per MB and the
luma and sub-block modes of both passes, so that a candidate that transformed
another group's mode, or a search that ended at another block, shows up as an
MB.  The classes of MB positions a case is there for (both I16 / mixed / both
I4 in frames 0 and 1 by the oracle's pass-2 modes; `i4_lost`: searches the
oracle started and ended early, over both passes and every frame) are counted
from the oracle's debug output and asserted.

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

# (argv: the repository root, the case as JSON, "oracle" to stop after the classes)
_CHILD = r"""
import json, os, sys
sys.path[:0] = [os.path.join(sys.argv[1], "image-webp_amd"), os.path.join(sys.argv[1], "tests")]
import numpy as np
import oracle_lib as O
from zwebp.shard import frame_seed
from zwebp.synth import synth_rgba
c = json.loads(sys.argv[2])
w, h, q, m, kinds = c["w"], c["h"], c["q"], c["m"], c["kinds"]
n = len(kinds)
mbw, mbh = (w + 15) // 16, (h + 15) // 16
nmb = mbw * mbh
imgs = [synth_rgba(w, h, frame_seed(i), kinds[i]) for i in range(n)]
refs, dbgs = [], []
for im in imgs:
    rc, ref, dbg = O.encode(im, w, h, 3, q, m, debug=True)
    assert rc == 0
    refs.append(ref)
    dbgs.append(dbg)
# the classes of MB positions of frames 0 and 1, by the oracle's pass-2 luma modes
i4 = [np.array([dbgs[f]["p2_info"][k].luma_mode == 4 for k in range(nmb)]) for f in (0, 1)]
cls = {"both_i16": int((~i4[0] & ~i4[1]).sum()), "mixed": int((i4[0] ^ i4[1]).sum()), "both_i4": int((i4[0] & i4[1]).sum()),
       "i4_lost": int(sum(sum(d["i4_exit_score"]) + sum(d["i4_exit_hdr"]) for d in dbgs))}
print("classes", json.dumps(cls))
for k, v in c.get("classes_min", {}).items():
    assert cls[k] >= v, (k, cls)
for k, v in c.get("classes_max", {}).items():
    assert cls[k] <= v, (k, cls)
if len(sys.argv) > 3 and sys.argv[3] == "oracle":
    sys.exit(0)

def modes_of(info):
    a = np.array([[info[k].luma_mode] + list(info[k].bpred) for k in range(nmb)], np.uint8)
    a[a[:, 0] != 4, 1:] = 0
    return a

def check(p, i, pass_, recon):
    g, _ = p.mbinfo(i, pass_)
    g = g[:, [0] + list(range(4, 20))].copy()
    g[g[:, 0] != 4, 1:] = 0
    o = modes_of(dbgs[i]["p%d_info" % pass_])
    d = np.nonzero((g != o).any(axis=1))[0]
    assert d.size == 0, "frame %d pass %d modes: %d MBs differ, first (y, x) %s: %s vs %s" % (
        i, pass_, d.size, divmod(int(d[0]), mbw), g[d[0]].tolist(), o[d[0]].tolist())
    A, B = p.planes(i, 1)[0].reshape(mbh * 16, mbw * 16), dbgs[i][recon].reshape(mbh * 16, mbw * 16)
    d = np.argwhere((A != B).reshape(mbh, 16, mbw, 16).any(axis=(1, 3)))
    assert d.size == 0, "frame %d %s: %d MBs differ, first (y, x) %s" % (i, recon, len(d), d[0].tolist())

import zwebp
L = zwebp.load_library()
assert L.zwk_encode_fp(1, mbw, n) == 1, "pass 1 does not run in frame pairs"
assert L.zwk_encode_fp(2, mbw, n) == 1, "pass 2 does not run in frame pairs"
ctx = zwebp.Context(0)
out = zwebp.encode_batch(imgs, w, h, zwebp.ColorType.Rgba8, q, m, ctx=ctx)
bad = [i for i in range(n) if out[i] != refs[i]]
p = zwebp.Pipeline(n, w, h, zwebp.ColorType.Rgba8, q, m, ctx=ctx)
for i in range(n):
    p.upload(i, imgs[i])
p.run_pass1(True)
for i in range(n):
    check(p, i, 1, "recon1_y")
p.encode()
for i in range(n):
    check(p, i, 2, "recon_y")
    assert p.output(i) == refs[i], "pipeline stream %d" % i
p.close()
assert not bad, bad
ctx.close()
print("ok")
"""

N136 = dict(w=136, h=72, q=75, m=4, kinds=["natural", "natural"])  # 9 x 5 MBs, ragged both ways
ALL3 = dict(both_i16=5, mixed=5, both_i4=5)

CASES = {
    # K = 4 at three quantisers; searches that win, and searches that start and lose to I16
    "q75": dict(N136, classes_min=dict(ALL3, i4_lost=1)),
    "q90": dict(N136, q=90, classes_min=dict(ALL3, i4_lost=1)),
    "q30": dict(N136, q=30, classes_min=dict(both_i16=5, i4_lost=1)),
    # one MB: the one-block steps' borders only, no top-right MB
    "one_mb_noise_q98": dict(w=16, h=16, q=98, m=4, kinds=["noise", "noise"], classes_min=dict(both_i16=1, i4_lost=1)),
    # one MB row (the top-right border of every MB) and one MB column (the left border)
    "one_row": dict(w=32, h=16, q=75, m=4, kinds=["natural", "natural"], classes_min=dict(both_i4=2)),
    "one_column": dict(w=16, h=32, q=75, m=4, kinds=["natural", "natural"], classes_min=dict(both_i4=2)),
    # K = 3: quad 3 of every group is never eligible
    "method3": dict(N136, m=3, classes_min=dict(mixed=5, both_i4=1, i4_lost=1)),
    "method2": dict(N136, m=2, classes_min=dict(mixed=5, both_i4=1, i4_lost=1)),
    # K = 10: the single form, which this search falls through to
    "method5": dict(N136, m=5, classes_min=dict(both_i4=5)),
    # one MB of a pair, or both, never searched
    "natural_flat": dict(N136, kinds=["natural", "flat"], classes_min=dict(mixed=5), classes_max=dict(both_i4=0)),
    "flat_flat": dict(N136, kinds=["flat", "flat"], classes_max=dict(mixed=0, both_i4=0)),
    # three frames: a pair and the odd last workgroup
    "three_frames": dict(w=200, h=120, q=75, m=4, kinds=["natural"] * 3, classes_min=dict(ALL3, i4_lost=1)),
    # both ends of the quantiser
    "q1": dict(N136, q=1, classes_min=dict(both_i16=5, i4_lost=1)),
    "q100": dict(N136, q=100, classes_min=dict(both_i4=5)),
}


def run_case(name, *more):
    env = dict(os.environ, ZW_ENC_FP="1", ZW_ENC_ROWS="0")
    return subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(CASES[name]), *more], env=env,
                          capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("name", list(CASES))
def test_i4_pair_equals_oracle(name):
    r = run_case(name)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
