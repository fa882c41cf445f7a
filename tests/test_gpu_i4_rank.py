"""The paired I4 search's value vector and ranking (i4p_values / i4p_step in
image-webp_amd/csrc/zw_enc_kernels.hip): TrueMotion's sixteen predictions as
clamped value-vector entries, and the modes ranked by byte dot products instead
of an exact SSE (zw_enc_i4pair.h).  Two-frame batches of the extreme-contrast
frames (tests/enc_extreme.py) where these can go wrong: blocks TrueMotion wins,
blocks whose L + T - P leaves 0..255 (whether TrueMotion wins them or has to
keep losing them), and flat neighbourhoods, where DC, TrueMotion, VE and HE
predict alike and the ranking's ties decide the candidates.  Every stream is
compared byte for byte with the oracle's, and the luma and sub-block modes of
both passes and the reconstructed Y plane per MB.

Each case first asserts a census from the oracle's debug output, so it cannot
pass without reaching the code: per frame and per pass, over the MBs whose luma
mode is B and their sub-blocks off the frame's top row and left column,
  tm_win    blocks with sub-mode TrueMotion (1),
  tm_clamp  blocks where L[r] + T[j] - P of the pass's reconstructed plane
            leaves 0..255 for some pixel,
  tm_win_clamp  blocks in both,
  flat      blocks whose L, T and P are all equal.
The floors hold for every frame of the kind and both passes; the oracle gave
(pass 1 / pass 2): tm Q75 m4 tm_win 95 / 71, tm_win_clamp 7 / 3; tm Q98 m4
tm_win_clamp 10 / 8; tm Q75 m3 tm_win_clamp 4 / 2; checker1 Q75 m4 tm_clamp
121 / 121 (tm_win 0 / 0: TrueMotion clamps everywhere and must keep losing);
binnoise Q75 m4 tm_clamp 93 / 106; quilt Q75 m4 tm_win 162 / 203, tm_clamp
255 / 248, flat 4 / 60; quilt Q98 m4 flat 21 / 24; quilt Q30 m4 tm_clamp
239 / 260.  (tm_win over every sub-block of those MBs, the frame's top row and
left column included, is 101 / 81 for tm and 165 / 210 for quilt at Q75 m4;
every other figure is the same either way.)

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

# (argv: the repository root, the case as JSON)
_CHILD = r"""
import json, os, sys
sys.path[:0] = [os.path.join(sys.argv[1], "image-webp_amd"), os.path.join(sys.argv[1], "tests")]
import numpy as np
import enc_extreme as X
import oracle_lib as O
c = json.loads(sys.argv[2])
q, m, kinds = c["q"], c["m"], c["kinds"]
n = len(kinds)
w, h = X.dims(kinds[0])
assert all(X.dims(k) == (w, h) for k in kinds)
mbw, mbh = (w + 15) // 16, (h + 15) // 16
nmb = mbw * mbh
imgs = [X.frame(k) for k in kinds]
refs, dbgs = [], []
for k in kinds:
    ref, dbg = X.oracle(k, q, m)
    refs.append(ref)
    dbgs.append(dbg)

def census(dbg, pass_):
    info = dbg["p%d_info" % pass_]
    R = dbg["recon1_y" if pass_ == 1 else "recon_y"].reshape(mbh * 16, mbw * 16).astype(np.int64)
    cnt = dict(tm_win=0, tm_clamp=0, tm_win_clamp=0, flat=0)
    for k in range(nmb):
        if info[k].luma_mode != 4:
            continue
        mby, mbx = divmod(k, mbw)
        for b in range(16):
            y0, x0 = mby * 16 + (b >> 2) * 4, mbx * 16 + (b & 3) * 4
            if y0 == 0 or x0 == 0:
                continue
            L, T, P = R[y0:y0 + 4, x0 - 1], R[y0 - 1, x0:x0 + 4], R[y0 - 1, x0 - 1]
            tm = L[:, None] + T[None, :] - P
            win = info[k].bpred[b] == 1
            clamp = bool((tm < 0).any() or (tm > 255).any())
            cnt["tm_win"] += int(win)
            cnt["tm_clamp"] += int(clamp)
            cnt["tm_win_clamp"] += int(win and clamp)
            cnt["flat"] += int((L == P).all() and (T == P).all())
    return cnt

for i, k in enumerate(kinds):
    for pass_ in (1, 2):
        cnt = census(dbgs[i], pass_)
        print("census frame %d %s q%d m%d pass %d" % (i, k, q, m, pass_), json.dumps(cnt))
        for key, floor in c["floors"].get(k, {}).items():
            assert cnt[key] >= floor, (k, pass_, key, floor, cnt)

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
out = zwebp.encode_batch(imgs, w, h, X.RGB8, q, m, ctx=ctx)
bad = [i for i in range(n) if out[i] != refs[i]]
p = zwebp.Pipeline(n, w, h, X.RGB8, q, m, ctx=ctx)
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

# floors per frame kind, for every frame of the kind and both passes
Q75 = dict(q=75, m=4, floors=dict(tm=dict(tm_win=50, tm_win_clamp=2), checker1=dict(tm_clamp=100),
                                  binnoise=dict(tm_clamp=80), quilt=dict(tm_win=100, tm_clamp=150, flat=2)))

CASES = {
    # TrueMotion wins (some of its blocks clamped) beside a frame where it clamps everywhere and loses, either way round
    "tm_checker1": dict(Q75, kinds=["tm", "checker1"]),
    "checker1_tm": dict(Q75, kinds=["checker1", "tm"]),
    "tm_binnoise": dict(Q75, kinds=["tm", "binnoise"]),
    # unlike contents as neighbours: wins, clamps and flat four-way ties of DC / TM / VE / HE
    "quilt_quilt": dict(Q75, kinds=["quilt", "quilt"]),
    # both ends of the quantiser and K = 3
    "tm_tm_q98": dict(q=98, m=4, kinds=["tm", "tm"], floors=dict(tm=dict(tm_win_clamp=5))),
    "tm_tm_m3": dict(q=75, m=3, kinds=["tm", "tm"], floors=dict(tm=dict(tm_win_clamp=1))),
    "quilt_quilt_q98": dict(q=98, m=4, kinds=["quilt", "quilt"], floors=dict(quilt=dict(flat=10))),
    "quilt_quilt_q30": dict(q=30, m=4, kinds=["quilt", "quilt"], floors=dict(quilt=dict(tm_clamp=150))),
}


def run_case(name):
    env = dict(os.environ, ZW_ENC_FP="1", ZW_ENC_ROWS="0")
    return subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(CASES[name])], env=env,
                          capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("name", list(CASES))
def test_i4_rank_equals_oracle(name):
    r = run_case(name)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
