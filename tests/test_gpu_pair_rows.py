"""Pass 1 in frame pairs at the edges of its row schedule (PairRowSchedule1 in
image-webp_amd/csrc/zw_enc_rows.h): the slow-row rounds, the join row from
which the chain waves take rows too, the floor under which there is no join,
and the odd last workgroup, whose second chain wave has no chain but still
owns rows.  Small frames, every stream compared byte for byte with the
oracle's.  The heights around the join row and the floor are read from the
header's knobs, so they follow a re-tuned schedule.

Every case runs in a fresh child process with ZW_ENC_FP=1 ZW_ENC_ROWS=0 (read
once per process): both passes then run their frame-pair kernels on any batch
of two frames or more."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import os, sys
sys.path[:0] = [os.path.join(sys.argv[1], "image-webp_amd"), os.path.join(sys.argv[1], "tests")]
import oracle_lib as O
import zwebp
from zwebp.synth import synth_rgba
mbw, mbh, n = (int(v) for v in sys.argv[2:5])
w, h = mbw * 16 - 3, mbh * 16 - 5  # (not whole MBs: the padded edge too)
imgs = [synth_rgba(w, h, 0x5EED9000 + 16 * mbh + i, ("natural", "noise", "flat")[(i + mbh) % 3]) for i in range(n)]
refs = []
for im in imgs:
    rc, ref, _ = O.encode(im, w, h, 3, 75, 4)
    assert rc == 0
    refs.append(ref)
ctx = zwebp.Context(0)
assert zwebp.load_library().zwk_encode_fp(1, mbw, n) == 1, "pass 1 does not run in frame pairs"
out = zwebp.encode_batch(imgs, w, h, zwebp.ColorType.Rgba8, 75, 4, ctx=ctx)
bad = [i for i in range(n) if out[i] != refs[i]]
assert not bad, bad
ctx.close()
print("ok")
"""


def _knob(name):
    src = open(os.path.join(ROOT, "image-webp_amd", "csrc", "zw_enc_rows.h")).read()
    return int(re.search(r"#define %s (\d+)" % name, src).group(1))


def _join_row(mbh):
    num, den, floor = _knob("ZW_P1P_JOIN_NUM"), _knob("ZW_P1P_JOIN_DEN"), _knob("ZW_P1P_JOIN_MIN")
    return mbh if mbh < floor else (mbh * num + den - 1) // den


FLOOR = _knob("ZW_P1P_JOIN_MIN")
J = _join_row(68)  # the join row of the headline's 1080p frames

# (MB columns, MB rows, frames): 2 frames are one pair, 3 a pair and the odd
# last workgroup
CASES = [
    (13, 1, 3),
    (1, 2, 2),
    (2, 7, 3),
    (13, 11, 2),
    (13, 12, 3),
    (2, 13, 2),
    (13, 25, 3),
    (13, FLOOR - 1, 3),
    (13, FLOOR, 2),
    (2, J - 1, 3),
    (13, J, 2),
    (1, J + 1, 3),
    (2, 68, 3),
]


@pytest.mark.parametrize("mbw,mbh,n", CASES)
def test_pair_rows_streams_equal_oracle(mbw, mbh, n):
    env = dict(os.environ, ZW_ENC_FP="1", ZW_ENC_ROWS="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(mbw), str(mbh), str(n)], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
