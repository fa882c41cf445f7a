"""The paired final luma transform's task masks (no GPU): zw_enc_pairfinal.h
walked on the host by tools/pair_final_check.cpp -- the need masks against
their definition over all 2^16 trivially-zero patterns x 256 edge settings, at
most 40 tasks an MB, the raster chain's context always in the block's mask,
the numbering of two MBs' tasks a bijection, the one-call decision -- and the
trivially-zero predicate pinned against the oracle's trellis.  On the device a
wrong mask is a block that gathers another block's levels."""
import os
import subprocess

import numpy as np

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "image-webp_amd", "csrc")
TOOL = os.path.join(ROOT, "tools", "pair_final_check.cpp")


def _build(tmp_path):
    exe = str(tmp_path / "pair_final_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", CSRC, TOOL, "-o", exe])
    return exe


def test_pair_final_masks(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr


def test_trivially_zero_blocks_quantise_to_zero(tmp_path):
    """A block the predicate calls trivially zero has all-zero trellis levels in
    the oracle under every start context (Y1 after Y2: ctype 0, first 1), at two
    quantisers and two lambdas; and the predicate does call a fair share of
    small blocks trivially zero (so the check is not vacuous)."""
    exe = _build(tmp_path)
    for q_dc, q_ac, lam in ((24, 30, 350), (50, 74, 2900), (24, 30, 1)):
        rng = np.random.default_rng(q_ac * 7 + lam)
        n = 4000
        # around the quantiser step: from all-zero blocks to clearly nonzero ones
        scale = rng.choice([0.1, 0.3, 0.5, 0.7, 1.0, 2.0], size=(n, 1)) * q_ac
        co = (rng.standard_normal((n, 16)) * scale / (1 + 0.3 * np.arange(16))).astype(np.int32)
        text = "\n".join(" ".join(str(v) for v in row) for row in co.tolist()) + "\n"
        out = subprocess.run([exe, "trivial", str(q_ac)], input=text, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        triv = np.array([int(v) for v in out.stdout.split()], dtype=bool)
        assert triv.shape == (n,)
        assert 0.05 * n < triv.sum() < 0.95 * n, triv.sum()
        for ctx0 in (0, 1, 2):
            lv, _ = O.quant_blocks(co, ctx0, 0, 1, True, lam, q_dc, q_ac, 0)
            nz = (lv[:, 1:] != 0).any(axis=1)
            bad = np.nonzero(triv & nz)[0]
            assert bad.size == 0, (q_ac, lam, ctx0, co[bad[0]].tolist(), lv[bad[0]].tolist())
