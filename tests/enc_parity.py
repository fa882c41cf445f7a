"""Stage-by-stage comparison of the device encoder with the oracle (helper
module, not a test): source planes, analysis alphas, pass-1 modes and
reconstruction, probabilities, skip probability, pass-2 modes, levels,
reconstruction and bitstream, so a failure names the first stage and macroblock
that diverged.  Shared by test_gpu_parity.py and test_enc_extreme.py."""
import numpy as np

import oracle_lib as O
import zwebp
from zwebp.synth import synth_rgba

ENC_CASES = [
    (64, 48, "natural", 75, 4, 3),
    (300, 257, "natural", 75, 4, 3),
    (768, 512, "natural", 75, 4, 3),
    (333, 211, "noise", 75, 4, 2),
    (256, 256, "flat", 75, 4, 3),
    (200, 120, "natural", 20, 4, 3),
    (96, 80, "natural", 95, 4, 3),
    (160, 128, "natural", 75, 0, 3),
    (160, 128, "natural", 75, 2, 3),
    (160, 128, "natural", 75, 3, 3),
    (160, 128, "natural", 75, 5, 3),
    (160, 128, "natural", 75, 6, 3),
    (123, 77, "natural", 0, 4, 0),
    (123, 77, "natural", 100, 4, 1),
    (1, 1, "natural", 75, 4, 3),
    (4000, 16, "natural", 75, 4, 3),
    (16, 1100, "natural", 60, 4, 3),
]


def enc_case_seed(w, h):
    return 0x5EED0000 + w * 7 + h


def _img(w, h, kind, seed, color):
    rgba = synth_rgba(w, h, seed, kind)
    if color == zwebp.ColorType.Rgba8:
        return rgba
    if color == zwebp.ColorType.Rgb8:
        return np.ascontiguousarray(rgba[..., :3])
    if color == zwebp.ColorType.La8:
        return np.ascontiguousarray(rgba[..., [0, 3]])
    return np.ascontiguousarray(rgba[..., 0])


def _mb_rows(a, per):
    return a.reshape(-1, per)


def _plane_mb_diff(a, b, stride, mb):
    """MB indices whose (mb x mb) tile differs."""
    A = a.reshape(-1, stride)
    B = b.reshape(-1, stride)
    d = (A != B).reshape(A.shape[0] // mb, mb, stride // mb, mb).any(axis=(1, 3))
    return np.nonzero(d.reshape(-1))[0]


def _modes_of(info, nmb):
    m = np.array([[info[i].luma_mode, info[i].chroma_mode, info[i].skip, info[i].segment] + list(info[i].bpred)
                  for i in range(nmb)], np.uint8)
    m[m[:, 0] != 4, 4:] = 0
    return m


def _check_encode(ctx, w, h, kind, q, m, color, seed):
    """Stage-by-stage comparison; collects every stage's first divergence."""
    return _check_encode_img(ctx, _img(w, h, kind, seed, color), w, h, q, m, color)


def _check_encode_img(ctx, img, w, h, q, m, color, oracle=None):
    """_check_encode on a given frame; oracle: an (rc, stream, debug) of O.encode(..., debug=True)
    computed before (read only), else it is computed here."""
    rc, ref, dbg = oracle if oracle is not None else O.encode(img, w, h, color, q, m, debug=True)
    assert rc == 0
    p = zwebp.Pipeline(1, w, h, color, q, m, ctx=ctx)
    rep = []
    try:
        p.upload(0, img)
        nmb = p.mbw * p.mbh
        ys, cs = p.mbw * 16, p.mbw * 8
        # pass 1 alone (with its reconstruction)
        p.run_pass1(True)
        y, u, v = p.planes(0, 0)
        for a, b, n in ((y, dbg["src_y"], "Y"), (u, dbg["src_u"], "U"), (v, dbg["src_v"], "V")):
            if not np.array_equal(a, b):
                rep.append(f"source plane {n} differs")
        if dbg["segments_enabled"]:
            al = p.alpha(0)
            d = np.nonzero(al != dbg["mb_alpha"])[0]
            if d.size:
                rep.append(f"alpha: {d.size} MBs differ, first {d[0]}: {al[d[0]]} vs {dbg['mb_alpha'][d[0]]}")
        m1, _ = p.mbinfo(0, 1)
        g1 = m1.copy()
        g1[g1[:, 0] != 4, 4:] = 0
        o1 = _modes_of(dbg["p1_info"], nmb)
        d = np.nonzero((g1[:, [0, 1]] != o1[:, [0, 1]]).any(axis=1) | (g1[:, 4:] != o1[:, 4:]).any(axis=1))[0]
        if d.size:
            i = int(d[0])
            rep.append(f"pass-1 modes: {d.size} MBs differ, first MB {i} (x={i % p.mbw},y={i // p.mbw}): "
                       f"{g1[i].tolist()} vs {o1[i].tolist()}")
        r1y, _, _ = p.planes(0, 1)
        d = _plane_mb_diff(r1y, dbg["recon1_y"], ys, 16)
        if d.size:
            rep.append(f"pass-1 recon Y: {d.size} MBs differ, first MB {d[0]}")
        # full encode
        p.enable_debug()
        p.encode()
        gp, gsp = p.probs(0)
        if not np.array_equal(gp, dbg["final_probs"]):
            rep.append(f"pass-2 probabilities differ in {int((gp != dbg['final_probs']).sum())} entries")
        if gsp != dbg["skip_prob"]:
            rep.append(f"skip prob {gsp} vs {dbg['skip_prob']}")
        modes, levels = p.mbinfo(0, 2)
        gm = modes.copy()
        gm[gm[:, 0] != 4, 4:] = 0
        om = _modes_of(dbg["p2_info"], nmb)
        d = np.nonzero((gm != om).any(axis=1))[0]
        if d.size:
            i = int(d[0])
            rep.append(f"pass-2 modes: {d.size} MBs differ, first MB {i} (x={i % p.mbw},y={i // p.mbw}): "
                       f"{gm[i].tolist()} vs {om[i].tolist()}")
        ol = dbg["levels"].reshape(nmb, 25, 16)
        gl = levels.astype(np.int32)
        gl[gm[:, 2] == 1] = 0
        gl[gm[:, 0] == 4, 16] = 0
        d = np.nonzero((gl != ol).reshape(nmb, -1).any(axis=1))[0]
        if d.size:
            i = int(d[0])
            blk = int(np.nonzero((gl[i] != ol[i]).any(axis=1))[0][0])
            rep.append(f"levels: {d.size} MBs differ, first MB {i} block {blk} (mode {gm[i, 0]}): "
                       f"{gl[i, blk].tolist()} vs {ol[i, blk].tolist()}")
            if gm[i, 0] == 4:
                gd = p.i4_dump(0)[i, blk]
                od = dbg["i4_dump"].reshape(nmb, 16, 34)[i, blk]
                rep.append(f"  I4 dump gpu coeffs {gd[:16].tolist()} pred {gd[16:32].tolist()} ctx0 {gd[32]} mode {gd[33]}")
                rep.append(f"  I4 dump orc coeffs {od[:16].tolist()} pred {od[16:32].tolist()} ctx0 {od[32]} mode {od[33]}")
        ry, ru, rv = p.planes(0, 1)
        for a, b, s, mb, n in ((ry, dbg["recon_y"], ys, 16, "Y"), (ru, dbg["recon_u"], cs, 8, "U"),
                               (rv, dbg["recon_v"], cs, 8, "V")):
            d = _plane_mb_diff(a, b, s, mb)
            if d.size:
                A, B = a.reshape(-1, s), b.reshape(-1, s)
                r0, c0 = (d[0] // (s // mb)) * mb, (d[0] % (s // mb)) * mb
                ta, tb = A[r0:r0 + mb, c0:c0 + mb], B[r0:r0 + mb, c0:c0 + mb]
                pos = np.argwhere(ta != tb)
                rep.append(f"recon {n}: {d.size} MBs differ, first MB {d[0]}, {len(pos)} px, first at {pos[0].tolist()}"
                           f" gpu {int(ta[tuple(pos[0])])} oracle {int(tb[tuple(pos[0])])}")
        out = p.output(0)
        if out != ref:
            rep.append(f"bitstream differs (len {len(out)} vs {len(ref)})")
    finally:
        p.close()
    assert not rep, "\n".join(rep)
    return ref
