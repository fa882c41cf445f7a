"""Coefficients past +-2047 and the reference's 16-bit inverse transform.

tests/golden/wide_*.vp8 are written by vp8_synth.wide_mbs from the `params`
and arguments kept in tests/golden/decode_wide.json (tools/make_synth_golden.py
--wide).  Their levels are placed by band of m = |level * dequantiser|:

  wrap    2048 <= m <= 32767: nothing saturates, the butterflies' sums wrap
  sat     m > 32767: the full iDCT saturates its input
  dconly  I16 MBs without luma AC tokens under a large Y2 block: the DC-only
          residual (c0 + 4) >> 3 crosses +-32768 and +-65536
  cat6    levels 512..2114: every extra bit of DCT category 6

What the reference does there (zenwebp 0.2.0): coefficients are kept and
dequantised as i32 (decoder/vp8.rs:326, :951); the iWHT (common/transform.rs:
82-114), the DC-only shortcut (transform.rs:13-16, taken at vp8.rs:1110-1117
when the block's token run is empty) and the residue's addition
(common/prediction.rs:138-152) are i32; only the full iDCT
(common/transform_simd_intrinsics.rs:478-632) packs its input to i16 with
saturation and then wraps.  libwebp differs out there, so the oracle alone pins
these streams.

CPU: the three inverse transforms restated in numpy from the Rust against the
oracle's, one-MB frames whose planes are worked out here from the written
levels, the product's host parser and the device token parse's state machine
on every stream, and the cases the fixtures must keep holding.
GPU: every stream through every decode path, alone and in a batch with
libwebp-pinned neighbours, planes and RGBA.  All comparisons are bit-exact.
"""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import vp8_synth as S
import zwebp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLD, "decode_wide.json")) as _f:
    MANIFEST = json.load(_f)["streams"]
BY_NAME = {e["name"]: e for e in MANIFEST}
NAMES = [e["name"] for e in MANIFEST]
MAIN = [n for n in NAMES if (BY_NAME[n]["width"], BY_NAME[n]["height"]) == (80, 48)]
ONE_MB = [n for n in NAMES if (BY_NAME[n]["width"], BY_NAME[n]["height"]) == (16, 16)]
HAND = ["wide_mb_hand0", "wide_mb_hand1", "wide_mb_hand2"]
BANDS = S.WIDE_BANDS
ZIGZAG = [0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15]  # scan position -> raster index (RFC 6386 s13)
Y2_MAX = S.MAX_LEVEL * 440  # the largest product: level 2114, y2ac at index 127
# The six libwebp-pinned streams the wide ones share a batch with: both filters, segments in both modes,
# 1 / 2 / 4 partitions, probability updates, no skip flag
SYNTH_NEIGHBOURS = ["synth_default", "synth_sharp1_simple_p2", "synth_sharp4_simple_p4", "synth_lfd_pos",
                    "synth_qd_base0_allprobs", "synth_skip_absent"]


def _band(name):
    return BY_NAME[name]["gen"]["band"]


def _vp8(name):
    with open(os.path.join(GOLD, name + ".vp8"), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def _mbs(name):
    e = BY_NAME[name]
    return S.wide_mbs(e["params"], **e["gen"])


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The oracle's decode of a fixture: computed once, shared, never written to."""
    rc, r = O.decode(_vp8(name))
    assert rc == 0
    for k in ("y", "u", "v"):
        r[k].setflags(write=False)
    return r


# --------------------------------------------------------------------------
# The reference's inverse transforms, restated from the Rust (not from
# oracle/or_dsp.c) over N blocks at once
# --------------------------------------------------------------------------
def np_iwht(blocks):
    """iwht4x4, common/transform.rs:82-114: i32 throughout."""
    b = np.asarray(blocks, np.int64).reshape(-1, 16)
    r0, r1, r2, r3 = b[:, 0:4], b[:, 4:8], b[:, 8:12], b[:, 12:16]
    a1, b1, c1, d1 = r0 + r3, r1 + r2, r1 - r2, r0 - r3
    t = np.stack([a1 + b1, c1 + d1, a1 - b1, d1 - c1], axis=1)  # (N, row, column)
    a1, b1, c1, d1 = t[:, :, 0] + t[:, :, 3], t[:, :, 1] + t[:, :, 2], t[:, :, 1] - t[:, :, 2], t[:, :, 0] - t[:, :, 3]
    out = np.stack([(a1 + b1 + 3) >> 3, (c1 + d1 + 3) >> 3, (a1 - b1 + 3) >> 3, (d1 - c1 + 3) >> 3], axis=2)
    assert np.abs(t).max(initial=0) < 2 ** 31  # (no i32 overflow within the reachable range)
    return out.reshape(-1, 16)


def np_idct_dc(blocks):
    """idct4x4_dc, common/transform.rs:13-16: (block[0] + 4) >> 3 in i32, everywhere."""
    b = np.asarray(blocks, np.int64).reshape(-1, 16)
    return np.repeat((b[:, :1] + 4) >> 3, 16, axis=1)


# SSE2 on (N, 8) int16 arrays; numpy's int16 array arithmetic wraps as _mm_add_epi16 / _mm_sub_epi16 do
def _lo64(a, b):
    return np.concatenate([a[:, :4], b[:, :4]], axis=1)  # _mm_unpacklo_epi64


def _hi64(a, b):
    return np.concatenate([a[:, 4:], b[:, 4:]], axis=1)  # _mm_unpackhi_epi64


def _lo16(a, b):
    return np.stack([a[:, :4], b[:, :4]], axis=2).reshape(-1, 8)  # _mm_unpacklo_epi16


def _hi16(a, b):
    return np.stack([a[:, 4:], b[:, 4:]], axis=2).reshape(-1, 8)  # _mm_unpackhi_epi16


def _mulhi(a, k):
    return ((a.astype(np.int32) * np.asarray(k, np.int32)) >> 16).astype(np.int16)  # _mm_mulhi_epi16


def _swap64(a):
    return np.concatenate([a[:, 4:], a[:, :4]], axis=1)  # _mm_shuffle_epi32(a, 0b01_00_11_10)


_K1K2 = [20091] * 4 + [-30068] * 4  # _mm_set_epi16 lists its lanes from the highest down
_K2K1 = [-30068] * 4 + [20091] * 4


def _itransform_pass(in01, in23, dc_add, shift):
    """itransform_pass_sse2 (:530-574) and, with the 4 added to the first row and
    the arithmetic >> 3, itransform_pass2_sse2 (:580-625)."""
    in1, in3 = _hi64(in01, in01), _hi64(in23, in23)
    dc = in01 + np.asarray(dc_add, np.int16)
    a_d3, b_c3 = dc + in23, dc - in23
    c1d1, c2d2 = _mulhi(in1, _K2K1), _mulhi(in3, _K1K2)
    c = _hi64(b_c3, b_c3) + (c1d1 - c2d2)
    du = a_d3 + (c1d1 + c2d2)
    d = _hi64(du, du)
    comb_ab, comb_dc = _lo64(a_d3, b_c3), _lo64(d, c)
    tmp01, tmp23 = comb_ab + comb_dc, _swap64(comb_ab - comb_dc)
    if shift:
        tmp01, tmp23 = tmp01 >> 3, tmp23 >> 3  # _mm_srai_epi16
    t0, t1 = _lo16(tmp01, tmp23), _hi16(tmp01, tmp23)
    return _lo16(t0, t1), _hi16(t0, t1)


def np_idct16(blocks):
    """idct4x4_sse2, common/transform_simd_intrinsics.rs:478-524: _mm_packs_epi32
    saturates the i32 input to i16, both passes are wrapping i16."""
    x = np.clip(np.asarray(blocks, np.int64).reshape(-1, 16), -32768, 32767).astype(np.int16)
    with np.errstate(over="ignore"):
        t01, t23 = _itransform_pass(x[:, :8], x[:, 8:], [0] * 8, False)
        o01, o23 = _itransform_pass(t01, t23, [4] * 4 + [0] * 4, True)
    return np.concatenate([o01, o23], axis=1).astype(np.int64)


# --------------------------------------------------------------------------
# From the written levels to coefficient blocks, residuals and classes
# --------------------------------------------------------------------------
def _mb_blocks(params, mb):
    """-> (coef (24, 16) raster order with the luma DCs from the iWHT, nz[24]: the
    block's token run is non-empty, res (24, 16) the residual the reference adds,
    y2 (16,) the dequantised Y2 block or None)."""
    ydc, yac, y2dc, y2ac, uvdc, uvac = S.dequant_factors(params)[mb["segment"]]
    lv = np.asarray(mb["levels"], np.int64)
    i16 = mb["ymode"] != S.B_PRED
    coef = np.zeros((24, 16), np.int64)
    for b in range(24):
        dc, ac = (ydc, yac) if b < 16 else (uvdc, uvac)
        coef[b][ZIGZAG] = lv[b] * np.array([dc] + [ac] * 15)
    nz = np.array([bool(lv[b][(1 if i16 and b < 16 else 0):].any()) for b in range(24)])
    y2 = None
    if i16:
        y2 = np.zeros(16, np.int64)
        y2[ZIGZAG] = lv[24] * np.array([y2dc] + [y2ac] * 15)
        coef[:16, 0] = np_iwht(y2)[0]
    res = np.where(nz[:, None], np_idct16(coef), np_idct_dc(coef))
    return coef, nz, res, y2


@functools.lru_cache(maxsize=None)
def _blocks(name):
    """Per MB of the stream: _mb_blocks."""
    p = BY_NAME[name]["params"]
    return [_mb_blocks(p, mb) for mb in _mbs(name)]


def _d_class(c0):
    """The interval of a DC-only block's d = (c0 + 4) >> 3."""
    d = (int(c0) + 4) >> 3
    if d >= 65536:
        return "d >= 65536"
    if d >= 32768:
        return "32768 <= d <= 65535"
    if d <= -65537:
        return "d <= -65537"
    if d <= -32769:
        return "-65536 <= d <= -32769"
    return "|d| < 32768, |c0| > 32767" if abs(int(c0)) > 32767 else "small"


def _block_kind(nz, c0):
    return "full iDCT" if nz else (f"DC-only, c0 = {int(c0)}, {_d_class(c0)}" if c0 else "no residual")


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_writer_reproduces_wide_fixture(name):
    e = BY_NAME[name]
    assert S.write_keyframe(e["params"], _mbs(name)) == _vp8(name)
    assert len(_vp8(name)) <= 8192
    assert e["pinned_by"] == "oracle" and e["reason"]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_decode_matches_wide_manifest(name):
    e, r = BY_NAME[name], _oracle(name)
    assert S.plane_digests(r["y"], r["u"], r["v"], e["width"], e["height"], r["mbw"] * 16,
                           r["mbw"] * 8) == e["yuv_sha256"]


def _random_blocks(band, n, rng):
    """Coefficient blocks as the band's streams hold them, drawn directly."""
    if band == "wrap":
        b = rng.integers(-32768, 32768, (n, 16))
        b[rng.random((n, 16)) < 0.6] = 0
        b[: n // 4] = np.where(b[: n // 4] == 0, 0, np.sign(b[: n // 4]) * rng.integers(28000, 32768, (n // 4, 16)))
    elif band == "sat":
        b = rng.integers(-Y2_MAX, Y2_MAX + 1, (n, 16))
        b[:, 1:] = np.clip(b[:, 1:], -S.MAX_LEVEL * 284, S.MAX_LEVEL * 284)
        b[rng.random((n, 16)) < 0.5] = 0
        b[: n // 2] = np.where(rng.random((n // 2, 16)) < 0.5, b[: n // 2], b[: n // 2] // 16)
    elif band == "dconly":
        b = np.zeros((n, 16), np.int64)
        b[:, 0] = rng.integers(-2 * Y2_MAX, 2 * Y2_MAX + 1, n)
    else:
        b = rng.integers(512, S.MAX_LEVEL + 1, (n, 16)) * rng.integers(4, 38, (n, 16)) * rng.choice([-1, 1], (n, 16))
        b[rng.random((n, 16)) < 0.7] = 0
    return np.asarray(b, np.int64)


def _edge_blocks():
    vals = [s * v for v in (32767, 32768, Y2_MAX, 32764, 32765, 32766) for s in (1, -1)]
    out = []
    for v in vals:
        out.append(np.full(16, v))
        for k in range(16):
            out.append(np.eye(16, dtype=np.int64)[k] * v)
        for w in vals:  # a pair in the positions the first butterfly adds and subtracts
            for k, m in ((0, 8), (4, 12), (0, 2), (1, 3)):
                blk = np.zeros(16, np.int64)
                blk[k], blk[m] = v, w
                out.append(blk)
    return np.array(out, np.int64)


@pytest.mark.parametrize("band", BANDS)
def test_numpy_transforms_match_oracle(band):
    """np_iwht / np_idct16, restated from the Rust, against the oracle's C
    (or_iwht_c, or_idct_c): the band's own blocks, 20 000 random ones, the edges."""
    rng = np.random.default_rng(0x51DE + BANDS.index(band))
    own = [mb for n in NAMES if _band(n) == band for mb in _blocks(n)]
    full = np.concatenate([np.concatenate([coef for coef, _, _, _ in own]), _random_blocks(band, 20000, rng),
                           _edge_blocks()])
    assert np.array_equal(np_idct16(full), O.blocks("or_idct_c", full).reshape(-1, 16))
    y2 = [y for _, _, _, y in own if y is not None]
    lim = Y2_MAX if band != "cat6" else S.MAX_LEVEL * 37
    wht = np.concatenate([np.array(y2, np.int64).reshape(-1, 16), rng.integers(-lim, lim + 1, (20000, 16)),
                          _edge_blocks()])
    assert np.array_equal(np_iwht(wht), O.blocks("or_iwht_c", wht).reshape(-1, 16))


def _one_mb_planes(params, mb):
    """The planes of a 16 x 16 frame of one MB, luma DC or B_PRED with every
    sub-block B_DC, chroma DC: prediction (128 without neighbours,
    prediction.rs:182-204; B_DC from 127 above and 129 left, :15-72, :326-343)
    plus the residual in i32, clamped (:138-152)."""
    _, _, res, _ = _mb_blocks(params, mb)
    assert mb["uvmode"] == 0 and not mb["skip"]
    res = res.reshape(24, 4, 4)
    if mb["ymode"] == 0:
        y = np.zeros((16, 16), np.int64)
        for b in range(16):
            y[b // 4 * 4:b // 4 * 4 + 4, b % 4 * 4:b % 4 * 4 + 4] = 128 + res[b]
    else:
        assert mb["ymode"] == S.B_PRED and not any(mb["bmodes"])
        ws = np.zeros((17, 17), np.int64)
        ws[0, :], ws[1:, 0] = 127, 129
        for b in range(16):
            y0, x0 = b // 4 * 4 + 1, b % 4 * 4 + 1
            pred = (ws[y0 - 1, x0:x0 + 4].sum() + ws[y0:y0 + 4, x0 - 1].sum() + 4) >> 3
            ws[y0:y0 + 4, x0:x0 + 4] = np.clip(pred + res[b], 0, 255)
        y = ws[1:, 1:]
    c = np.zeros((2, 8, 8), np.int64)
    for b in range(8):
        k = b % 4
        c[b // 4, k // 2 * 4:k // 2 * 4 + 4, k % 2 * 4:k % 2 * 4 + 4] = 128 + res[16 + b]
    return [np.clip(a, 0, 255).astype(np.uint8).reshape(-1) for a in (y, c[0], c[1])]


@pytest.mark.parametrize("name", ONE_MB)
def test_one_mb_planes_from_levels(name):
    """Path selection and residue: the full iDCT where the block's token run is
    non-empty, else the DC-only value in i32, added to a prediction known without
    a decoder -- the oracle's planes."""
    e = BY_NAME[name]
    assert e["params"]["filter_level"] == 0
    r = _oracle(name)
    y, u, v = _one_mb_planes(e["params"], _mbs(name)[0])
    assert np.array_equal(y, r["y"]) and np.array_equal(u, r["u"]) and np.array_equal(v, r["v"])


# Luma of the three hand-built MBs by 4 x 4 block in raster order, worked on the CPU
HAND_LUMA = ([255] * 10 + [0, 0, 255, 255, 0, 0], [0] * 10 + [255, 255, 0, 0, 255, 255],
             [255] * 6 + [0] * 6 + [255] * 4)
HAND_C0 = ([315514] * 4, [-315515] * 4, [548054, 548054, 315514, 315514])  # the iWHT's outputs for blocks 0, 1, 4, 5
HAND_D = ([39439] * 4, [-39439] * 4, [68507, 68507, 39439, 39439])        # (c0 + 4) >> 3: none of them an i16


def test_hand_built_mbs():
    """The three smallest MBs whose DC-only d = (c0 + 4) >> 3 leaves i16: their
    levels are the stated ones, the iWHT gives the stated DCs, and the oracle's
    luma is flat per block with the stated values (an i16 wrap of d would turn
    blocks 0, 1, 4, 5 of the first two into the opposite extreme)."""
    for n, name in enumerate(HAND):
        e = BY_NAME[name]
        (mb,) = _mbs(name)
        assert (e["width"], e["height"]) == (16, 16) and len(_vp8(name)) == (37, 37, 50)[n]
        assert S.dequant_factors(e["params"])[0][2:4] == (314, 440)
        assert (mb["ymode"], mb["uvmode"], mb["skip"]) == (0, 0, 0)
        want = np.zeros((25, 16), np.int64)
        want[24][:len(S.HAND_Y2[n])] = S.HAND_Y2[n]
        assert np.array_equal(mb["levels"], want)
        coef, nz, _, _ = _mb_blocks(e["params"], mb)
        assert not nz.any()
        assert [int(coef[b, 0]) for b in (0, 1, 4, 5)] == HAND_C0[n]
        assert [int((coef[b, 0] + 4) >> 3) for b in (0, 1, 4, 5)] == HAND_D[n]
        y = _oracle(name)["y"].reshape(16, 16)
        blocks = [y[b // 4 * 4:b // 4 * 4 + 4, b % 4 * 4:b % 4 * 4 + 4] for b in range(16)]
        assert all(len(np.unique(blk)) == 1 for blk in blocks)
        assert [int(blk[0, 0]) for blk in blocks] == HAND_LUMA[n]


# ---- the product's own parsers, on the CPU
@pytest.fixture(scope="module")
def product_dump(tmp_path_factory):
    """tools/dec_header_dump.cpp over every wide stream: per stream the MB records of parse_mbs."""
    exe = str(tmp_path_factory.mktemp("wide") / "dec_header_dump")
    csrc = os.path.join(ROOT, "image-webp_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", csrc, os.path.join(ROOT, "tools", "dec_header_dump.cpp"),
                           os.path.join(csrc, "zw_dec_parse.cpp"), "-o", exe])
    out = subprocess.run([exe] + [os.path.join(GOLD, n + ".vp8") for n in NAMES], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    res, lines = {}, iter(out.stdout.splitlines())
    for name in NAMES:
        e = BY_NAME[name]
        nmb = ((e["width"] + 15) // 16) * ((e["height"] + 15) // 16)
        frame, probs = next(lines).split(), next(lines).split()
        assert frame[0] == "frame" and probs[0] == "probs"
        mbs = [next(lines).split() for _ in range(nmb)]
        assert all(m[0] == "mb" for m in mbs)
        res[name] = ([int(v) for v in frame[1:]], [[int(v) for v in m[1:]] for m in mbs])
    return res


@pytest.mark.parametrize("name", NAMES)
def test_product_records_match_written_wide(product_dump, name):
    """parse_mbs (the host token parse): the dequantisers, and every MB's modes,
    segment, skip flag and all 25 x 16 levels, category 6's full range among them."""
    frame, recs = product_dump[name]
    dq = S.dequant_factors(BY_NAME[name]["params"])
    assert frame[26:50] == [v for s in range(4) for v in dq[s]]
    assert len(recs) == len(_mbs(name))
    for k, (r, mb) in enumerate(zip(recs, _mbs(name))):
        assert r[:4] == [mb["ymode"], mb["uvmode"], mb["skip"], mb["segment"]], k
        if mb["ymode"] == S.B_PRED:
            assert r[4:20] == mb["bmodes"], k
        assert r[20:] == [int(v) for v in mb["levels"].reshape(-1)], k


@pytest.mark.parametrize("name", NAMES)
def test_tokl_wide(name):
    """The device token parse's state machine on the host: takes the
    single-partition streams wider than 16 and writes the host parser's records."""
    e = BY_NAME[name]
    taken = e["params"]["log2_nparts"] == 0 and e["width"] > 16
    assert zwebp.dbg_tokl_frame(_vp8(name)) == (0, 1 if taken else -1)


# ---- what the fixtures must keep holding
def _positions(name):
    """(dequantiser name, block kind, scan position, first position, level, quantiser indices'
    dequantisers) of every non-zero level."""
    p = BY_NAME[name]["params"]
    dq = S.dequant_factors(p)
    for mb in _mbs(name):
        i16 = mb["ymode"] != S.B_PRED
        for b in range(25):
            kind = "Y2" if b == 24 else ("U" if 16 <= b < 20 else ("V" if b >= 20 else ("Y I16" if i16 else "Y B_PRED")))
            first = 1 if (b < 16 and i16) else 0
            names = ("ydc", "yac") if b < 16 else (("uvdc", "uvac") if b < 24 else ("y2dc", "y2ac"))
            for n in range(16):
                v = int(mb["levels"][b][n])
                if v:
                    qn = names[0 if n == 0 else 1]
                    q = dict(zip(("ydc", "yac", "y2dc", "y2ac", "uvdc", "uvac"), dq[mb["segment"]]))[qn]
                    yield qn, kind, n, first, v, q


def test_wide_coverage():
    """A regeneration must not quietly lose a case."""
    # -- per-block classes, from the manifest's levels and the numpy restatement
    dclass, sat, wrap_in = {}, 0, []
    for name in NAMES:
        for coef, nz, _, _ in _blocks(name):
            for b in range(24):
                if nz[b]:
                    if (coef[b] > 32767).any() or (coef[b] < -32768).any():
                        sat += 1
                    else:
                        wrap_in.append(coef[b])
                elif b < 16 and coef[b, 0]:
                    k = _d_class(coef[b, 0])
                    dclass[k] = dclass.get(k, 0) + 1
    for k in ("32768 <= d <= 65535", "-65536 <= d <= -32769", "d >= 65536", "d <= -65537", "|d| < 32768, |c0| > 32767"):
        assert dclass.get(k, 0) >= 4, (k, dclass)
    assert sat >= 20
    wrap_in = np.array(wrap_in, np.int64)
    wrapped = (np_idct16(wrap_in) != O.blocks("or_idct_scalar_c", wrap_in).reshape(-1, 16)).any(axis=1)
    assert int(wrapped.sum()) >= 20  # the 16-bit result differs from the 64-bit one though no input saturated
    # -- DCT category 6: every extra bit set and clear, in every kind of block at the first and the last position
    ones = zeros = 0
    places = set()
    for name in NAMES:
        if _band(name) != "cat6":
            continue
        p = BY_NAME[name]["params"]
        assert all(0 <= q <= 20 for q in S.quant_indices(p))
        for _, kind, n, first, v, _ in _positions(name):
            if abs(v) >= 512:
                extra = abs(v) - 67
                ones |= extra
                zeros |= ~extra & 2047
                places.add((kind, "first" if n == first else ("last" if n == 15 else "mid"), v > 0))
    assert ones == 2047 and zeros == 2047, (ones, zeros)
    assert places >= {(k, w, s) for k in ("Y2", "Y I16", "Y B_PRED", "U", "V") for w in ("first", "last")
                      for s in (False, True)}
    # -- level +-2114 with each of the six dequantisers at index 127; the exact i16 edges
    top, products = set(), set()
    for name in NAMES:
        for qn, _, _, _, v, q in _positions(name):
            if abs(v) == S.MAX_LEVEL and q == dict(ydc=157, yac=284, y2dc=314, y2ac=440, uvdc=132, uvac=284)[qn] and \
                    S.dequant_factors(BY_NAME[name]["params"])[0] == (157, 284, 314, 440, 132, 284):
                top.add((qn, v > 0))
            products.add(v * q)
    assert top == {(qn, s) for qn in ("ydc", "yac", "y2dc", "y2ac", "uvdc", "uvac") for s in (False, True)}
    assert products >= {32767, -32767, 32768, -32768}
    # -- wrap never saturates an input; sat does
    for name in NAMES:
        if _band(name) == "wrap":
            assert all(-32768 <= coef.min() and coef.max() <= 32767 for coef, _, _, _ in _blocks(name)), name
            assert all(2048 <= abs(v * q) for _, _, _, _, v, q in _positions(name)), name
    # -- loop filter, partitions, segments, shapes
    for band in BANDS:
        ps = [BY_NAME[n]["params"] for n in MAIN if _band(n) == band]
        assert any(p["filter_level"] == 0 for p in ps), band
        assert any(p["filter_type"] == 0 and p["filter_level"] >= 30 for p in ps), band
        assert any(p["filter_type"] == 1 and p["filter_level"] > 0 for p in ps), band
    assert any(BY_NAME[n]["params"]["log2_nparts"] == 2 for n in NAMES)
    assert any(BY_NAME[n]["params"]["segments"] and len({q for q in S.quant_indices(BY_NAME[n]["params"])}) == 4 and
               {mb["segment"] for mb in _mbs(n)} == {0, 1, 2, 3} for n in NAMES)
    sizes = {(e["width"], e["height"]) for e in MANIFEST}
    assert sizes == {(80, 48), (37, 21), (32, 16), (16, 16)}
    assert len(ONE_MB) >= 48 and {_band(n) for n in ONE_MB} == set(BANDS) and set(HAND) <= set(ONE_MB)
    assert {BY_NAME[n]["gen"]["force"]["ymode"] for n in ONE_MB if "force" in BY_NAME[n]["gen"]} == {0, S.B_PRED}
    # the hand-built MBs verbatim inside multi-MB frames, one of them through the device token parse
    assert sorted(n for _, n in BY_NAME["wide_dconly_lf0"]["gen"]["hand"]) == [0, 1, 2]
    assert BY_NAME["wide_hand_32x16"]["params"]["log2_nparts"] == 0
    # every mode on every kind of MB position, skipped and empty MBs
    seen = set()
    for name in MAIN:
        for k, mb in enumerate(_mbs(name)):
            mbx, mby = k % 5, k // 5
            where = "inside" if (mbx, mby) == (2, 1) else ("edge")
            seen |= {(where, "y", mb["ymode"]), (where, "uv", mb["uvmode"])}
            seen.add("skip" if mb["skip"] else ("empty" if not mb["levels"].any() else "coded"))
    assert seen >= {(w, "y", m) for w in ("inside", "edge") for m in range(5)} | \
        {(w, "uv", m) for w in ("inside", "edge") for m in range(4)} | {"skip", "empty", "coded"}


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    return zwebp.Context(0)


def _first_diff(name, y, u, v):
    """'' when the planes (MB-aligned, as the oracle's) are the oracle's, else the
    first differing MB and block and the path the block's residual took."""
    r = _oracle(name)
    mbw = r["mbw"]
    for plane, got, want, size, base in (("Y", y, r["y"], 16, 0), ("U", u, r["u"], 8, 16), ("V", v, r["v"], 8, 20)):
        got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
        if got.shape != want.shape:
            return f"{name}: plane {plane} has {got.size} bytes, the oracle's {want.size}"
        bad = np.flatnonzero(got != want)
        if bad.size:
            row, col = divmod(int(bad[0]), mbw * size)
            mbx, mby = col // size, row // size
            b = base + (row % size) // 4 * (size // 4) + (col % size) // 4
            coef, nz, _, _ = _blocks(name)[mby * mbw + mbx]
            mb = _mbs(name)[mby * mbw + mbx]
            return (f"{name}: plane {plane} differs first at ({col}, {row}): MB ({mbx}, {mby}) ymode {mb['ymode']} "
                    f"skip {mb['skip']}, block {b} ({_block_kind(nz[b], coef[b, 0])}): got {int(got[bad[0]])}, "
                    f"oracle {int(want[bad[0]])}; {bad.size} bytes differ")
    return ""


@pytest.mark.gpu
@pytest.mark.parametrize("tokens", ["host", "device"])
@pytest.mark.parametrize("rows", ["default", "0"])
@pytest.mark.parametrize("name", NAMES)
def test_gpu_decode_wide(ctx, monkeypatch, name, rows, tokens):
    """vp8_decode_frame, tokens parsed on the host and on the device, through the
    row-parallel and the workgroup-per-frame kernels: the oracle's planes and the
    manifest's digests."""
    if rows != "default":
        monkeypatch.setenv("ZW_DEC_ROWS", rows)
    monkeypatch.setenv("ZW_DEC_TOKENS", tokens)
    e = BY_NAME[name]
    fr = zwebp.vp8_decode_frame(_vp8(name), ctx=ctx)
    assert (fr.width, fr.height) == (e["width"], e["height"])
    msg = _first_diff(name, fr.ybuf, fr.ubuf, fr.vbuf)
    assert not msg, msg
    assert S.plane_digests(fr.ybuf, fr.ubuf, fr.vbuf, e["width"], e["height"], fr.y_stride,
                           fr.uv_stride) == e["yuv_sha256"]


@functools.lru_cache(maxsize=None)
def _synth_oracle(name):
    with open(os.path.join(GOLD, name + ".vp8"), "rb") as f:
        vp8 = f.read()
    rc, r = O.decode(vp8)
    assert rc == 0 and (r["hdr"].width, r["hdr"].height) == (80, 48)
    for k in ("y", "u", "v"):
        r[k].setflags(write=False)
    return vp8, r


def _batch():
    """The 80 x 48 wide streams, two by two between six libwebp-pinned synth
    streams: [(name, stream, oracle result or None for a wide one)]."""
    out = []
    for k, name in enumerate(MAIN):
        out.append((name, _vp8(name), None))
        if k % 2 == 1:
            n = SYNTH_NEIGHBOURS[(k // 2) % len(SYNTH_NEIGHBOURS)]
            out.append((n,) + _synth_oracle(n))
    assert len(MAIN) >= 12 and {n for n, _, r in out if r is not None} == set(SYNTH_NEIGHBOURS)
    return out


def _batch_env(monkeypatch, tokens, rows):  # (as test_synth_streams._batch_env)
    monkeypatch.setenv("ZW_DEC_TOKENS", tokens)
    monkeypatch.setenv("ZW_DEC_ROWS", rows)
    if tokens == "mixed":
        monkeypatch.setenv("ZW_DEC_CHUNK", "4")
        monkeypatch.setenv("ZW_DEC_TOKENS_HOST", "0.4")


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ["0", "1"])
@pytest.mark.parametrize("tokens", ["device", "mixed"])
def test_gpu_batch_wide(ctx, monkeypatch, tokens, rows):
    """The wide 80 x 48 streams between ordinary ones as one decode_batch: every
    frame the oracle's."""
    _batch_env(monkeypatch, tokens, rows)
    batch = _batch()
    frames = zwebp.decode_batch([s for _, s, _ in batch], ctx=ctx)
    assert len(frames) == len(batch)
    bad = []
    for k, ((name, _, r), fr) in enumerate(zip(batch, frames)):
        if r is None:
            msg = _first_diff(name, fr.ybuf, fr.ubuf, fr.vbuf)
        else:
            same = np.array_equal(fr.ybuf, r["y"]) and np.array_equal(fr.ubuf, r["u"]) and np.array_equal(fr.vbuf, r["v"])
            msg = "" if same else f"{name}: differs from the oracle"
        if msg:
            bad.append(f"frame {k}: {msg}")
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ["0", "1"])
@pytest.mark.parametrize("tokens", ["device", "mixed"])
def test_gpu_rgb_batch_wide(ctx, monkeypatch, tokens, rows):
    """The same batch through decode_rgb_batch (RGBA, fancy upsampling) against
    the oracle's planes through its fill_rgb_buffer_fancy."""
    _batch_env(monkeypatch, tokens, rows)
    batch = _batch()
    imgs = zwebp.decode_rgb_batch([s for _, s, _ in batch], 4, zwebp.UpsamplingMethod.Bilinear, ctx=ctx)
    assert len(imgs) == len(batch)
    bad = []
    for k, ((name, _, r), im) in enumerate(zip(batch, imgs)):
        r = r or _oracle(name)
        want = O.yuv_to_rgb_fancy(r["y"], r["u"], r["v"], 80, 48, 4)
        got = np.frombuffer(bytes(im), np.uint8)
        if got.size != want.size or (got != want).any():
            px = int(np.flatnonzero(got != want)[0]) // 4 if got.size == want.size else -1
            where = ""
            if px >= 0 and name in BY_NAME:
                x, y = px % 80, px // 80
                b = (y % 16) // 4 * 4 + (x % 16) // 4
                coef, nz, _, _ = _blocks(name)[(y // 16) * 5 + x // 16]
                where = f" first at ({x}, {y}): MB ({x // 16}, {y // 16}) luma block {b} ({_block_kind(nz[b], coef[b, 0])})"
            bad.append(f"frame {k} {name}:{where}")
    assert not bad, "\n".join(bad)
