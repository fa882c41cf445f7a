"""The encoder on extreme-contrast frames, at both ends of the quantiser.

Every encoder test compares the device with the oracle bit for bit, but only
over the arithmetic its inputs reach, and the synthetic and gallery inputs stay
well inside it: no I4 rate past the reference's `rate as u16` (vp8.rs:1979,
:2005; the product restates the wrap in rdscore() and in three
`(rate & 0xffffu) * l_i4` forms), no level past 242, hardly any TM / V
macroblock, no saturated frame against the 127 / 129 borders.  The frames of
enc_extreme.py reach all of these.

CPU part: a census from the oracle's debug output asserts that each fixture
reaches what it is for (floors at or below the values measured when the
fixtures were final, listed in DESIGN.md), that the existing inputs do not wrap
the I4 rate, and that every oracle stream of the set decodes (oracle and, where
it is installed, the system libwebp, to the same planes).

GPU part, all bit-exact: the stage-by-stage comparison of enc_parity.py with
the row kernels and the workgroup-per-frame kernels, the frame-pair kernels in
fresh child processes, token partitions and the host emitter's other group
shapes, device statistics against the host replay, and the product's decoder on
the product's Q100 streams.
"""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import enc_extreme as X
import oracle_lib as O
import vp8_synth as S
from enc_parity import ENC_CASES, _check_encode_img, _img, enc_case_seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

# sub-block modes (the oracle's bpred numbering), MB luma and chroma modes
B_DC, B_TM, B_VE, B_HE, B_LD, B_RD, B_VR, B_VL, B_HD, B_HU = range(10)


def _census(name, q, m):
    """What one oracle encode reached; pass-2 figures unless named otherwise."""
    w, h = X.dims(name)
    _, d = X.oracle(name, q, m)
    nmb = ((w + 15) // 16) * ((h + 15) // 16)
    md = X.modes(d, nmb)
    lv = np.abs(d["levels"].reshape(nmb, 25, 16))
    return dict(nmb=nmb, rate_max=max(d["i4_rate_max"]), wrap_trials=d["i4_wrap_trials"][1],
                wrap_winners=d["i4_wrap_winners"][1], exit_score=sum(d["i4_exit_score"]), exit_hdr=sum(d["i4_exit_hdr"]),
                y=int(lv[:, :16].max()), y2=int(lv[:, 16].max()), uv=int(lv[:, 17:].max()),
                skipped=sum(d["p2_info"][i].skip for i in range(nmb)),
                luma=np.bincount(md[:, 0], minlength=5), chroma=np.bincount(md[:, 1], minlength=4),
                sub=np.bincount(md[md[:, 0] == 4, 2:].reshape(-1), minlength=10))


# ---------------------------------------------------------------------------
# CPU: the census -- conditions, not measurements (the measured values are in
# DESIGN.md, "Extreme-contrast encoder inputs")
# ---------------------------------------------------------------------------
def test_fixtures_are_what_the_table_says():
    assert len(X.NAMES) == 14 and all(X.dims(n) == (48, 48) for n in X.NAMES if n != "quilt")
    assert X.dims("quilt") == (150, 100)
    c = X.frame("checker1")
    assert c[0, 0, 0] == 0 and c[0, 1, 0] == 255 and c[1, 0, 1] == 255 and c[1, 1, 2] == 0
    b = X.frame("binnoise")
    assert set(np.unique(b)) == {0, 255} and 0.4 < (b == 255).mean() < 0.6
    for n in X.NAMES:  # every fixture keeps the two ends and the middle of the quantiser
        assert {100, 75, 0} <= {q for q, _ in X.SETTINGS[n]}, n
        assert set(X.SETTINGS[n]) <= set(X.ALL_SETTINGS)
    q = X.frame("quilt")  # unlike contents are neighbours
    assert (q[:32, 0:32] == 0).all() and (q[:32, 32:64] == 255).all() and np.array_equal(q[:32, 64:96], c[:32, :32])


@pytest.mark.parametrize("q,m,floor", [(100, 4, 100), (100, 6, 100), (98, 5, 100)])
def test_census_checker1_wrapped_rate_wins(q, m, floor):
    """The u16 wrap decides the modes: most of the 144 sub-blocks are chosen at a rate past 65 535."""
    c = _census("checker1", q, m)
    assert c["wrap_winners"] >= floor and c["rate_max"] > 65535, c
    assert c["wrap_trials"] >= c["wrap_winners"]


@pytest.mark.parametrize("name", ["vstripe1", "hstripe1"])
def test_census_stripes_wrap_wins_and_loses(name):
    c6, c4 = _census(name, 100, 6), _census(name, 100, 4)
    assert c6["wrap_winners"] >= 1, c6
    assert c4["wrap_trials"] >= 1 and c4["wrap_winners"] == 0, c4  # the wrapped candidate loses


def test_census_level_magnitudes():
    for m in (4, 6):
        assert _census("checker16", 100, m)["y2"] >= 1024
        assert _census("sat8", 100, m)["uv"] >= 256
        for name in ("black", "white"):
            c = _census(name, 100, m)
            assert c["y2"] >= 512 and c["skipped"] >= 6 and c["nmb"] == 9, (name, c)
    assert _census("diag45", 100, 6)["y"] >= 256


def test_census_macroblock_modes():
    c = _census("sat2", 100, 4)
    assert (c["chroma"] > 0).all(), c["chroma"]
    c = _census("uvtm", 75, 4)
    assert (c["luma"] > 0).all() and (c["chroma"] > 0).all(), (c["luma"], c["chroma"])


def test_census_sub_block_modes():
    total = np.zeros(10, np.int64)
    for name, q, m in X.CASES:
        c = _census(name, q, m)
        total += c["sub"]
        if name == "diag45":
            assert c["sub"][B_LD] >= 100, (q, m, c["sub"])
        if name == "diag135":
            assert c["sub"][B_RD] >= 100, (q, m, c["sub"])
        if name == "tm":  # at Q0 most MBs go to I16: most of what stays I4, and never below 30
            assert c["sub"][B_TM] >= 30 and c["sub"][B_TM] == c["sub"].max(), (q, m, c["sub"])
    assert (total > 0).all(), total


def test_census_quilt_takes_both_early_exits():
    for q, m in ((75, 4), (0, 4)):
        c = _census("quilt", q, m)
        assert c["exit_score"] >= 1 and c["exit_hdr"] >= 1, c
    assert sum(_census("quilt", q, m)["exit_hdr"] for q, m in X.SETTINGS["quilt"]) >= 4


@pytest.mark.parametrize("name", ["binnoise", "diag45", "diag135", "quilt"])
def test_census_q0_block_sse(name):
    """At Q0 a 4 x 4 block's squared error passes 40 000: the 32-bit I4 score
    sse * 256 + rate * lambda then goes past 10 M (35.6 M among the trials), which the
    kernels key as (score << 2) | k and so need below 2^30.  Recomputed here from the
    source and the reconstruction, not taken from the encoder's own sums."""
    w, h = X.dims(name)
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    for q, m in ((0, 4), (0, 6)):
        _, d = X.oracle(name, q, m)
        e = (d["src_y"].astype(np.int64) - d["recon_y"].astype(np.int64)) ** 2
        sse = e.reshape(mbh * 4, 4, mbw * 4, 4).sum(axis=(1, 3))
        assert sse.max() >= 40000, (q, m, int(sse.max()))


def _gallery_rgb(path):
    b = open(path, "rb").read()
    rc, hd = O.decode_header(b)
    rc2, r = O.decode(b)
    assert rc == 0 and rc2 == 0
    return O.yuv_to_rgb_fancy(r["y"], r["u"], r["v"], hd.width, hd.height, 3), hd.width, hd.height


def test_census_existing_inputs_never_wrap():
    """New ground: over the stage-by-stage cases and the gallery pictures no I4 rate
    reaches 65 536 (largest measured: 41 174, printed below).  Should a later input
    make this false, turn it into a comment."""
    top = 0
    for w, h, kind, q, m, color in ENC_CASES:
        rc, _, d = O.encode(_img(w, h, kind, enc_case_seed(w, h), color), w, h, color, q, m, debug=True)
        assert rc == 0
        top = max(top, *d["i4_rate_max"])
        assert sum(d["i4_wrap_trials"]) == 0, (w, h, kind, q, m)
    files = sorted(glob.glob(os.path.join(GOLD, "gallery*.vp8")))
    assert files
    for f in files:
        rgb, w, h = _gallery_rgb(f)
        rc, _, d = O.encode(rgb, w, h, 2, 75, 4, debug=True)
        assert rc == 0
        top = max(top, *d["i4_rate_max"])
        assert sum(d["i4_wrap_trials"]) == 0, f
    print("largest I4 rate over the existing inputs:", top)
    assert 0 < top < 65536


def test_debug_capture_leaves_the_stream_alone():
    """The counters go only into the census struct of a debug encode, cleared per call;
    the debug struct itself keeps the layout every binding checks."""
    import ctypes
    assert O.lib().or_debug_struct_size() == ctypes.sizeof(O.EncDebug)
    assert O.lib().or_census_struct_size() == ctypes.sizeof(O.I4Census) == 40
    for name, q, m in (("checker1", 100, 6), ("quilt", 0, 4)):
        w, h = X.dims(name)
        ref, d = X.oracle(name, q, m)
        rc, plain, _ = O.encode(X.frame(name), w, h, X.RGB8, q, m)
        assert rc == 0 and plain == ref
        rc, again, d2 = O.encode(X.frame(name), w, h, X.RGB8, q, m, debug=True)
        assert again == ref and all(d2[k] == d[k] for k in O.I4_CENSUS)


# ---------------------------------------------------------------------------
# CPU: stream validity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", X.NAMES)
def test_oracle_streams_decode(name):
    """The oracle's decoder reads every stream of the set back to the encoder's own
    reconstruction (before the loop filter).  Chroma only up to quantiser index 117:
    past it the reference's encoder keeps the chroma DC step of its table (up to 157,
    vp8.rs:2341, :2464) where every decoder caps it at 132 (decoder/vp8.rs:498), so at
    Q0 (index 127) its chroma reconstruction is not what a decoder shows.  The grey
    fixtures do not see this; the coloured ones must."""
    coloured = 0
    for q, m in X.SETTINGS[name]:
        vp8, d = X.oracle(name, q, m)
        rc, r = O.decode(vp8, want_unfiltered=True)
        assert rc == 0, (q, m)
        w, h = X.dims(name)
        assert (r["hdr"].width, r["hdr"].height) == (w, h)
        assert np.array_equal(r["uy"], d["recon_y"]), (q, m)
        same = np.array_equal(r["uu"], d["recon_u"]) and np.array_equal(r["uv"], d["recon_v"])
        if d["base_quant_index"] <= 117:
            assert same, (q, m)
        else:
            coloured += not same
    assert coloured == (len([1 for q, _ in X.SETTINGS[name] if q == 0]) if name in ("sat8", "sat2", "uvtm", "quilt") else 0)


@pytest.mark.skipif(S.libwebp() is None, reason="system libwebp absent")
@pytest.mark.parametrize("name", X.NAMES)
def test_libwebp_decodes_to_the_same_planes(name):
    w, h = X.dims(name)
    mbw = (w + 15) // 16
    for q, m in X.SETTINGS[name]:
        vp8, _ = X.oracle(name, q, m)
        rc, r = O.decode(vp8)
        assert rc == 0
        got = S.libwebp_yuv_digests(vp8)
        assert got is not None, "libwebp rejects the stream"
        assert got == S.plane_digests(r["y"], r["u"], r["v"], w, h, mbw * 16, mbw * 8), (q, m)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import zwebp
    return zwebp.Context(0)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ["1", "0"])
@pytest.mark.parametrize("name,q,m", X.CASES, ids=[f"{n}-q{q}-m{m}" for n, q, m in X.CASES])
def test_gpu_stage_by_stage(ctx, monkeypatch, name, q, m, rows):
    """rows "1": the row kernels, "0": one workgroup per frame."""
    monkeypatch.setenv("ZW_ENC_ROWS", rows)
    w, h = X.dims(name)
    vp8, dbg = X.oracle(name, q, m)
    _check_encode_img(ctx, X.frame(name), w, h, q, m, X.RGB8, oracle=(0, vp8, dbg))


_PAIR_CHILD = r"""
import json, os, sys
sys.path[:0] = [os.path.join(sys.argv[1], "image-webp_amd"), os.path.join(sys.argv[1], "tests")]
import numpy as np
import enc_extreme as X
import oracle_lib as O
import zwebp
from zwebp.shard import frame_seed
from zwebp.synth import synth_rgba
c = json.loads(sys.argv[2])
w = h = X.SIZE
mbw = mbh = (w + 15) // 16
L = zwebp.load_library()
ctx = zwebp.Context(0)
for names in c["batches"]:
    n = len(names)
    imgs = [np.ascontiguousarray(synth_rgba(w, h, frame_seed(i), "natural")[..., :3]) if k == "natural" else X.frame(k)
            for i, k in enumerate(names)]
    assert L.zwk_encode_fp(1, mbw, n) == 1, "pass 1 does not run in frame pairs"
    assert L.zwk_encode_fp(2, mbw, n) == 1, "pass 2 does not run in frame pairs"
    for q, m in c["settings"]:
        what = "%s q%d m%d" % ("+".join(names), q, m)
        refs, dbgs = [], []
        for im in imgs:
            rc, ref, dbg = O.encode(im, w, h, X.RGB8, q, m, debug=True)
            assert rc == 0
            refs.append(ref)
            dbgs.append(dbg)
        out = zwebp.encode_batch(imgs, w, h, X.RGB8, q, m, ctx=ctx)
        p = zwebp.Pipeline(n, w, h, X.RGB8, q, m, ctx=ctx)
        for i in range(n):
            p.upload(i, imgs[i])
        p.encode()
        for i in range(n):
            for a, name, mb in zip(p.planes(i, 1), ("recon_y", "recon_u", "recon_v"), (16, 8, 8)):
                A, B = a.reshape(mbh * mb, mbw * mb), dbgs[i][name].reshape(mbh * mb, mbw * mb)
                d = np.argwhere((A != B).reshape(mbh, mb, mbw, mb).any(axis=(1, 3)))
                assert d.size == 0, "%s frame %d %s: %d MBs differ, first (y, x) %s" % (what, i, name, len(d), d[0].tolist())
            assert p.output(i) == refs[i], "%s: pipeline stream %d" % (what, i)
        p.close()
        bad = [i for i in range(n) if out[i] != refs[i]]
        assert not bad, (what, bad)
ctx.close()
print("ok")
"""

PAIR_BATCHES = [("checker1", "checker1"), ("checker1", "natural"), ("black", "binnoise"),
                ("vstripe1", "hstripe1", "checker16"), ("sat8", "uvtm")]


@pytest.mark.gpu
@pytest.mark.parametrize("names", PAIR_BATCHES, ids=["+".join(b) for b in PAIR_BATCHES])
def test_gpu_frame_pairs(names):
    """Both passes in frame pairs (a fresh process: ZW_ENC_FP is read once), the
    three-frame batch for the odd last workgroup: streams and reconstructed planes
    against the oracle at Q100 m4 and m6 and Q0 m4."""
    env = dict(os.environ, ZW_ENC_FP="1", ZW_ENC_ROWS="0")
    case = dict(batches=[list(names)], settings=[(100, 4), (100, 6), (0, 4)])
    r = subprocess.run([sys.executable, "-c", _PAIR_CHILD, ROOT, json.dumps(case)], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.gpu
@pytest.mark.parametrize("nparts", [2, 8])
def test_gpu_token_partitions(ctx, nparts):
    import zwebp
    names = ("checker1", "diag45")
    w = h = X.SIZE
    for q, m in ((100, 4), (100, 6)):
        refs = [X.oracle(n, q, m, nparts)[0] for n in names]
        for n, ref in zip(names, refs):
            out = zwebp.encode_frame_lossy(X.frame(n), w, h, X.RGB8, q, m, ctx=ctx, token_partitions=nparts)
            assert out == ref, (n, q, m, nparts)
        outs = zwebp.encode_batch([X.frame(n) for n in names], w, h, X.RGB8, q, m, ctx=ctx, token_partitions=nparts)
        assert [bytes(o) for o in outs] == refs, (q, m, nparts)


_EMIT_CHILD = r"""
import os, sys
sys.path[:0] = [os.path.join(sys.argv[1], "image-webp_amd"), os.path.join(sys.argv[1], "tests")]
import enc_extreme as X
import zwebp
names = ("checker16", "white", "checker16", "sat8", "checker1")
n, w, h = 18, X.SIZE, X.SIZE
refs = [X.oracle(k, 100, 4)[0] for k in names]
ctx = zwebp.Context(0)
p = zwebp.Pipeline(n, w, h, X.RGB8, 100, 4, ctx=ctx)
for i in range(n):
    p.upload(i, X.frame(names[i % len(names)]))
p.encode_repeat(2)
bad = [i for i in range(n) if p.output(i) != refs[i % len(names)]]
assert not bad, (len(bad), bad[:4])
p.close()
ctx.close()
print("ok")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"ZW_EMIT_GROUP": "7"}, {"ZW_CODE16": "0"}], ids=["vector_7_lanes", "four_interleaved"])
def test_gpu_emission_groups(env):
    """The host emitter's other shapes on cat6 levels (checker16's Y2 of 1 752 among
    them): 18 frames in groups of 7 (and a last group of 4), and with the vector
    coder off.  A fresh process per case (the knobs are read once)."""
    r = subprocess.run([sys.executable, "-c", _EMIT_CHILD, ROOT], env=dict(os.environ, **env), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.gpu
@pytest.mark.parametrize("names", [("checker1", "checker16"), ("sat8", "black")], ids="+".join)
def test_gpu_device_stats_equal_host_replay(ctx, monkeypatch, names):
    import zwebp
    w = h = X.SIZE
    imgs = [X.frame(n) for n in names]
    for q, m in ((100, 4), (100, 6)):
        dev = zwebp.encode_batch(imgs, w, h, X.RGB8, q, m, ctx=ctx)
        with monkeypatch.context() as mp:
            mp.setenv("ZW_HOST_STATS", "1")
            host = zwebp.encode_batch(imgs, w, h, X.RGB8, q, m, ctx=ctx)
        for i, n in enumerate(names):
            assert dev[i] == host[i], (n, q, m)
            assert dev[i] == X.oracle(n, q, m)[0], (n, q, m)


@pytest.fixture(scope="module")
def product_q100(ctx):
    """The product's own Q100 streams, encoded once."""
    import zwebp
    return {(n, m): zwebp.encode_frame_lossy(X.frame(n), *X.dims(n), X.RGB8, 100, m, ctx=ctx)
            for n in X.NAMES for m in (4, 6)}


@pytest.mark.gpu
@pytest.mark.parametrize("tokens", ["host", "device"])
@pytest.mark.parametrize("rows", ["default", "0"])
@pytest.mark.parametrize("name", X.NAMES)
def test_gpu_round_trip_q100(ctx, monkeypatch, product_q100, name, rows, tokens):
    """The product's decoder on the product's streams (Y2 levels times the dequantiser
    well past i16 / 8), both token parsers and both kernel families, against the oracle."""
    import zwebp
    if rows != "default":
        monkeypatch.setenv("ZW_DEC_ROWS", rows)
    monkeypatch.setenv("ZW_DEC_TOKENS", tokens)
    for m in (4, 6):
        vp8 = bytes(product_q100[(name, m)])
        rc, r = O.decode(vp8)
        assert rc == 0
        fr = zwebp.vp8_decode_frame(vp8, ctx=ctx)
        for a, b in ((fr.ybuf, r["y"]), (fr.ubuf, r["u"]), (fr.vbuf, r["v"])):
            assert np.array_equal(a, b), (name, m)
