"""Synthesized key frames for the header paths no encoder at hand emits.

tests/golden/synth_*.vp8 are written by tests/vp8_synth.py from the `params`
and random_mbs arguments kept in tests/golden/decode_synth.json
(tools/make_synth_golden.py): sharpness, loop-filter deltas, delta-mode segment
values and their clamps, a segment map that is not updated or only partly
given, quantiser index deltas with their floor and cap, an absent skip flag,
several token partitions beside other header blocks, coefficient probability
updates, every intra mode on every frame edge, the large token categories.  The
expected planes are the system libwebp's (WebPDecodeYUV), except where the
reference knowingly departs from libwebp ("pinned_by": "oracle", with the line
that decides it).

CPU: the writer's bool encoder against the oracle's, the fixtures reproduced
from the manifest, the oracle's decode / header / MB info against what was
written, libwebp again where it is installed, the list of features the
fixtures must keep holding, the device token parse's state machine on the host,
and the product's own header parse (quantisers, filter table, coefficient
probabilities, MB records) against values worked out here from `params`.
GPU: every stream through every decode path, alone and as one batch whose
neighbours differ in every per-frame parameter.  All comparisons are bit-exact.
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
with open(os.path.join(GOLD, "decode_synth.json")) as _f:
    MANIFEST = json.load(_f)["streams"]
BY_NAME = {e["name"]: e for e in MANIFEST}
NAMES = [e["name"] for e in MANIFEST]
MAIN = [e["name"] for e in MANIFEST if (e["width"], e["height"]) == (80, 48)]
QD_KEYS = ("ydc_delta", "y2dc_delta", "y2ac_delta", "uvdc_delta", "uvac_delta")


def _vp8(name):
    with open(os.path.join(GOLD, name + ".vp8"), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def _mbs(name):
    e = BY_NAME[name]
    return S.random_mbs(e["params"], **e["gen"])


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The oracle's decode of a fixture: computed once, shared, never written to."""
    rc, r = O.decode(_vp8(name), want_info=True)
    assert rc == 0
    for k in ("y", "u", "v"):
        r[k].setflags(write=False)
    return r


def _digests(name, y, u, v, y_stride, uv_stride):
    e = BY_NAME[name]
    return S.plane_digests(y, u, v, e["width"], e["height"], y_stride, uv_stride)


# --------------------------------------------------------------------------
# What `params` mean, worked out here (RFC 6386 s9.3, s9.6, s14.1, s15.2;
# the order of the two clamps as the reference has it, decoder/vp8.rs:1470-1523)
# --------------------------------------------------------------------------
def _opt(v):
    return 0 if v is None else v


def _lf_deltas(p):
    d = p["lf_delta"]
    if not d or not d["update"]:
        return 0, 0
    return _opt(d["ref"][0]), _opt(d["mode"][0])


def _lf_trace(p):
    """Per (segment, is_i4): the level before each clamp, the final level, the
    interior limit with how it came about, the hev threshold."""
    seg = p["segments"]
    ref0, mode0 = _lf_deltas(p)
    out = {}
    for s in range(4):
        for i4 in (0, 1):
            t = dict(pre1=p["filter_level"], pre2=0, level=0, ilimit=0, hev=0, floored=False, capped=False, once=0)
            if p["filter_level"] != 0:
                if seg:
                    v = _opt(seg["lf"][s]) if seg["update_data"] else 0
                    t["pre1"] = v if (seg["absolute"] or not seg["update_data"]) else p["filter_level"] + v
                d = (ref0 + (mode0 if i4 else 0)) if p["lf_delta"] else 0
                t["pre2"] = min(max(t["pre1"], 0), 63) + d
                t["once"] = min(max(t["pre1"] + d, 0), 63)  # a decoder that clamps once, after the deltas
                lvl = min(max(t["pre2"], 0), 63)
                il = lvl
                if p["sharpness"] > 0:
                    il >>= 2 if p["sharpness"] > 4 else 1
                    if il > 9 - p["sharpness"]:
                        il, t["capped"] = 9 - p["sharpness"], True
                if il == 0:
                    il, t["floored"] = 1, lvl > 0
                t.update(level=lvl, ilimit=il, hev=2 if lvl >= 40 else (1 if lvl >= 15 else 0))
            out[(s, i4)] = t
    return out


def _used(name):
    """The (segment, is_i4) pairs the stream's MBs take."""
    return {(mb["segment"], int(mb["ymode"] == S.B_PRED)) for mb in _mbs(name)}


def _used_trace(name):
    tr = _lf_trace(BY_NAME[name]["params"])
    return [tr[k] for k in sorted(_used(name))]


def _quant_base(name):
    """Unclamped base quantiser indices of the segments in use."""
    q = S.quant_indices(BY_NAME[name]["params"])
    return [q[s] for s in sorted({s for s, _ in _used(name)})]


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
def test_bool_encoder_matches_oracle_kat():
    """vp8_synth.BoolEncoder (one big integer) against the oracle's byte-wise
    encoder (or_bool_encoder_kat) on random bit / probability sequences, the
    extreme probabilities and long runs that carry included."""
    rng = np.random.default_rng(0xB001)
    seqs = []
    for trial in range(60):
        n = int(rng.integers(1, 600))
        lo, hi = ((1, 256), (1, 4), (250, 256), (120, 136))[trial % 4]
        seqs.append([(int(b), int(p)) for b, p in zip(rng.integers(0, 2, n), rng.integers(lo, hi, n))])
    seqs.append([(1, 1)] * 300)      # the unlikely branch throughout: the value creeps up to a carry
    seqs.append([(0, 255), (1, 255)] * 200)
    seqs.append([(1, 128)] * 257 + [(0, 128)] * 3)
    seqs.append([(0, 1)] * 40)
    for seq in seqs:
        e = S.BoolEncoder()
        for b, p in seq:
            e.put(b, p)
        ops = np.array([(0, b, p) for b, p in seq], np.int32).reshape(-1)
        out = np.zeros(len(seq) + 16, np.uint8)
        n = O.lib().or_bool_encoder_kat(O._p(ops), len(seq), O._p(out), out.size)
        assert n <= out.size and bytes(out[:n]) == e.finish()


@pytest.mark.parametrize("name", NAMES)
def test_writer_reproduces_fixture(name):
    e = BY_NAME[name]
    vp8 = S.write_keyframe(e["params"], _mbs(name))
    assert vp8 == _vp8(name)
    assert len(vp8) <= 8192


@pytest.mark.parametrize("name", NAMES)
def test_oracle_decode_matches_manifest(name):
    r = _oracle(name)
    assert _digests(name, r["y"], r["u"], r["v"], r["mbw"] * 16, r["mbw"] * 8) == BY_NAME[name]["yuv_sha256"]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_header_matches_params(name):
    e, p = BY_NAME[name], BY_NAME[name]["params"]
    rc, h = O.decode_header(_vp8(name))
    assert rc == 0
    seg, data = p["segments"], bool(p["segments"] and p["segments"]["update_data"])
    ref0, mode0 = _lf_deltas(p)
    want = dict(width=e["width"], height=e["height"], mbw=(e["width"] + 15) // 16, mbh=(e["height"] + 15) // 16,
                filter_type=p["filter_type"], filter_level=p["filter_level"], sharpness=p["sharpness"],
                segments_enabled=int(seg is not None), seg_delta_values=int(data and not seg["absolute"]),
                seg_lf_level=[_opt(v) for v in seg["lf"]] if data else [0] * 4,
                seg_quant_level=[_opt(v) for v in seg["quant"]] if data else [0] * 4,
                lf_adj_enabled=int(p["lf_delta"] is not None), ref_delta0=ref0, mode_delta0=mode0,
                num_partitions=1 << p["log2_nparts"])
    got = {k: (list(getattr(h, k)) if isinstance(v, list) else getattr(h, k)) for k, v in want.items()}
    assert got == want
    assert {k for k, _ in O.FrameHdr._fields_} == set(want)  # every field FrameHdr exposes


@pytest.mark.parametrize("name", NAMES)
def test_oracle_mb_info_matches_written(name):
    info, mbs = _oracle(name)["info"], _mbs(name)
    assert len(info) == len(mbs)
    for k, (i, mb) in enumerate(zip(info, mbs)):
        assert (i.luma_mode, i.chroma_mode, i.segment, i.skip) == (mb["ymode"], mb["uvmode"], mb["segment"],
                                                                   mb["skip"]), k
        if mb["ymode"] == S.B_PRED:
            assert list(i.bpred) == mb["bmodes"], k


@pytest.mark.skipif(S.libwebp() is None, reason="system libwebp absent")
@pytest.mark.parametrize("name", NAMES)
def test_libwebp_decode_matches_manifest(name):
    e = BY_NAME[name]
    d = S.libwebp_yuv_digests(_vp8(name))
    assert d is not None, "libwebp rejects the stream"
    if e["pinned_by"] == "libwebp":
        assert d == e["yuv_sha256"]
    else:  # pinned by the oracle because libwebp differs there: still so
        assert d != e["yuv_sha256"] and e["reason"]


@pytest.mark.parametrize("name", NAMES)
def test_tokl_synth(name):
    """The device token parse's state machine on the host: takes single-partition
    frames of two or more MB columns and writes the host parser's records."""
    e = BY_NAME[name]
    taken = e["params"]["log2_nparts"] == 0 and e["width"] > 16
    assert zwebp.dbg_tokl_frame(_vp8(name)) == (0, 1 if taken else -1)


def _edge_modes(names):
    """(edge, luma mode) and (edge, sub-block mode) pairs present over the streams."""
    ymodes, bmodes = set(), set()
    for name in names:
        e = BY_NAME[name]
        mbw, mbh = (e["width"] + 15) // 16, (e["height"] + 15) // 16
        for k, mb in enumerate(_mbs(name)):
            mbx, mby = k % mbw, k // mbw
            edges = [n for n, on in (("top", mby == 0), ("left", mbx == 0), ("right", mbx == mbw - 1),
                                     ("bottom", mby == mbh - 1), ("inside", 0 < mbx < mbw - 1 and 0 < mby < mbh - 1))
                     if on]
            for n in edges:
                ymodes.add((n, mb["ymode"]))
                ymodes.add((n, "uv", mb["uvmode"]))
            if mb["ymode"] == S.B_PRED:
                for i, m in enumerate(mb["bmodes"]):
                    x, y = i % 4, i // 4
                    for n in edges:
                        on = dict(top=y == 0, left=x == 0, right=x == 3, bottom=y == 3, inside=True)[n]
                        if on:
                            bmodes.add((n, m))
    return ymodes, bmodes


def _maxlevel(name):
    return max(int(np.abs(mb["levels"]).max()) for mb in _mbs(name))


def _skipped(name, i4):
    return any(mb["skip"] and (mb["ymode"] == S.B_PRED) == i4 for mb in _mbs(name))


def _nondefault_block(p):
    return bool(p["segments"] or p["lf_delta"] or p["sharpness"] or any(p[k] is not None for k in QD_KEYS))


def _explicit(p):
    s = p["segments"]
    return sum(v is not None for v in s["map_probs"]) if s and s["update_map"] else -1


def _sharp(value, ftype):
    def pred(n, p):
        tr = _used_trace(n)
        return (p["sharpness"], p["filter_type"]) == (value, ftype) and any(t["floored"] for t in tr) and \
            any(t["capped"] for t in tr)
    return pred


def _qd(key, value):
    return lambda n, p: p[key] == value


# Each feature the fixtures must hold: name -> predicate(stream name, params).
# A libwebp-pinned stream must satisfy it, except where noted at the end.
FEATURES = {
    # the rows of header fields and stream properties the other fixtures never take
    "sharpness > 0": lambda n, p: p["sharpness"] > 0,
    "lf deltas through the header, ref and mode non-zero": lambda n, p: all(_lf_deltas(p)),
    "delta-mode segments with non-zero seg_lf": lambda n, p: bool(
        p["segments"] and p["segments"]["update_data"] and not p["segments"]["absolute"]
        and any(_opt(v) for v in p["segments"]["lf"])),
    "negative seg_lf delta clamps at 0": lambda n, p: any(t["pre1"] < 0 for t in _used_trace(n)),
    "seg_lf delta pushes past 63": lambda n, p: any(t["pre1"] > 63 for t in _used_trace(n)),
    "segments enabled, map not updated": lambda n, p: bool(p["segments"] and not p["segments"]["update_map"]),
    "segment tree probabilities partly explicit": lambda n, p: _explicit(p) in (1, 2),
    "negative quantiser deltas at base 0": lambda n, p: p["yac"] == 0 and not p["segments"] and all(
        _opt(p[k]) < 0 for k in QD_KEYS),
    "quantiser deltas clamp at 127": lambda n, p: not p["segments"] and any(
        p["yac"] + _opt(p[k]) > 127 for k in QD_KEYS),
    "y2ac floor of 8 through deltas": lambda n, p: any(
        int(S.AC_QUANT[min(max(b + _opt(p["y2ac_delta"]), 0), 127)]) * 155 // 100 < 8 and _opt(p["y2ac_delta"]) < 0
        for b in _quant_base(n)),
    "uvdc cap of 132 through deltas": lambda n, p: any(
        b >= 117 and _opt(p["uvdc_delta"]) > 0 and int(S.DC_QUANT[min(b + p["uvdc_delta"], 127)]) > 132
        for b in _quant_base(n)),
    "skip flag absent": lambda n, p: p["skip_prob"] is None,
    "simple filter without segments": lambda n, p: p["filter_type"] == 1 and not p["segments"],
    "simple filter with sharpness": lambda n, p: p["filter_type"] == 1 and p["sharpness"] > 0,
    "simple filter with many skipped MBs": lambda n, p: p["filter_type"] == 1 and sum(
        mb["skip"] for mb in _mbs(n)) >= 4,
    "several partitions beside a non-default header": lambda n, p: p["log2_nparts"] > 0 and _nondefault_block(p),
    "token category 3": lambda n, p: any(11 <= abs(v) <= 18 for mb in _mbs(n) for v in mb["levels"].flat),
    "token category 4": lambda n, p: any(19 <= abs(v) <= 34 for mb in _mbs(n) for v in mb["levels"].flat),
    "token category 5": lambda n, p: any(35 <= abs(v) <= 66 for mb in _mbs(n) for v in mb["levels"].flat),
    "token category 6": lambda n, p: _maxlevel(n) >= 67,
    "token category 6 with more than 8 extra bits": lambda n, p: _maxlevel(n) >= 67 + 256,
    # sharpness 1, 4, 7 x both filters, the interior limit on its floor of 1 and on its cap of 9 - sharpness
    **{f"sharpness {v}, filter type {t}, floor and cap": _sharp(v, t) for v in (1, 4, 7) for t in (0, 1)},
    # loop-filter deltas
    "ref_delta0 > 0": lambda n, p: _lf_deltas(p)[0] > 0,
    "ref_delta0 < 0": lambda n, p: _lf_deltas(p)[0] < 0,
    "mode_delta0 > 0": lambda n, p: _lf_deltas(p)[1] > 0,
    "mode_delta0 < 0": lambda n, p: _lf_deltas(p)[1] < 0,
    "lf deltas enabled with the update block": lambda n, p: bool(p["lf_delta"] and p["lf_delta"]["update"]),
    "lf deltas enabled without the update block": lambda n, p: bool(p["lf_delta"] and not p["lf_delta"]["update"]),
    "first clamp decides (low)": lambda n, p: _lf_deltas(p)[0] > 0 and any(
        t["pre1"] < 0 and t["level"] != t["once"] for t in _used_trace(n)),
    "first clamp decides (high)": lambda n, p: any(t["pre1"] > 63 and t["level"] != t["once"] for t in _used_trace(n)),
    "second clamp decides (> 63)": lambda n, p: bool(p["lf_delta"]) and any(t["pre2"] > 63 for t in _used_trace(n)),
    "second clamp decides (< 0)": lambda n, p: bool(p["lf_delta"]) and any(t["pre2"] < 0 for t in _used_trace(n)),
    "frame level 0 beside a non-zero absolute segment level": lambda n, p: bool(
        p["filter_level"] == 0 and p["segments"] and p["segments"]["update_data"] and p["segments"]["absolute"]
        and any(_opt(p["segments"]["lf"][s]) for s, _ in _used(n))),
    # segment values and map
    "segment values absolute": lambda n, p: bool(p["segments"] and p["segments"]["update_data"]
                                                 and p["segments"]["absolute"]),
    "segment values as deltas": lambda n, p: bool(p["segments"] and p["segments"]["update_data"]
                                                  and not p["segments"]["absolute"]),
    "seg_quant delta clamps at 0": lambda n, p: bool(p["segments"]) and min(_quant_base(n)) < 0,
    "seg_quant delta clamps at 127": lambda n, p: bool(p["segments"]) and max(_quant_base(n)) > 127,
    "map not updated, values present": lambda n, p: bool(p["segments"] and not p["segments"]["update_map"]
                                                         and p["segments"]["update_data"]),
    "map updated, no values": lambda n, p: bool(p["segments"] and p["segments"]["update_map"]
                                                and not p["segments"]["update_data"]),
    "one explicit map probability": lambda n, p: _explicit(p) == 1,
    "two explicit map probabilities": lambda n, p: _explicit(p) == 2,
    "three explicit map probabilities": lambda n, p: _explicit(p) == 3,
    # quantiser deltas at both ends
    **{f"{k} = {v}": _qd(k, v) for k in QD_KEYS for v in (-15, 15)},
    # the skip flag
    "skip prob 1": lambda n, p: p["skip_prob"] == 1,
    "skip prob 255": lambda n, p: p["skip_prob"] == 255,
    **{f"skipped {'B_PRED' if i4 else 'I16'} MB, filter type {t}":
       (lambda i4, t: lambda n, p: p["filter_type"] == t and p["filter_level"] > 0 and _skipped(n, i4))(i4, t)
       for i4 in (False, True) for t in (0, 1)},
    "no skip flag, MBs without coefficients, both filters' inner-edge rule": lambda n, p: p["skip_prob"] is None and any(
        not mb["levels"].any() for mb in _mbs(n)),
    # partitions
    **{f"{k} partitions beside a non-default header":
       (lambda k: lambda n, p: 1 << p["log2_nparts"] == k and _nondefault_block(p))(k) for k in (2, 4, 8)},
    # coefficient probabilities
    "every coefficient probability updated": lambda n, p: len(p["coeff_probs"]) == 1056 and min(p["coeff_probs"]) >= 0,
    "no coefficient probability updated": lambda n, p: not p["coeff_probs"],
    # shapes
    "partial MBs on both axes": lambda n, p: p["width"] % 16 and p["height"] % 16,
    "one MB column": lambda n, p: p["width"] <= 16 and p["height"] > 16,
    "more than 16 MB rows, device token parse": lambda n, p: p["height"] > 256 and p["width"] > 16
    and p["log2_nparts"] == 0,
    "more than 16 MB rows, 8 partitions": lambda n, p: p["height"] > 256 and p["log2_nparts"] == 3,
}
# Only a decoder with the reference's two clamps (decoder/vp8.rs:1487, :1496) can pin these.
ORACLE_ONLY = {"first clamp decides (low)", "first clamp decides (high)"}


def test_feature_coverage():
    """A regeneration must not quietly lose a case: every feature has a stream,
    libwebp-pinned unless only the reference's clamp order shows it; at most 3
    streams lean on the oracle alone, and those are exactly the ones on which a
    single clamp gives another filter level."""
    missing = []
    for feat, pred in FEATURES.items():
        pins = {e["pinned_by"] for e in MANIFEST if pred(e["name"], e["params"])}
        if not ("oracle" in pins if feat in ORACLE_ONLY else "libwebp" in pins):
            missing.append(feat)
    assert not missing, missing
    oracle_pinned = [e["name"] for e in MANIFEST if e["pinned_by"] == "oracle"]
    assert len(oracle_pinned) <= 3 and all(BY_NAME[n]["reason"] for n in oracle_pinned)
    for e in MANIFEST:
        differs = any(t["level"] != t["once"] for t in _used_trace(e["name"]))
        assert differs == (e["pinned_by"] == "oracle"), e["name"]
    # every mode on every frame edge (and inside), over the libwebp-pinned streams
    ymodes, bmodes = _edge_modes([e["name"] for e in MANIFEST if e["pinned_by"] == "libwebp"])
    for edge in ("top", "left", "right", "bottom", "inside"):
        assert {m[1:] for m in ymodes if m[0] == edge} >= {(m,) for m in range(5)} | {("uv", m) for m in range(4)}, edge
        assert {m for n, m in bmodes if n == edge} == set(range(10)), edge
    # the main family shares one size and one batch; its neighbours must be able to differ
    assert len(MAIN) >= 20 and len({_frame_key(n) for n in MAIN}) == len(MAIN)


def _frame_key(name):
    """What a batch kernel could wrongly read from another frame."""
    p = BY_NAME[name]["params"]
    s = p["segments"]
    mode = (s["update_map"], s["update_data"], s["absolute"]) if s else None
    return (p["filter_type"], p["sharpness"], _lf_deltas(p) if p["lf_delta"] else None, mode, p["log2_nparts"],
            (p["yac"],) + tuple(p[k] for k in QD_KEYS), p["skip_prob"], bool(p["coeff_probs"]), p["filter_level"])


# ---- the product's own header parse (image-webp_amd/csrc/zw_dec_parse.cpp), on the CPU
@pytest.fixture(scope="module")
def product_dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("synth") / "dec_header_dump")
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
        res[name] = ([int(v) for v in frame[1:]], [int(v) for v in probs[1:]], [[int(v) for v in m[1:]] for m in mbs])
    return res


@pytest.mark.parametrize("name", NAMES)
def test_product_header_tables(product_dump, name):
    """parse_header, the dequantisers, filter_table (from the header, the way
    the decode paths call it) and the coefficient probabilities of the product's
    CPU code against `params`."""
    e, p = BY_NAME[name], BY_NAME[name]["params"]
    frame, probs, _ = product_dump[name]
    seg, data = p["segments"], bool(p["segments"] and p["segments"]["update_data"])
    ref0, mode0 = _lf_deltas(p)
    mbw, mbh = (e["width"] + 15) // 16, (e["height"] + 15) // 16
    want = [e["width"], e["height"], mbw, mbh, p["filter_type"], p["filter_level"], p["sharpness"],
            int(seg is not None), int(bool(seg and seg["update_map"])), int(data and not seg["absolute"]),
            int(p["lf_delta"] is not None), ref0, mode0, 1 << p["log2_nparts"],
            -1 if p["skip_prob"] is None else p["skip_prob"]]
    want += [_opt(v) for v in seg["quant"]] if data else [0] * 4
    want += [_opt(v) for v in seg["lf"]] if data else [0] * 4
    want += [255 if v is None else v for v in seg["map_probs"]] if seg and seg["update_map"] else [255] * 3
    dq = S.dequant_factors(p)
    for s in range(4):
        want += list(dq[s])
    tr = _lf_trace(p)
    want += [p["filter_type"], mbw, mbh]
    for key in ("level", "ilimit", "hev"):
        want += [tr[(s, i4)][key] for s in range(4) for i4 in (0, 1)]
    assert frame == want
    exp = S.COEFF_PROBS.reshape(-1).copy()
    for k, v in enumerate(p["coeff_probs"]):
        if v >= 0:
            exp[k] = v
    assert probs == [int(v) for v in exp]


@pytest.mark.parametrize("name", NAMES)
def test_product_records_match_written(product_dump, name):
    """parse_mbs (the host token parse): every MB's modes, segment, skip flag and
    all 25 x 16 levels are the ones that were written."""
    _, _, recs = product_dump[name]
    for k, (r, mb) in enumerate(zip(recs, _mbs(name))):
        assert r[:4] == [mb["ymode"], mb["uvmode"], mb["skip"], mb["segment"]], k
        if mb["ymode"] == S.B_PRED:
            assert r[4:20] == mb["bmodes"], k
        assert r[20:] == [int(v) for v in mb["levels"].reshape(-1)], k


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    return zwebp.Context(0)


def _same_planes(fr, r):
    return np.array_equal(fr.ybuf, r["y"]) and np.array_equal(fr.ubuf, r["u"]) and np.array_equal(fr.vbuf, r["v"])


@pytest.mark.gpu
@pytest.mark.parametrize("tokens", ["host", "device"])
@pytest.mark.parametrize("rows", ["default", "0"])
@pytest.mark.parametrize("name", NAMES)
def test_gpu_decode_synth(ctx, monkeypatch, name, rows, tokens):
    """vp8_decode_frame with the token partitions parsed on the host and on the
    device, through the row-parallel and the workgroup-per-frame kernels: the
    manifest's digests and the oracle's planes."""
    if rows != "default":
        monkeypatch.setenv("ZW_DEC_ROWS", rows)
    monkeypatch.setenv("ZW_DEC_TOKENS", tokens)
    e = BY_NAME[name]
    fr = zwebp.vp8_decode_frame(_vp8(name), ctx=ctx)
    assert (fr.width, fr.height) == (e["width"], e["height"])
    assert _digests(name, fr.ybuf, fr.ubuf, fr.vbuf, fr.y_stride, fr.uv_stride) == e["yuv_sha256"]
    assert _same_planes(fr, _oracle(name))


def _batch_order():
    """The 80 x 48 streams, each next to the one that differs from it in the
    most per-frame parameters (filter type, sharpness, LF deltas, segment mode,
    partition count; then quantisers, skip probability, coefficient
    probabilities, frame filter level), then once more taking every second one, so that other pairs meet."""
    left, order = list(MAIN[1:]), [MAIN[0]]
    while left:
        a = _frame_key(order[-1])
        nxt = max(left, key=lambda n: sum(x != y for x, y in zip(a, _frame_key(n))))
        left.remove(nxt)
        order.append(nxt)
    order += order[::2] + order[1::2]
    diffs = [[x != y for x, y in zip(_frame_key(a), _frame_key(b))] for a, b in zip(order, order[1:])]
    assert all(any(d) for d in diffs) and all(any(d[k] for d in diffs) for k in range(5))
    return order


def _batch_env(monkeypatch, tokens, rows):
    monkeypatch.setenv("ZW_DEC_TOKENS", tokens)
    monkeypatch.setenv("ZW_DEC_ROWS", rows)
    if tokens == "mixed":
        monkeypatch.setenv("ZW_DEC_CHUNK", "4")
        monkeypatch.setenv("ZW_DEC_TOKENS_HOST", "0.4")


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ["0", "1"])
@pytest.mark.parametrize("tokens", ["device", "mixed"])
def test_gpu_batch_synth(ctx, monkeypatch, tokens, rows):
    """All 80 x 48 streams as one batch: a kernel that takes the filter type,
    sharpness, filter levels, quantisers, probabilities or partitions of another
    frame gives that frame other planes than the oracle's."""
    _batch_env(monkeypatch, tokens, rows)
    order = _batch_order()
    frames = zwebp.decode_batch([_vp8(n) for n in order], ctx=ctx)
    assert len(frames) == len(order)
    bad = [(k, n) for k, (n, fr) in enumerate(zip(order, frames)) if not _same_planes(fr, _oracle(n))]
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ["0", "1"])
@pytest.mark.parametrize("tokens", ["device", "mixed"])
def test_gpu_rgb_batch_synth(ctx, monkeypatch, tokens, rows):
    _batch_env(monkeypatch, tokens, rows)
    order = _batch_order()
    imgs = zwebp.decode_rgb_batch([_vp8(n) for n in order], 4, zwebp.UpsamplingMethod.Bilinear, ctx=ctx)
    want = {}
    for n in set(order):
        r = _oracle(n)
        want[n] = bytes(O.yuv_to_rgb_fancy(r["y"], r["u"], r["v"], 80, 48, 4))
    bad = [(k, n) for k, (n, im) in enumerate(zip(order, imgs)) if bytes(im) != want[n]]
    assert not bad, bad


TRUNCATED = {"synth_lfd_pos": lambda p: bool(p["lf_delta"] and p["lf_delta"]["update"]),
             "synth_sharp4_simple_p4": lambda p: p["log2_nparts"] == 2,
             "synth_skip_absent": lambda p: p["skip_prob"] is None}


@pytest.mark.gpu
@pytest.mark.parametrize("tokens", ["host", "device"])
@pytest.mark.parametrize("name", sorted(TRUNCATED))
def test_gpu_truncated_synth(ctx, monkeypatch, name, tokens):
    """Truncated streams (LF deltas; 4 partitions; no skip flag): the oracle's
    DecodingError variant, or the oracle's planes where it reads zeros past the end."""
    monkeypatch.setenv("ZW_DEC_TOKENS", tokens)
    assert TRUNCATED[name](BY_NAME[name]["params"])
    vp8 = _vp8(name)
    cuts = sorted(set(range(10, len(vp8), max(1, len(vp8) // 24))) | set(range(len(vp8) - 8, len(vp8))))
    errors = 0
    for n in cuts:
        s = vp8[:n]
        rc, r = O.decode(s)
        if rc != 0:
            with pytest.raises(zwebp.DecodingError) as e:
                zwebp.vp8_decode_frame(s, ctx=ctx)
            assert e.value.code == rc, f"cut {n}: variant {e.value.code} != oracle {rc}"
            errors += 1
        else:
            assert _same_planes(zwebp.vp8_decode_frame(s, ctx=ctx), r), n
    assert errors > 0
