"""The host VP8L reader and the ALPH chunk (csrc/zw_vp8l_dec.cpp), no GPU: every
fixture of tests/golden/alpha against the manifest tests/golden/decode_alpha.json
(digests from libwebp and the reference crate's own decodes, see
tools/make_alpha_golden.py), the container parse with and without the alpha
flag, and the ALPH header rules of read_alpha_chunk (decoder/extended.rs:273-334)."""
import ctypes
import ctypes.util
import json
import os

import numpy as np
import pytest

import alpha_ref as R
import zwebp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA = os.path.join(ROOT, "tests", "golden", "alpha")
with open(os.path.join(ROOT, "tests", "golden", "decode_alpha.json")) as _f:
    MANIFEST = json.load(_f)
ALPH_FILES = sorted(k for k, v in MANIFEST.items() if v["kind"] == "alph")
VP8L_FILES = sorted(k for k, v in MANIFEST.items() if v["kind"] == "vp8l")

_LIBWEBP = ctypes.util.find_library("webp")


def _read(name):
    with open(os.path.join(ALPHA, name), "rb") as f:
        return f.read()


def _code(fn, *a, **kw):
    with pytest.raises(zwebp.DecodingError) as e:
        fn(*a, **kw)
    return e.value.code


def test_manifest_covers_the_kinds():
    """One fixture of each kind the reader has a path for."""
    e = [MANIFEST[n] for n in ALPH_FILES]
    assert len([n for n in ALPH_FILES if n.startswith("gallery_")]) == 5
    assert any(x["header"] & 3 == 0 for x in e), "raw data"
    assert any(x["filter"] == 1 for x in e), "a filtered plane"
    assert any(x["header"] >> 4 == 1 for x in e), "the preprocessing bit"
    assert any(x["transforms"] == [] and x["header"] & 3 == 1 for x in e), "no transform"
    assert any(0 in x["transforms"] for x in e), "the predictor transform"
    for bits in (1, 2, 4, 8):
        assert any(n.endswith(f"_b{bits}.webp") for n in ALPH_FILES), f"colour indexing, {bits}-bit indices"
    tf = [t for n in VP8L_FILES for t in MANIFEST[n]["transforms"]]
    assert {0, 1, 2} <= set(tf), "predictor, cross-colour and subtract-green in the lossless fixtures"


@pytest.mark.parametrize("name", ALPH_FILES)
def test_alph_plane_and_final_alpha(name):
    e, data = MANIFEST[name], _read(name)
    info = zwebp.webp_parse(data, alpha=True)
    assert (info["width"], info["height"]) == (e["width"], e["height"]) and info["has_alpha"] == 1
    chunks = {cc: (off, size) for cc, off, size in R.riff_chunks(data)}
    assert (info["alph_offset"], info["alph_len"]) == chunks[b"ALPH"]
    assert (info["vp8_offset"], info["vp8_len"]) == chunks[b"VP8 "]
    payload = data[info["alph_offset"]:info["alph_offset"] + info["alph_len"]]
    assert payload[0] == e["header"]
    plane, filt = zwebp.dbg_alph_plane(payload, e["width"], e["height"])
    assert filt == e["filter"]
    assert R.sha(plane) == e["prefilter"], "the plane before the filter is undone"
    assert R.sha(R.unfilter(plane, filt)) == e["alpha"], "the final alpha plane"


@pytest.mark.skipif(_LIBWEBP is None, reason="system libwebp not installed")
@pytest.mark.parametrize("name", ALPH_FILES)
def test_final_alpha_equals_libwebp(name):
    lib = ctypes.CDLL(_LIBWEBP)
    lib.WebPDecodeRGBA.restype = ctypes.POINTER(ctypes.c_uint8)
    lib.WebPDecodeRGBA.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int),
                                   ctypes.POINTER(ctypes.c_int)]
    lib.WebPFree.argtypes = [ctypes.c_void_p]
    data = _read(name)
    w, h = ctypes.c_int(), ctypes.c_int()
    p = lib.WebPDecodeRGBA(data, len(data), ctypes.byref(w), ctypes.byref(h))
    assert p
    want = np.ctypeslib.as_array(p, (h.value, w.value, 4))[..., 3].copy()
    lib.WebPFree(p)
    info = zwebp.webp_parse(data, alpha=True)
    payload = data[info["alph_offset"]:info["alph_offset"] + info["alph_len"]]
    plane, filt = zwebp.dbg_alph_plane(payload, w.value, h.value)
    assert np.array_equal(R.unfilter(plane, filt), want)


@pytest.mark.parametrize("name", VP8L_FILES)
def test_vp8l_headered_stream(name):
    e, data = MANIFEST[name], _read(name)
    argb = zwebp.dbg_vp8l_decode(R.chunk(data, b"VP8L"))
    assert argb.shape == (e["height"], e["width"]) and argb.dtype == np.uint32
    assert R.sha(argb.astype("<u4")) == e["argb"]


def test_vp8l_header_errors():
    payload = bytearray(R.chunk(_read(VP8L_FILES[0]), b"VP8L"))
    bad = bytearray(payload)
    bad[0] = 0x2E
    assert _code(zwebp.dbg_vp8l_decode, bytes(bad)) == 28  # LosslessSignatureInvalid
    bad = bytearray(payload)
    bad[4] |= 0x20  # version 1
    assert _code(zwebp.dbg_vp8l_decode, bytes(bad)) == 29  # VersionNumberInvalid
    assert _code(zwebp.dbg_vp8l_decode, bytes(payload[:3])) == 15
    assert _code(zwebp.dbg_vp8l_decode, bytes(payload[:len(payload) // 2])) == 15


def test_parse_is_opt_in():
    data = _read("gallery_1.webp")
    assert _code(zwebp.webp_parse, data) == 5  # the default keeps refusing
    assert _code(zwebp.WebPDecoder, data) == 5
    info = zwebp.webp_parse(data, alpha=True)
    assert info["is_lossy"] == 1 and info["is_lossless"] == 0 and info["is_animated"] == 0
    d = zwebp.WebPDecoder(data, alpha=True)
    assert d.has_alpha() and d.is_lossy()
    assert d.output_buffer_size() == info["width"] * info["height"] * 4
    # still out of scope with the flag: VP8L images
    assert _code(zwebp.webp_parse, _read(VP8L_FILES[0]), alpha=True) == 5


def test_alpha_flag_without_alph_chunk():
    data = _read("gallery_1.webp")
    info = zwebp.webp_parse(data, alpha=True)
    vp8 = data[info["vp8_offset"]:info["vp8_offset"] + info["vp8_len"]]
    assert _code(zwebp.webp_parse, R.webp_with_alph(vp8, None, info["width"], info["height"]), alpha=True) == 20
    again = zwebp.webp_parse(R.webp_with_alph(vp8, b"\x00" * 9, info["width"], info["height"]), alpha=True)
    assert again["alph_len"] == 9


def test_parse_ex_flags():
    L = zwebp.load_library()
    data = _read("gallery_1.webp")
    ex = zwebp._WebpInfoEx()
    assert L.zw_webp_parse_ex(data, len(data), 0, ctypes.byref(ex)) == 5  # flags 0 is zw_webp_parse
    assert L.zw_webp_parse_ex(data, len(data), 2, ctypes.byref(ex)) == 3  # an unknown flag
    assert L.zw_webp_parse_ex(data, len(data), 1, ctypes.byref(ex)) == 0 and ex.alph_len > 0


def test_alph_header_rules():
    w, h = 5, 3
    body = bytes(range(w * h))
    for pre in (2, 3):
        assert _code(zwebp.dbg_alph_plane, bytes([pre << 4]) + body, w, h) == 23  # InvalidAlphaPreprocessing
    for comp in (2, 3):
        assert _code(zwebp.dbg_alph_plane, bytes([comp]) + body, w, h) == 24  # InvalidCompressionMethod
    assert _code(zwebp.dbg_alph_plane, b"", w, h) == 15  # an empty payload
    assert _code(zwebp.dbg_alph_plane, bytes([0]) + body[:-1], w, h) == 15  # raw data short of w * h
    for filt in range(4):
        for pre in (0, 1):  # (the preprocessing bit changes nothing)
            plane, f = zwebp.dbg_alph_plane(bytes([(pre << 4) | (filt << 2)]) + body + b"tail", w, h)
            assert f == filt and plane.tobytes() == body


def test_error_names():
    assert zwebp.DecodingError(23).name == "InvalidAlphaPreprocessing"
    assert zwebp.DecodingError(29).name == "VersionNumberInvalid"
    L = zwebp.load_library()
    assert L.zw_strerror(25) == b"invalid lossless Huffman code" and L.zw_strerror(30) == b"unknown error"


def test_forward_filter_inverts():
    """The checker's own two halves agree (the GPU tests build their payloads with forward_filter)."""
    for name, plane in R.test_planes(13, 9, 7).items():
        for filt in range(4):
            assert np.array_equal(R.unfilter(R.forward_filter(plane, filt), filt), plane), (name, filt)
