"""The host half of the lossless decode's split, no GPU: zw_dbg_vp8l_inverse_host
(the inverse transforms of csrc/zw_vp8l_dec.cpp) against the plain restatement
tests/vp8l_ref.py on its case list, and for every VP8L fixture the split reader
(zw_dbg_vp8l_read_coded) followed by the host inverses against the whole-frame
decode, the manifests' digests and, where it is installed, libwebp."""
import ctypes
import ctypes.util
import json
import os

import numpy as np
import pytest

import alpha_ref as R
import vp8l_ref as V
import zwebp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLDEN, "decode_alpha.json")) as _f:
    OLD = {k: v for k, v in json.load(_f).items() if v["kind"] == "vp8l"}
with open(os.path.join(GOLDEN, "decode_lossless.json")) as _f:
    NEW = json.load(_f)
FIXTURES = [("alpha", n) for n in sorted(OLD)] + [("lossless", n) for n in sorted(NEW)]

_LIBWEBP = ctypes.util.find_library("webp")


def _read(folder, name):
    with open(os.path.join(GOLDEN, folder, name), "rb") as f:
        return f.read()


def rgba_of_argb(argb):
    a = np.asarray(argb, np.uint32)
    return np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255, a >> 24], -1).astype(np.uint8)


@pytest.mark.parametrize("name", sorted(V.CASES))
def test_host_inverse_equals_restatement(name):
    w, h, images, want = V.case(name)
    got = zwebp.dbg_vp8l_inverse_host(V.hook_images(images), w, h)
    assert got.shape == want.shape
    assert np.array_equal(got, want)


@pytest.mark.parametrize("folder,name", FIXTURES)
def test_split_reader_then_host_inverse(folder, name):
    payload = R.chunk(_read(folder, name), b"VP8L")
    whole = rgba_of_argb(zwebp.dbg_vp8l_decode(payload))
    w, h, coded, tfs = zwebp.dbg_vp8l_read_coded(payload)
    assert (h, w) == whole.shape[:2]
    got = zwebp.dbg_vp8l_inverse_host([(coded, tfs)], w, h)[0]
    assert np.array_equal(got, whole), "the split read and the host inverses against decode_frame"
    if folder == "alpha":
        assert [t for t, _, _ in tfs] == OLD[name]["transforms"]
        assert R.sha(zwebp.dbg_vp8l_decode(payload).astype("<u4")) == OLD[name]["argb"]
    else:
        e = NEW[name]
        assert (w, h) == (e["width"], e["height"])
        assert [[t, b] for t, b, _ in tfs] == e["transforms"]
        assert R.sha(got) == e["rgba"], "libwebp's RGBA decode (the manifest's digest)"
    # the restatement on a real stream's transforms (the small fixtures only: it works pixel by pixel)
    if w * h <= 130 * 130:
        assert np.array_equal(V.inverse(coded, tfs, w, h), whole)


@pytest.mark.skipif(_LIBWEBP is None, reason="system libwebp not installed")
@pytest.mark.parametrize("folder,name", FIXTURES)
def test_split_decode_equals_libwebp(folder, name):
    lib = ctypes.CDLL(_LIBWEBP)
    lib.WebPDecodeRGBA.restype = ctypes.POINTER(ctypes.c_uint8)
    lib.WebPDecodeRGBA.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int),
                                   ctypes.POINTER(ctypes.c_int)]
    lib.WebPFree.argtypes = [ctypes.c_void_p]
    data = _read(folder, name)
    payload = R.chunk(data, b"VP8L")
    # libwebp reads the bare VP8L chunk as a simple file: what the stream itself holds, whatever a VP8X header says
    simple = b"RIFF" + (len(payload) + (len(payload) & 1) + 12).to_bytes(4, "little") + b"WEBPVP8L" + \
        len(payload).to_bytes(4, "little") + payload + (b"\0" if len(payload) & 1 else b"")
    wi, hi = ctypes.c_int(), ctypes.c_int()
    p = lib.WebPDecodeRGBA(simple, len(simple), ctypes.byref(wi), ctypes.byref(hi))
    assert p
    want = np.ctypeslib.as_array(p, (hi.value, wi.value, 4)).copy()
    lib.WebPFree(p)
    w, h, coded, tfs = zwebp.dbg_vp8l_read_coded(payload)
    got = zwebp.dbg_vp8l_inverse_host([(coded, tfs)], w, h)[0]
    if not (payload[4] >> 4) & 1:  # (without the header's alpha bit libwebp reports opaque pixels)
        got = got.copy()
        got[..., 3] = 255
    assert np.array_equal(got, want)


def test_hook_refuses_bad_sizes():
    coded = np.zeros((4, 8, 4), np.uint8)
    sub = np.zeros((1, 2, 4), np.uint8)

    def code(tfs, w=8, h=4):
        with pytest.raises(zwebp.DecodingError) as e:
            zwebp.dbg_vp8l_inverse_host([(coded, tfs)], w, h)
        return e.value.code
    assert code([(0, 1, sub)]) == 3  # size_bits below 2
    assert code([(0, 10, sub)]) == 3
    assert code([(0, 2, sub[:, :1])]) == 3  # a sub-image shorter than ceil(8 / 4) x ceil(4 / 4)
    assert code([(2, 0, None), (2, 0, None)]) == 3  # a type given twice
    assert code([(3, 0, sub)]) == 3 and code([(3, 257, sub)]) == 3
    assert code([(4, 2, sub)]) == 3
    assert code([], w=0) == 3


def test_parse_lossless_flag():
    simple = _read("alpha", sorted(OLD)[0])
    with pytest.raises(zwebp.DecodingError) as e:
        zwebp.webp_parse(simple)
    assert e.value.code == 5  # the default keeps refusing
    with pytest.raises(zwebp.DecodingError) as e:
        zwebp.webp_parse(simple, alpha=True)
    assert e.value.code == 5
    info = zwebp.webp_parse(simple, lossless=True)
    chunks = {cc: (off, size) for cc, off, size in R.riff_chunks(simple)}
    assert info["is_lossless"] == 1 and info["is_lossy"] == 0
    assert (info["vp8_offset"], info["vp8_len"]) == chunks[b"VP8L"]
    payload = R.chunk(simple, b"VP8L")
    assert info["has_alpha"] == (payload[4] >> 4) & 1  # bit 28 of the four bytes after the signature
    bad = bytearray(simple)
    bad[20] = 0x2E
    with pytest.raises(zwebp.DecodingError) as e:
        zwebp.webp_parse(bytes(bad), lossless=True)
    assert e.value.code == 28
    bad = bytearray(simple)
    bad[24] |= 0x20
    with pytest.raises(zwebp.DecodingError) as e:
        zwebp.webp_parse(bytes(bad), lossless=True)
    assert e.value.code == 29
    d = zwebp.WebPDecoder(simple, lossless=True)
    assert d.is_lossy() is False and d.dimensions() == (info["width"], info["height"])
    assert d.output_buffer_size() == info["width"] * info["height"] * (4 if info["has_alpha"] else 3)
    L = zwebp.load_library()
    ex = zwebp._WebpInfoEx()
    assert L.zw_webp_parse_ex(simple, len(simple), 2, ctypes.byref(ex)) == 3  # 2 stays an unknown flag
    assert L.zw_webp_parse_ex(simple, len(simple), 8, ctypes.byref(ex)) == 3
    assert L.zw_webp_parse_ex(simple, len(simple), 4, ctypes.byref(ex)) == 0 and ex.is_lossless == 1
    assert L.zw_webp_parse_ex(simple, len(simple), 5, ctypes.byref(ex)) == 0
