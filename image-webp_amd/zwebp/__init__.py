"""zwebp -- MI355X-native VP8 lossy block-transform pipeline (Python host side).

Thin ctypes layer over the C ABI in ``include/zwebp.h`` (``zwebp/libzwebp.so``,
built by ``make -C image-webp_amd``).  The names mirror the reference crate's
public surface for the lossy path:

  ===============================  =============================================
  here                             reference (zenwebp 0.2.0)
  ===============================  =============================================
  ``encode_frame_lossy``           ``encoder/vp8.rs:3132`` encode_frame_lossy
  ``EncoderParams.lossy``          ``encoder/api.rs:445`` EncoderParams::lossy
  ``WebPEncoder.encode``           ``encoder/api.rs:1291`` WebPEncoder::encode
  ``vp8_decode_frame``             ``decoder/vp8.rs:1526`` Vp8Decoder::decode_frame
  ``WebPDecoder``                  ``decoder/api.rs:306-906`` WebPDecoder (lossy)
  ``decode_rgb/decode_rgba``       ``decoder/api.rs:938-993``
  ``UpsamplingMethod``             ``decoder/api.rs:268``
  ``yuv_to_rgb``                   ``decoder/yuv.rs:82/:402`` fill_rgb_buffer_*
  ``rgb_to_yuv420``                ``decoder/yuv.rs:656`` convert_image_yuv
  ``loop_filter_frame``            ``decoder/vp8.rs:1172`` filter_row_in_cache
  ``EncodingError/DecodingError``  ``encoder/api.rs:35``, ``decoder/api.rs:79``
  ===============================  =============================================

Every call runs on the GPU.  There is no CPU fallback: if the library is not
built, or no HIP device is visible, the first call raises.
"""
import ctypes
import os
import threading
import weakref

import numpy as np

__all__ = [
    "ColorType", "EncoderParams", "WebPEncoder", "ZwError", "EncodingError", "DecodingError", "Context",
    "Frame", "Pipeline", "encode_frame_lossy", "encode_batch", "vp8_decode_frame", "decode_batch",
    "rgb_to_yuv420", "loop_filter_frame", "quant_blocks", "transform_quant_blocks", "library_path", "load_library",
    "UpsamplingMethod", "WebPDecoder", "decode_rgb", "decode_rgba", "vp8_decode_rgb", "decode_rgb_batch",
    "decode_rgb_batch_into", "decode_rgba_into", "decode_rgb_into",
    "decode_batch_device", "decode_batch_device_ptr", "decode_webp_batch_device",
    "decode_batch_device_resized", "decode_batch_device_resized_ptr", "decode_webp_batch_device_resized",
    "vp8_frame_dims",
    "encode_batch_device", "encode_batch_device_ptr", "encode_webp_batch_device",
    "yuv_to_rgb", "webp_parse", "encode_frame_lossless", "encode_alpha",
]

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libzwebp.so"


class ColorType:
    """ColorType (encoder/api.rs:83-92), same discriminants as the C ABI."""
    L8 = 0
    La8 = 1
    Rgb8 = 2
    Rgba8 = 3
    BYTES = {0: 1, 1: 2, 2: 3, 3: 4}


_ERRS = {
    1: "InvalidDimensions", 2: "InvalidBufferSize", 3: "InvalidArgument", 4: "DeviceError",
    5: "Unsupported", 6: "OutOfMemory", 10: "Vp8MagicInvalid", 11: "ColorSpaceInvalid",
    12: "LumaPredictionModeInvalid", 13: "IntraPredictionModeInvalid", 14: "ChromaPredictionModeInvalid",
    15: "BitStreamError", 16: "UnsupportedFeature", 17: "NotEnoughInitData",
    23: "InvalidAlphaPreprocessing", 24: "InvalidCompressionMethod", 25: "HuffmanError", 26: "TransformError",
    27: "InvalidColorCacheBits", 28: "LosslessSignatureInvalid", 29: "VersionNumberInvalid",
}


class ZwError(Exception):
    def __init__(self, code, what=""):
        self.code = code
        self.name = _ERRS.get(code, "Unknown")
        super().__init__(f"{what}: {self.name} (code {code})" if what else f"{self.name} (code {code})")


class EncodingError(ZwError):
    pass


class DecodingError(ZwError):
    pass


def library_path():
    return os.environ.get("ZWEBP_LIB", os.path.join(_HERE, LIB_NAME))


class _Frame(ctypes.Structure):
    _fields_ = [("width", ctypes.c_uint16), ("height", ctypes.c_uint16),
                ("y_stride", ctypes.c_uint32), ("uv_stride", ctypes.c_uint32), ("mb_rows", ctypes.c_uint32),
                ("y", ctypes.c_void_p), ("u", ctypes.c_void_p), ("v", ctypes.c_void_p),
                ("filter_type", ctypes.c_uint8), ("filter_level", ctypes.c_uint8),
                ("sharpness_level", ctypes.c_uint8), ("pad", ctypes.c_uint8)]


class _Bytes(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("len", ctypes.c_size_t)]


class _Image(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("len", ctypes.c_size_t), ("width", ctypes.c_uint32),
                ("height", ctypes.c_uint32), ("color", ctypes.c_int)]


class _EncParams(ctypes.Structure):
    _fields_ = [("use_lossy", ctypes.c_int), ("lossy_quality", ctypes.c_uint8), ("method", ctypes.c_uint8),
                ("use_predictor_transform", ctypes.c_int)]


class _Metadata(ctypes.Structure):
    _fields_ = [("icc", ctypes.c_void_p), ("icc_len", ctypes.c_size_t), ("exif", ctypes.c_void_p),
                ("exif_len", ctypes.c_size_t), ("xmp", ctypes.c_void_p), ("xmp_len", ctypes.c_size_t)]


class _WebpInfo(ctypes.Structure):
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("has_alpha", ctypes.c_int),
                ("is_lossy", ctypes.c_int), ("is_lossless", ctypes.c_int), ("is_animated", ctypes.c_int),
                ("vp8_offset", ctypes.c_uint64), ("vp8_len", ctypes.c_uint64)]


class _WebpInfoEx(ctypes.Structure):
    _fields_ = _WebpInfo._fields_ + [("alph_offset", ctypes.c_uint64), ("alph_len", ctypes.c_uint64)]


WEBP_ALPHA = 1  # ZW_WEBP_ALPHA
WEBP_LOSSLESS = 4  # ZW_WEBP_LOSSLESS


def _webp_flags(alpha, lossless):
    return (WEBP_ALPHA if alpha else 0) | (WEBP_LOSSLESS if lossless else 0)


class _Vp8lTransform(ctypes.Structure):
    _fields_ = [("type", ctypes.c_uint32), ("bits", ctypes.c_uint32), ("data", ctypes.c_void_p),
                ("len", ctypes.c_size_t)]


class _Vp8lImage(ctypes.Structure):
    _fields_ = [("coded", ctypes.c_void_p), ("ntransforms", ctypes.c_int), ("t", _Vp8lTransform * 4)]


class _DeviceImages(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("capacity", ctypes.c_size_t), ("layout", ctypes.c_int),
                ("dtype", ctypes.c_int), ("channels", ctypes.c_int), ("upsampling", ctypes.c_int),
                ("frame_stride", ctypes.c_size_t), ("plane_stride", ctypes.c_size_t),
                ("row_stride", ctypes.c_size_t), ("scale", ctypes.c_float * 4), ("bias", ctypes.c_float * 4)]


class _Rect(ctypes.Structure):
    _fields_ = [("x", ctypes.c_uint32), ("y", ctypes.c_uint32), ("w", ctypes.c_uint32), ("h", ctypes.c_uint32)]


# (name, restype, argtypes) for every symbol in include/zwebp.h
_VP, _SZ, _U32, _I, _U8 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint8
SIGNATURES = [
    ("zw_ctx_create", _I, [_I, ctypes.POINTER(_VP)]),
    ("zw_ctx_destroy", None, [_VP]),
    ("zw_ctx_release_buffers", None, [_VP]),
    ("zw_strerror", ctypes.c_char_p, [_I]),
    ("zw_bytes_free", None, [ctypes.POINTER(_Bytes)]),
    ("zw_frame_free", None, [ctypes.POINTER(_Frame)]),
    ("zw_encode_frame_lossy", _I, [_VP, _VP, _SZ, _U32, _U32, _I, _U8, _U8, ctypes.POINTER(_Bytes)]),
    ("zw_encode_frame_lossy_ex", _I, [_VP, _VP, _SZ, _U32, _U32, _I, _U8, _U8, _I, ctypes.POINTER(_Bytes)]),
    ("zw_encode_webp", _I, [_VP, _VP, _SZ, _U32, _U32, _I, _U8, _U8, ctypes.POINTER(_Bytes)]),
    ("zw_encode_webp_ex", _I, [_VP, _VP, _SZ, _U32, _U32, _I, ctypes.POINTER(_EncParams), ctypes.POINTER(_Metadata),
                               ctypes.POINTER(_Bytes)]),
    ("zw_encode_frame_lossless", _I, [_VP, _SZ, _U32, _U32, _I, _I, ctypes.POINTER(_Bytes)]),
    ("zw_encode_alpha", _I, [_VP, _SZ, _U32, _U32, _I, ctypes.POINTER(_Bytes)]),
    ("zw_encode_batch", _I, [_VP, _I, ctypes.POINTER(_Image), _U8, _U8, ctypes.POINTER(_Bytes)]),
    ("zw_encode_batch_ex", _I, [_VP, _I, ctypes.POINTER(_Image), _U8, _U8, _I, ctypes.POINTER(_Bytes)]),
    ("zw_encode_webp_batch", _I, [_VP, _I, ctypes.POINTER(_Image), _U8, _U8, ctypes.POINTER(_Bytes)]),
    ("zw_vp8_decode_frame", _I, [_VP, _VP, _SZ, ctypes.POINTER(_Frame)]),
    ("zw_vp8_decode_batch", _I, [_VP, _I, ctypes.POINTER(_VP), ctypes.POINTER(_SZ), ctypes.POINTER(_Frame)]),
    ("zw_vp8_decode_rgb", _I, [_VP, _VP, _SZ, _I, _I, ctypes.POINTER(_Bytes), ctypes.POINTER(_U32),
                               ctypes.POINTER(_U32)]),
    ("zw_vp8_decode_rgb_batch", _I, [_VP, _I, ctypes.POINTER(_VP), ctypes.POINTER(_SZ), _I, _I,
                                     ctypes.POINTER(_Bytes), _VP, _VP]),
    ("zw_vp8_decode_rgb_batch_into", _I, [_VP, _I, ctypes.POINTER(_VP), ctypes.POINTER(_SZ), _I, _I,
                                          ctypes.POINTER(_VP), ctypes.POINTER(_SZ), _U32, _VP, _VP]),
    ("zw_vp8_decode_batch_device", _I, [_VP, _I, ctypes.POINTER(_VP), ctypes.POINTER(_SZ),
                                        ctypes.POINTER(_DeviceImages), ctypes.POINTER(_U32), ctypes.POINTER(_U32)]),
    ("zw_vp8_decode_batch_device_resized", _I, [_VP, _I, ctypes.POINTER(_VP), ctypes.POINTER(_SZ),
                                                ctypes.POINTER(_DeviceImages), _U32, _U32, ctypes.POINTER(_Rect),
                                                ctypes.POINTER(_U32), ctypes.POINTER(_U32)]),
    ("zw_dbg_resize_taps", _I, [_U32, _U32, _U32, ctypes.POINTER(ctypes.c_int32)]),
    ("zw_vp8_decode_batch_device_resized_ex", _I, [_VP, _I, ctypes.POINTER(_VP), ctypes.POINTER(_SZ),
                                                   ctypes.POINTER(_DeviceImages), _U32, _U32, ctypes.POINTER(_Rect),
                                                   ctypes.POINTER(_U32), ctypes.POINTER(_U32), _I]),
    ("zw_dbg_resize_aa_taps", _I, [_U32, _U32, _U32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                   ctypes.POINTER(ctypes.c_uint16), _I]),
    ("zw_encode_batch_device", _I, [_VP, _I, ctypes.POINTER(_DeviceImages), _U32, _U32, _U8, _U8, _I,
                                    ctypes.POINTER(_Bytes)]),
    ("zw_pipe_set_input_device", _I, [_VP, ctypes.POINTER(_DeviceImages)]),
    ("zw_webp_parse", _I, [_VP, _SZ, ctypes.POINTER(_WebpInfo)]),
    ("zw_webp_decode_into", _I, [_VP, _VP, _SZ, _I, _I, _VP, _SZ, _U32, ctypes.POINTER(_U32),
                                 ctypes.POINTER(_U32)]),
    ("zw_webp_decode", _I, [_VP, _VP, _SZ, _I, _I, ctypes.POINTER(_Bytes), ctypes.POINTER(_U32),
                            ctypes.POINTER(_U32)]),
    ("zw_decode_rgb_kernel_ms", _I, [_VP, ctypes.POINTER(ctypes.c_float)]),
    ("zw_yuv_to_rgb", _I, [_VP, _VP, _VP, _VP, _U32, _U32, _U32, _U32, _I, _I, _VP]),
    ("zw_rgb_to_yuv420", _I, [_VP, _VP, _U32, _U32, _I, _VP, _VP, _VP]),
    ("zw_transform_quant_blocks", _I, [_VP, _SZ, _VP, _VP, _I, _I, _I, _I, _VP, _VP]),
    ("zw_transform_quant_blocks_device", _I, [_VP, _VP, _SZ, _VP, _VP, _I, _I, _I, _I, _VP, _VP]),
    ("zw_transform_quant_mbs", _I, [_VP, _I, _U32, _U32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("zw_xmb_seg_table_bytes", _SZ, [_I]),
    ("zw_xmb_seg_table", _I, [_I, _VP, _VP]),
    ("zw_transform_quant_mbs_device", _I, [_VP, _VP, _I, _U32, _U32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("zw_transform_quant_mbs_rgb", _I, [_VP, _I, _U32, _U32, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("zw_transform_quant_mbs_rgb_device", _I, [_VP, _VP, _I, _U32, _U32, _I, _VP, _SZ, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("zw_quant_blocks", _I, [_VP, _I, _VP, _VP, _I, _I, _I, _U32, _I, _I, _I, _VP, _VP, _VP]),
    ("zw_loop_filter_frame", _I, [_VP, _VP, _VP, _VP, _U32, _U32, _VP, _I, _I, _I, _I, _I, _VP, _I, _I, _I]),
    ("zw_pipe_create", _I, [_VP, _I, _U32, _U32, _I, _U8, _U8, ctypes.POINTER(_VP)]),
    ("zw_pipe_destroy", None, [_VP]),
    ("zw_pipe_input_device_ptr", _VP, [_VP]),
    ("zw_pipe_upload", _I, [_VP, _I, _VP, _SZ]),
    ("zw_pipe_set_container", _I, [_VP, _I, ctypes.POINTER(_VP)]),
    ("zw_pipe_set_token_partitions", _I, [_VP, _I]),
    ("zw_decode_kernel_times", _I, [_VP, _VP]),
    ("zw_decode_stage_times", _I, [_VP, _VP]),
    ("zw_decode_token_ms", _I, [_VP, _VP]),
    ("zw_decode_token_stages", _I, [_VP, _VP]),
    ("zw_dbg_tokl_frame", _I, [_VP, _SZ, ctypes.POINTER(_I)]),
    ("zw_dbg_seam_stats", _I, [_VP, _I]),
    ("zw_pipe_encode", _I, [_VP]),
    ("zw_pipe_encode_repeat", _I, [_VP, _I]),
    ("zw_pipe_encode_host", _I, [_VP, _I, _VP]),
    ("zw_pipe_run_pass1", _I, [_VP, _I]),
    ("zw_pipe_run_device", _I, [_VP]),
    ("zw_pipe_output", _I, [_VP, _I, ctypes.POINTER(_Bytes)]),
    ("zw_pipe_read_planes", _I, [_VP, _I, _I, _VP, _VP, _VP]),
    ("zw_pipe_read_mbinfo", _I, [_VP, _I, _I, _VP, _VP]),
    ("zw_pipe_read_alpha", _I, [_VP, _I, _VP]),
    ("zw_pipe_enable_debug", _I, [_VP]),
    ("zw_pipe_read_debug", _I, [_VP, _I, _VP]),
    ("zw_pipe_read_segments", _I, [_VP, _I, _VP]),
    ("zw_pipe_read_probs", _I, [_VP, _I, _VP, ctypes.POINTER(_I)]),
    ("zw_pipe_kernel_times", _I, [_VP, ctypes.POINTER(ctypes.c_float), _I]),
    ("zw_pipe_lanes", _I, [_VP]),
    ("zw_pipe_launch_frames", _I, [_VP]),
    ("zw_host_threads", _I, []),
    ("zw_webp_parse_ex", _I, [_VP, _SZ, _I, ctypes.POINTER(_WebpInfoEx)]),
    ("zw_webp_decode_batch_device", _I, [_VP, _I, ctypes.POINTER(_VP), ctypes.POINTER(_SZ), _I,
                                         ctypes.POINTER(_DeviceImages), ctypes.POINTER(_U32), ctypes.POINTER(_U32)]),
    ("zw_webp_decode_ex", _I, [_VP, _VP, _SZ, _I, _I, _I, ctypes.POINTER(_Bytes), ctypes.POINTER(_U32),
                               ctypes.POINTER(_U32)]),
    ("zw_alph_decode", _I, [_VP, _VP, _SZ, _U32, _U32, _VP]),
    ("zw_dbg_alph_plane", _I, [_VP, _SZ, _U32, _U32, _VP, ctypes.POINTER(_I)]),
    ("zw_dbg_vp8l_decode", _I, [_VP, _SZ, _VP, ctypes.POINTER(_U32), ctypes.POINTER(_U32)]),
    ("zw_decode_alpha_times", _I, [_VP, ctypes.POINTER(ctypes.c_float)]),
    ("zw_decode_lossless_times", _I, [_VP, ctypes.POINTER(ctypes.c_float)]),
    ("zw_dbg_vp8l_inverse_host", _I, [_I, ctypes.POINTER(_Vp8lImage), _U32, _U32, _VP]),
    ("zw_dbg_vp8l_inverse_device", _I, [_VP, _I, ctypes.POINTER(_Vp8lImage), _U32, _U32, _VP]),
    ("zw_dbg_vp8l_read_coded", _I, [_VP, _SZ, ctypes.POINTER(_Bytes)]),
]

_LIB = None


def load_library():
    """Load libzwebp.so (no device access).  Raises if it is not built."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise ImportError(f"zwebp: HIP library not built ({path}); run `make -C image-webp_amd`")
        L = ctypes.CDLL(path)
        for name, res, args in SIGNATURES:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _check(rc, what, cls=ZwError):
    if rc != 0:
        raise cls(rc, what)


def host_threads():
    """Host worker threads per process (zw_host_threads)."""
    return load_library().zw_host_threads()


class Context:
    """One HIP device + stream (zw_ctx).  Not thread-safe; one per thread."""

    def __init__(self, device=0):
        L = load_library()
        h = ctypes.c_void_p()
        _check(L.zw_ctx_create(device, ctypes.byref(h)), "zw_ctx_create")
        self._h = h
        self._lib = L
        self.device = device

    @property
    def handle(self):
        return self._h

    def release_buffers(self):
        """Free the grow-only device scratch / pinned staging (zw_ctx_release_buffers)."""
        if self._h:
            self._lib.zw_ctx_release_buffers(self._h)

    def close(self):
        if self._h:
            self._lib.zw_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_DEFAULT = {}


def _ctx(ctx):
    """The caller's context, else this thread's default one (a zw_ctx is not
    thread-safe, and ctypes releases the GIL during every call)."""
    if ctx is not None:
        return ctx
    key = (os.getpid(), threading.get_ident())
    if key not in _DEFAULT:
        dev = int(os.environ.get("LOCAL_RANK", "0")) if os.environ.get("ZWEBP_DEVICE") is None else int(
            os.environ["ZWEBP_DEVICE"])
        _DEFAULT[key] = Context(dev)
    return _DEFAULT[key]


def _take_bytes(L, b):
    out = ctypes.string_at(b.data, b.len) if b.len else b""
    L.zw_bytes_free(ctypes.byref(b))
    return out


def _as_u8(data):
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(data), np.uint8)
    return np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)


def encode_frame_lossy(data, width, height, color, quality=75, method=4, ctx=None, token_partitions=1):
    """encode_frame_lossy (encoder/vp8.rs:3132): raw VP8 frame bytes.
    token_partitions (1, 2, 4, 8): MB row y's tokens in partition y % n
    (vp8.rs:352-354, :1419-1421; the reference fixes 1), coded on parallel
    host threads; 1 gives the reference's bytes."""
    c = _ctx(ctx)
    L = c._lib
    a = _as_u8(data)
    out = _Bytes()
    _check(L.zw_encode_frame_lossy_ex(c.handle, _ptr(a), a.size, width, height, color, quality, method,
                                      token_partitions, ctypes.byref(out)), "encode_frame_lossy", EncodingError)
    return _take_bytes(L, out)


def encode_batch(images, width, height, color, quality=75, method=4, ctx=None, token_partitions=1):
    """Encode many same-sized frames in one device pass; returns list of VP8 frames."""
    c = _ctx(ctx)
    L = c._lib
    arrs = [_as_u8(im) for im in images]
    n = len(arrs)
    imgs = (_Image * n)()
    for i, a in enumerate(arrs):
        imgs[i] = _Image(a.ctypes.data, a.size, width, height, color)
    outs = (_Bytes * n)()
    _check(L.zw_encode_batch_ex(c.handle, n, imgs, quality, method, token_partitions, outs), "encode_batch",
           EncodingError)
    return [_take_bytes(L, outs[i]) for i in range(n)]


def encode_webp_batch(images, width, height, color, quality=75, method=4, ctx=None):
    """n WebPEncoder::encode calls with EncoderParams::lossy(quality, method) in
    one device pass: a RIFF container per frame (VP8X + ALPH for LA8 / RGBA8)."""
    c = _ctx(ctx)
    L = c._lib
    arrs = [_as_u8(im) for im in images]
    n = len(arrs)
    imgs = (_Image * n)()
    for i, a in enumerate(arrs):
        imgs[i] = _Image(a.ctypes.data, a.size, width, height, color)
    outs = (_Bytes * n)()
    _check(L.zw_encode_webp_batch(c.handle, n, imgs, quality, method, outs), "encode_webp_batch", EncodingError)
    return [_take_bytes(L, outs[i]) for i in range(n)]


class EncoderParams:
    """EncoderParams (encoder/api.rs:415-458).  The default is lossless (VP8L),
    quality 95, method 4, predictor transform on, as in the reference."""

    def __init__(self, use_predictor_transform=True, use_lossy=False, lossy_quality=95, method=4):
        self.use_predictor_transform = use_predictor_transform
        self.use_lossy = use_lossy
        self.lossy_quality = lossy_quality
        self.method = method

    @classmethod
    def lossy(cls, quality, method=4):
        return cls(True, True, quality, method)

    @classmethod
    def lossless(cls):
        return cls()

    @classmethod
    def default(cls):
        return cls()

    def _c(self):
        return _EncParams(int(self.use_lossy), self.lossy_quality, self.method, int(self.use_predictor_transform))


class WebPEncoder:
    """WebPEncoder (encoder/api.rs:1244-1398) writing to a bytearray-like sink:
    new / set_params / set_icc_profile / set_exif_metadata / set_xmp_metadata / encode."""

    def __init__(self, writer=None, ctx=None):
        self.writer = writer if writer is not None else bytearray()
        self.params = EncoderParams.default()
        self.ctx = ctx
        self.icc = self.exif = self.xmp = b""

    def set_params(self, params):
        self.params = params

    def set_icc_profile(self, icc):
        self.icc = bytes(icc)

    def set_exif_metadata(self, exif):
        self.exif = bytes(exif)

    def set_xmp_metadata(self, xmp):
        self.xmp = bytes(xmp)

    def encode(self, data, width, height, color):
        # lossless encodes are host entropy coding and need no device
        c = _ctx(self.ctx) if self.params.use_lossy else None
        L = c._lib if c is not None else load_library()
        a = _as_u8(data)
        bufs = [np.frombuffer(m, np.uint8) if m else None for m in (self.icc, self.exif, self.xmp)]
        md = _Metadata(*[x for b in bufs for x in ((b.ctypes.data if b is not None else None),
                                                   (b.size if b is not None else 0))])
        out = _Bytes()
        prm = self.params._c()
        _check(L.zw_encode_webp_ex(c.handle if c is not None else None, _ptr(a) if a.size else None, a.size, width,
                                   height, color, ctypes.byref(prm), ctypes.byref(md), ctypes.byref(out)),
               "WebPEncoder.encode", EncodingError)
        self.writer += _take_bytes(L, out)
        return self.writer


def encode_frame_lossless(data, width, height, color, use_predictor_transform=True):
    """encode_frame_lossless (encoder/api.rs:945): the VP8L bitstream (host coder, no device)."""
    L = load_library()
    a = _as_u8(data)
    out = _Bytes()
    _check(L.zw_encode_frame_lossless(_ptr(a) if a.size else None, a.size, width, height, color,
                                      int(use_predictor_transform), ctypes.byref(out)), "encode_frame_lossless",
           EncodingError)
    return _take_bytes(L, out)


def encode_alpha(data, width, height, color):
    """encode_alpha_lossless (encoder/api.rs:1175): the ALPH chunk payload (host coder, no device)."""
    L = load_library()
    a = _as_u8(data)
    out = _Bytes()
    _check(L.zw_encode_alpha(_ptr(a) if a.size else None, a.size, width, height, color, ctypes.byref(out)),
           "encode_alpha_lossless", EncodingError)
    return _take_bytes(L, out)


class Frame:
    """Decoded keyframe (decoder/vp8.rs:153-183): MB-aligned Y/U/V planes."""

    def __init__(self, width, height, ybuf, ubuf, vbuf, y_stride, uv_stride, filter_type, filter_level,
                 sharpness_level):
        self.width, self.height = width, height
        self.ybuf, self.ubuf, self.vbuf = ybuf, ubuf, vbuf
        self.y_stride, self.uv_stride = y_stride, uv_stride
        self.filter_type, self.filter_level, self.sharpness_level = filter_type, filter_level, sharpness_level


def _take_frame(L, f):
    """Zero-copy: the planes are numpy views of the library's buffer, freed
    (zw_frame_free) when the last view goes away."""
    ysz = f.y_stride * f.mb_rows * 16
    csz = f.uv_stride * f.mb_rows * 8
    buf = (ctypes.c_uint8 * (ysz + 2 * csz)).from_address(f.y)
    owner = _Frame()
    ctypes.pointer(owner)[0] = f
    weakref.finalize(buf, L.zw_frame_free, owner)
    a = np.ctypeslib.as_array(buf)
    return Frame(f.width, f.height, a[:ysz], a[ysz:ysz + csz], a[ysz + csz:], f.y_stride, f.uv_stride,
                 f.filter_type, f.filter_level, f.sharpness_level)


def vp8_decode_frame(data, ctx=None):
    """Vp8Decoder::decode_frame (decoder/vp8.rs:1526)."""
    c = _ctx(ctx)
    L = c._lib
    a = _as_u8(data)
    f = _Frame()
    _check(L.zw_vp8_decode_frame(c.handle, _ptr(a) if a.size else None, a.size, ctypes.byref(f)),
           "decode_frame", DecodingError)
    return _take_frame(L, f)


def decode_batch(frames, ctx=None):
    c = _ctx(ctx)
    L = c._lib
    arrs = [_as_u8(d) for d in frames]
    n = len(arrs)
    ptrs = (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])
    lens = (ctypes.c_size_t * n)(*[a.size for a in arrs])
    outs = (_Frame * n)()
    _check(L.zw_vp8_decode_batch(c.handle, n, ptrs, lens, outs), "decode_batch", DecodingError)
    return [_take_frame(L, outs[i]) for i in range(n)]


def decode_kernel_times(ctx=None):
    """Device ms of the last decode batch on `ctx`: (k_dec_recon, k_loopfilter)."""
    c = _ctx(ctx)
    ms = (ctypes.c_float * 2)()
    _check(c._lib.zw_decode_kernel_times(c.handle, ms), "decode_kernel_times")
    return float(ms[0]), float(ms[1])


def decode_token_ms(ctx=None):
    """Device ms of the last decode batch's token parse (k_dec_tokl; 0 when
    the host parsed the tokens)."""
    c = _ctx(ctx)
    ms = ctypes.c_float()
    _check(c._lib.zw_decode_token_ms(c.handle, ctypes.byref(ms)), "decode_token_ms")
    return float(ms.value)


def dbg_tokl_frame(vp8):
    """Test hook (CPU only): (host parse code, match) for the device token
    parse's state machine stepped on the host over one VP8 frame; match 1 =
    records equal to the host parser's (or both failed), 0 = differ, -1 = a
    frame the device parse does not take."""
    L = load_library()
    a = _as_u8(vp8)
    m = ctypes.c_int(-1)
    rc = L.zw_dbg_tokl_frame(_ptr(a) if a.size else None, a.size, ctypes.byref(m))
    return rc, m.value


def dbg_resize_taps(src, dst, o):
    """Test hook (CPU only): (i0, i1, f) of the resize rule for output index
    `o` of `dst` over a source window of `src` pixels (zw_dbg_resize_taps)."""
    L = load_library()
    out = (ctypes.c_int32 * 3)()
    _check(L.zw_dbg_resize_taps(int(src), int(dst), int(o), out), "dbg_resize_taps")
    return int(out[0]), int(out[1]), int(out[2])


def dbg_resize_aa_taps(src, dst, o):
    """Test hook (CPU only): (first, [weights]) of the antialiased resize rule
    for output index `o` of `dst` over a source window of `src` pixels
    (zw_dbg_resize_aa_taps): the taps first .. first + len(weights) - 1 and
    their 12-bit weights, which sum to 4096."""
    L = load_library()
    src, dst, o = int(src), int(dst), int(o)
    cap = (2 * max(src, dst) + dst - 1) // dst if dst > 0 else 1
    first, count = ctypes.c_int32(0), ctypes.c_int32(0)
    w = (ctypes.c_uint16 * max(cap, 1))()
    _check(L.zw_dbg_resize_aa_taps(src, dst, o, ctypes.byref(first), ctypes.byref(count), w, cap), "dbg_resize_aa_taps")
    return int(first.value), [int(w[k]) for k in range(count.value)]


def dbg_seam_stats(reset=False):
    """Test hook: the encode seam's counters (batches led, frames in them, the
    largest batch) since the last reset."""
    L = load_library()
    out = (ctypes.c_uint64 * 3)()
    _check(L.zw_dbg_seam_stats(out, 1 if reset else 0), "dbg_seam_stats")
    return int(out[0]), int(out[1]), int(out[2])


def decode_token_stages(ctx=None):
    """Device time of the last batch's token parse by stage (ms): stage 1
    (k_dec_tok1, the decision chains), the count pass + offsets (k_dec_tok2
    count, scans, and the host's wait for the total), the record pass."""
    c = _ctx(ctx)
    ms = (ctypes.c_float * 3)()
    _check(c._lib.zw_decode_token_stages(c.handle, ms), "decode_token_stages")
    return float(ms[0]), float(ms[1]), float(ms[2])


def decode_stage_times(ctx=None):
    """Host stages of the last decode batch on `ctx`, wall ms summed over its
    chunks: (parse, download, fan-out)."""
    c = _ctx(ctx)
    ms = (ctypes.c_float * 3)()
    _check(c._lib.zw_decode_stage_times(c.handle, ms), "decode_stage_times")
    return float(ms[0]), float(ms[1]), float(ms[2])


class UpsamplingMethod:
    """UpsamplingMethod (decoder/api.rs:268-279): Bilinear (fancy, default) / Simple."""
    Bilinear = 0
    Simple = 1


def _take_image(L, b, w, h, bpp):
    """Zero-copy view of the library's image buffer (zw_bytes_free when unreferenced)."""
    if not b.len:
        L.zw_bytes_free(ctypes.byref(b))
        return np.zeros((h, w, bpp), np.uint8)
    buf = (ctypes.c_uint8 * b.len).from_address(b.data)
    owner = _Bytes(b.data, b.len)
    weakref.finalize(buf, L.zw_bytes_free, owner)
    return np.ctypeslib.as_array(buf).reshape(h, w, bpp)


def vp8_decode_rgb(data, bpp=3, upsampling=UpsamplingMethod.Bilinear, ctx=None):
    """decode_frame + Frame::fill_rgb / fill_rgba (decoder/vp8.rs:200-258) on the device: (h, w, bpp) u8."""
    c = _ctx(ctx)
    L = c._lib
    a = _as_u8(data)
    out, w, h = _Bytes(), ctypes.c_uint32(), ctypes.c_uint32()
    _check(L.zw_vp8_decode_rgb(c.handle, _ptr(a) if a.size else None, a.size, bpp, upsampling, ctypes.byref(out),
                               ctypes.byref(w), ctypes.byref(h)), "decode_rgb", DecodingError)
    return _take_image(L, out, w.value, h.value, bpp)


def decode_rgb_batch(frames, bpp=3, upsampling=UpsamplingMethod.Bilinear, ctx=None):
    """vp8_decode_rgb over a batch (runs of frames of one size, one device pass each)."""
    c = _ctx(ctx)
    L = c._lib
    arrs = [_as_u8(d) for d in frames]
    n = len(arrs)
    ptrs = (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])
    lens = (ctypes.c_size_t * n)(*[a.size for a in arrs])
    outs = (_Bytes * n)()
    ws, hs = (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    _check(L.zw_vp8_decode_rgb_batch(c.handle, n, ptrs, lens, bpp, upsampling, outs, ws, hs), "decode_rgb_batch",
           DecodingError)
    return [_take_image(L, outs[i], ws[i], hs[i], bpp) for i in range(n)]


def _writable_u8(buf):
    a = np.asarray(buf)
    if a.dtype != np.uint8 or not a.flags.c_contiguous or not a.flags.writeable:
        raise ValueError("output must be a writable C-contiguous uint8 buffer")
    return a


def decode_rgb_batch_into(frames, outs, bpp=3, upsampling=UpsamplingMethod.Bilinear, stride_bytes=None, ctx=None):
    """decode_rgb_batch into the caller's buffers (decode_rgba_into / decode_rgb_into,
    decoder/api.rs:1004-1128): outs[i] is a writable uint8 array of at least
    stride * height bytes, rows stride_bytes apart (one stride for every
    buffer; default the widest frame's width * bpp).  Returns [(width, height)]
    per frame."""
    c = _ctx(ctx)
    L = c._lib
    arrs = [_as_u8(d) for d in frames]
    dst = [_writable_u8(o) for o in outs]
    n = len(arrs)
    if len(dst) != n or n == 0:
        raise ValueError("one output buffer per frame")
    if stride_bytes is None:
        stride_bytes = max(webp_frame_width(a) for a in arrs) * bpp
    ptrs = (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])
    lens = (ctypes.c_size_t * n)(*[a.size for a in arrs])
    optr = (ctypes.c_void_p * n)(*[o.ctypes.data for o in dst])
    olen = (ctypes.c_size_t * n)(*[o.nbytes for o in dst])
    ws, hs = (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    _check(L.zw_vp8_decode_rgb_batch_into(c.handle, n, ptrs, lens, bpp, upsampling, optr, olen, int(stride_bytes),
                                          ws, hs), "decode_rgb_batch_into", DecodingError)
    return [(ws[i], hs[i]) for i in range(n)]


LAYOUTS = {"hwc": 0, "chw": 1}
DTYPES = {"u8": 0, "f16": 1, "f32": 2}


def _layout_code(layout):
    return LAYOUTS[layout] if isinstance(layout, str) else int(layout)


def _dtype_code(dtype):
    return DTYPES[dtype] if isinstance(dtype, str) else int(dtype)


def _vec4(v, default):
    """scale / bias: None, one number for every channel, or up to 4 per-channel values."""
    if v is None:
        return [default] * 4
    a = [float(x) for x in np.asarray(v, np.float64).reshape(-1)]
    if len(a) == 1:
        a = a * 4
    if len(a) > 4:
        raise ValueError("at most 4 per-channel values")
    return a + [default] * (4 - len(a))


def decode_batch_device_ptr(frames, ptr, capacity, width=None, height=None, channels=3, layout="chw", dtype="u8",
                            upsampling=UpsamplingMethod.Bilinear, scale=None, bias=None, frame_stride=None,
                            plane_stride=None, row_stride=None, ctx=None, _webp_flags=None):
    """zw_vp8_decode_batch_device, raw-pointer form: n VP8 key frames of one
    size into device memory at `ptr` (`capacity` elements of `dtype`), HWC
    (element i*frame_stride + y*row_stride + x*channels + c) or CHW
    (i*frame_stride + c*plane_stride + y*row_stride + x), strides in elements.
    Strides left None are the packed ones for `width` x `height` (the frames'
    size; needed only then).  u8 holds the bytes of decode_rgb_batch (channel 3
    = 255); f32 holds float32(v) * scale[c] + bias[c] (rounded multiply, rounded
    add), f16 that value rounded to nearest even.  Returns (width, height) once
    every write has completed.  The caller makes sure nothing of its own is
    still queued on that memory."""
    c = _ctx(ctx)
    L = c._lib
    arrs = [_as_u8(d) for d in frames]
    n = len(arrs)
    if n == 0:
        raise ValueError("no frames")
    lay = _layout_code(layout)
    if row_stride is None or frame_stride is None or (lay == 1 and plane_stride is None):
        if width is None or height is None:
            raise ValueError("width and height size the default strides")
        if row_stride is None:
            row_stride = width * channels if lay == 0 else width
        if plane_stride is None:
            plane_stride = row_stride * height
        if frame_stride is None:
            frame_stride = row_stride * height if lay == 0 else plane_stride * channels
    out = _DeviceImages(int(ptr), int(capacity), lay, _dtype_code(dtype), int(channels), int(upsampling),
                        int(frame_stride), int(plane_stride or 0), int(row_stride),
                        (ctypes.c_float * 4)(*_vec4(scale, 1.0)), (ctypes.c_float * 4)(*_vec4(bias, 0.0)))
    ptrs = (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])
    lens = (ctypes.c_size_t * n)(*[a.size for a in arrs])
    w, h = ctypes.c_uint32(), ctypes.c_uint32()
    if _webp_flags is not None:  # (whole WebP files: decode_webp_batch_device(alpha=True))
        _check(L.zw_webp_decode_batch_device(c.handle, n, ptrs, lens, int(_webp_flags), ctypes.byref(out),
                                             ctypes.byref(w), ctypes.byref(h)), "decode_webp_batch_device", DecodingError)
        return w.value, h.value
    _check(L.zw_vp8_decode_batch_device(c.handle, n, ptrs, lens, ctypes.byref(out), ctypes.byref(w), ctypes.byref(h)),
           "decode_batch_device", DecodingError)
    return w.value, h.value


def decode_batch_device(frames, out=None, channels=3, layout="chw", dtype="u8", upsampling=UpsamplingMethod.Bilinear,
                        scale=None, bias=None, ctx=None, _webp=None, _dims=None):
    """n VP8 key frames of one size decoded straight into a torch tensor on the
    context's device, with no download, upload or host copy
    (zw_vp8_decode_batch_device; the values are decode_batch_device_ptr's).

    out=None: allocates and returns torch.empty [N, C, H, W] (layout "chw") or
    [N, H, W, C] ("hwc") of `dtype` ("u8", "f16", "f32") with `channels` 3 or 4.
    out = a 4-d tensor [N, C, H, W] or [N, H, W, C] (C = 3 or 4 tells which; a
    tensor both shapes fit is read as `layout`): layout, dtype, channels and
    strides come from it.  Its innermost stride must be 1 (and the channel
    stride 1 for HWC): rows, planes and frames may be padded, nothing else;
    ValueError otherwise, or for a tensor of another device, dtype or size.
    `capacity` is what the tensor's storage holds from its first element.
    torch's current stream is synchronised before the call (a recycled
    allocator block may still have work queued on it); the call returns with
    every write complete.

    torch must initialise its HIP runtime before libzwebp.so loads in the
    process: import torch and touch the device (torch.zeros(1, device="cuda"))
    before the first zwebp call."""
    import torch
    c = _ctx(ctx)
    arrs = [_as_u8(d) for d in frames]
    n = len(arrs)
    if n == 0:
        raise ValueError("no frames")
    a0 = arrs[0]
    w = int(a0[6]) | ((int(a0[7]) & 0x3F) << 8) if a0.size >= 10 else 0
    h = int(a0[8]) | ((int(a0[9]) & 0x3F) << 8) if a0.size >= 10 else 0
    if _dims is not None:  # (whole files that may be lossless: the size the container parse gave)
        w, h = int(_dims[0]), int(_dims[1])
    webp_flags = None
    if _webp is not None:  # (frames = the files' VP8 payloads, for the size; the call takes the files)
        arrs, webp_flags = _webp
    tdt = {0: torch.uint8, 1: torch.float16, 2: torch.float32}
    dev = torch.device("cuda", c.device)
    if out is None:
        lay, dt = _layout_code(layout), _dtype_code(dtype)
        if lay not in (0, 1) or dt not in tdt or channels not in (3, 4):
            raise ValueError("layout hwc | chw, dtype u8 | f16 | f32, channels 3 | 4")
        # (a frame too short for a header: the smallest tensor; the call reports the decoder's error)
        shape = (n, channels, max(h, 1), max(w, 1)) if lay == 1 else (n, max(h, 1), max(w, 1), channels)
        out = torch.empty(shape, dtype=tdt[dt], device=dev)
    if not isinstance(out, torch.Tensor) or out.dim() != 4:
        raise ValueError("out must be a 4-d torch tensor")
    if not out.is_cuda or out.device.index != c.device:
        raise ValueError(f"out must be on cuda:{c.device}")
    dts = [k for k, v in tdt.items() if v == out.dtype]
    if not dts:
        raise ValueError("out must be uint8, float16 or float32")
    sh, st = tuple(out.shape), tuple(out.stride())
    fits_chw = sh[0] == n and sh[1] in (3, 4) and (sh[2], sh[3]) == (h, w)
    fits_hwc = sh[0] == n and sh[3] in (3, 4) and (sh[1], sh[2]) == (h, w)
    if fits_chw and fits_hwc:
        fits_chw = _layout_code(layout) == 1
    if fits_chw:
        lay, ch, fs, ps, rs, unit = 1, sh[1], st[0], st[1], st[2], (st[3],)
    elif fits_hwc:
        lay, ch, fs, ps, rs, unit = 0, sh[3], st[0], 0, st[1], (1 if st[2] == sh[3] else 0, st[3])
    else:
        raise ValueError(f"out must be [{n}, C, {h}, {w}] or [{n}, {h}, {w}, C] with C = 3 or 4")
    if any(u != 1 for u in unit) or min(fs, ps, rs) < 0:
        raise ValueError("out: only rows, planes and frames may be padded (innermost stride 1)")
    capacity = out.untyped_storage().nbytes() // out.element_size() - out.storage_offset()
    torch.cuda.current_stream(dev).synchronize()
    decode_batch_device_ptr(arrs, out.data_ptr(), capacity, w, h, ch, lay, dts[0], upsampling, scale, bias, fs, ps, rs,
                            ctx=c, _webp_flags=webp_flags)
    return out


def decode_webp_batch_device(files, out=None, channels=3, layout="chw", dtype="u8",
                             upsampling=UpsamplingMethod.Bilinear, scale=None, bias=None, ctx=None, alpha=False,
                             lossless=False):
    """decode_batch_device over lossy WebP files: each RIFF container is
    stripped with webp_parse (vp8_offset / vp8_len).  ALPH, VP8L and animated
    files raise DecodingError code 5, as webp_parse does.

    alpha=True (zw_webp_decode_batch_device with ZW_WEBP_ALPHA): files with an
    ALPH chunk decode too; `channels` (or the tensor's) must be 4, and channel 3
    holds each file's alpha (255 for a file without the alpha flag) by the same
    store rule as the colours (u8 the byte; f32 a * scale[3] + bias[3]; f16 that
    rounded to nearest even).  VP8L files (without lossless=True) and animated files raise code 5; a
    file with the alpha flag but no ALPH chunk raises code 20.

    lossless=True (ZW_WEBP_LOSSLESS): lossless (VP8L) files decode too, alone or
    mixed with lossy files of the same size, into 3 or 4 channels: the entropy
    decode on the host threads, the inverse transforms and the store on the
    device.  Channel 3 holds the decoded alpha of a file whose has_alpha is set
    and 255 otherwise.  Animated files still raise code 5."""
    vp8, arrs, dims = [], [], None
    for f in files:
        a = _as_u8(f)
        info = webp_parse(a, alpha=alpha, lossless=lossless)
        arrs.append(a)
        vp8.append(a[info["vp8_offset"]:info["vp8_offset"] + info["vp8_len"]])
        if dims is None:
            dims = (info["width"], info["height"])
    if not alpha and not lossless:
        return decode_batch_device(vp8, out, channels, layout, dtype, upsampling, scale, bias, ctx)
    return decode_batch_device(vp8, out, channels, layout, dtype, upsampling, scale, bias, ctx,
                               _webp=(arrs, _webp_flags(alpha, lossless)), _dims=dims if lossless else None)


def decode_batch_device_resized_ptr(frames, ptr, capacity, out_w, out_h, windows=None, channels=3, layout="chw",
                                    dtype="u8", upsampling=UpsamplingMethod.Bilinear, scale=None, bias=None,
                                    frame_stride=None, plane_stride=None, row_stride=None, ctx=None, antialias=False):
    """zw_vp8_decode_batch_device_resized_ex, raw-pointer form: n VP8 key frames,
    which may differ in size, cropped and resized into n images of `out_w` x
    `out_h` in device memory at `ptr` (`capacity` elements of `dtype`),
    addressed as decode_batch_device_ptr's; strides left None are the packed
    ones for the output size.  windows: None (whole frames) or one (x, y, w, h)
    per frame, in frame pixels (None entries = that whole frame).

    The values follow one integer rule (include/zwebp.h): bilinear, half-pixel
    centres, no antialiasing, taps inside the window, over the bytes
    decode_rgb_batch gives for the whole frame.  u8 holds (S + 32768) >> 16;
    f32 holds float32(S / 65536) * scale[c] + bias[c] (rounded multiply,
    rounded add), f16 that value rounded to nearest even.  A window of the
    output's size gives decode_batch_device's values.

    antialias=True takes the triangle filter instead (ZW_RESIZE_TRIANGLE_AA,
    include/zwebp.h): its support widens with the downscale factor, as PIL's
    and interpolate(mode="bilinear", antialias=True)'s does, in integers with
    12-bit weights; u8 / f32 / f16 store S = (T + 128) >> 8 as above.  An int
    is passed as the C entry's `filter` unchanged.

    Frames are grouped by size and each group is one decode pass: a batch
    costs one pass per distinct size.  Returns [(width, height)], the frames'
    source sizes, once every write has completed."""
    c = _ctx(ctx)
    L = c._lib
    arrs = [_as_u8(d) for d in frames]
    n = len(arrs)
    if n == 0:
        raise ValueError("no frames")
    lay = _layout_code(layout)
    frame_stride, plane_stride, row_stride = _packed_strides(lay, int(out_w), int(out_h), int(channels), frame_stride,
                                                             plane_stride, row_stride)
    out = _DeviceImages(int(ptr), int(capacity), lay, _dtype_code(dtype), int(channels), int(upsampling),
                        int(frame_stride), int(plane_stride or 0), int(row_stride),
                        (ctypes.c_float * 4)(*_vec4(scale, 1.0)), (ctypes.c_float * 4)(*_vec4(bias, 0.0)))
    rects = None
    if windows is not None:
        if len(windows) != n:
            raise ValueError("one window per frame")
        rects = (_Rect * n)()
        for i, r in enumerate(windows):
            if r is None:
                fw, fh = vp8_frame_dims(arrs[i])
                r = (0, 0, fw, fh)
            rects[i] = _Rect(*[int(v) for v in r])
    ptrs = (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])
    lens = (ctypes.c_size_t * n)(*[a.size for a in arrs])
    ws, hs = (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    filt = int(antialias)  # False / True = ZW_RESIZE_BILINEAR / ZW_RESIZE_TRIANGLE_AA
    _check(L.zw_vp8_decode_batch_device_resized_ex(c.handle, n, ptrs, lens, ctypes.byref(out), int(out_w), int(out_h),
                                                   rects, ws, hs, filt), "decode_batch_device_resized", DecodingError)
    return [(ws[i], hs[i]) for i in range(n)]


def decode_batch_device_resized(frames, size=None, out=None, windows=None, channels=3, layout="chw", dtype="u8",
                                upsampling=UpsamplingMethod.Bilinear, scale=None, bias=None, ctx=None, antialias=False):
    """n VP8 key frames, which may differ in size, cropped (windows) and
    resized to one size straight into a torch tensor on the context's device
    (zw_vp8_decode_batch_device_resized; the values and `windows` are
    decode_batch_device_resized_ptr's).  No full-size RGB tensor is made.
    Frames are grouped by size and each group is one decode pass: a batch
    costs one pass per distinct size.  antialias=True: the triangle filter
    (decode_batch_device_resized_ptr), what a loader that downscales wants.

    size = (H, W).  out=None: allocates and returns torch.empty [N, C, H, W]
    (layout "chw") or [N, H, W, C] ("hwc") of `dtype` with `channels` 3 or 4.
    out = a 4-d tensor: size (may then be None; else it must match), layout,
    dtype, channels and strides come from it under decode_batch_device's rules
    (innermost stride 1; rows, planes and frames may be padded; ValueError
    otherwise).  torch's current stream is synchronised before the call; the
    call returns with every write complete.  As for decode_batch_device, torch
    must initialise its HIP runtime before libzwebp.so loads in the process."""
    import torch
    c = _ctx(ctx)
    arrs = [_as_u8(d) for d in frames]
    n = len(arrs)
    if n == 0:
        raise ValueError("no frames")
    tdt = {0: torch.uint8, 1: torch.float16, 2: torch.float32}
    dev = torch.device("cuda", c.device)
    if size is not None:
        h, w = int(size[0]), int(size[1])
        if h <= 0 or w <= 0:
            raise ValueError("size = (H, W), both positive")
    if out is None:
        if size is None:
            raise ValueError("size = (H, W) or an out tensor")
        lay, dt = _layout_code(layout), _dtype_code(dtype)
        if lay not in (0, 1) or dt not in tdt or channels not in (3, 4):
            raise ValueError("layout hwc | chw, dtype u8 | f16 | f32, channels 3 | 4")
        out = torch.empty((n, channels, h, w) if lay == 1 else (n, h, w, channels), dtype=tdt[dt], device=dev)
    if not isinstance(out, torch.Tensor) or out.dim() != 4:
        raise ValueError("out must be a 4-d torch tensor")
    if not out.is_cuda or out.device.index != c.device:
        raise ValueError(f"out must be on cuda:{c.device}")
    dts = [k for k, v in tdt.items() if v == out.dtype]
    if not dts:
        raise ValueError("out must be uint8, float16 or float32")
    sh, st = tuple(out.shape), tuple(out.stride())
    fits_chw = sh[0] == n and sh[1] in (3, 4) and (size is None or (sh[2], sh[3]) == (h, w))
    fits_hwc = sh[0] == n and sh[3] in (3, 4) and (size is None or (sh[1], sh[2]) == (h, w))
    if fits_chw and fits_hwc:
        fits_chw = _layout_code(layout) == 1
    if fits_chw:
        lay, ch, h, w, fs, ps, rs, unit = 1, sh[1], sh[2], sh[3], st[0], st[1], st[2], (st[3],)
    elif fits_hwc:
        lay, ch, h, w, fs, ps, rs, unit = 0, sh[3], sh[1], sh[2], st[0], 0, st[1], (1 if st[2] == sh[3] else 0, st[3])
    else:
        raise ValueError(f"out must be [{n}, C, H, W] or [{n}, H, W, C] of `size` with C = 3 or 4")
    if any(u != 1 for u in unit) or min(fs, ps, rs) < 0 or h <= 0 or w <= 0:
        raise ValueError("out: only rows, planes and frames may be padded (innermost stride 1)")
    capacity = out.untyped_storage().nbytes() // out.element_size() - out.storage_offset()
    torch.cuda.current_stream(dev).synchronize()
    decode_batch_device_resized_ptr(arrs, out.data_ptr(), capacity, w, h, windows, ch, lay, dts[0], upsampling, scale,
                                    bias, fs, ps, rs, ctx=c, antialias=antialias)
    return out


def decode_webp_batch_device_resized(files, size=None, out=None, windows=None, channels=3, layout="chw", dtype="u8",
                                     upsampling=UpsamplingMethod.Bilinear, scale=None, bias=None, ctx=None,
                                     antialias=False):
    """decode_batch_device_resized over lossy WebP files: each RIFF container
    is stripped with webp_parse, as decode_webp_batch_device does (ALPH, VP8L
    and animated files raise DecodingError code 5)."""
    vp8 = []
    for f in files:
        a = _as_u8(f)
        info = webp_parse(a)
        vp8.append(a[info["vp8_offset"]:info["vp8_offset"] + info["vp8_len"]])
    return decode_batch_device_resized(vp8, size, out, windows, channels, layout, dtype, upsampling, scale, bias, ctx,
                                       antialias)


def _packed_strides(lay, width, height, channels, frame_stride, plane_stride, row_stride):
    if row_stride is None:
        row_stride = width * channels if lay == 0 else width
    if plane_stride is None:
        plane_stride = row_stride * height
    if frame_stride is None:
        frame_stride = row_stride * height if lay == 0 else plane_stride * channels
    return frame_stride, plane_stride, row_stride


def encode_batch_device_ptr(ptr, capacity, n, width, height, channels=3, layout="chw", dtype="u8", quality=75,
                            method=4, scale=None, bias=None, frame_stride=None, plane_stride=None, row_stride=None,
                            token_partitions=1, upsampling=0, ctx=None):
    """zw_encode_batch_device, raw-pointer form: n frames of `width` x `height`
    read from device memory at `ptr` (`capacity` elements of `dtype`), addressed
    as decode_batch_device_ptr writes them; strides left None are the packed
    ones.  u8 elements are the encoder's bytes; an f32 element x gives
    rint(clamp(float32(x * scale[c]) + bias[c], 0, 255)), ties to even, NaN 0;
    f16 converts to f32 first.  Channel 3 of 4 is never used.  Returns the list
    of VP8 frames, the bytes encode_batch gives for those u8 images.  The
    memory is only read, and every read has completed on return."""
    c = _ctx(ctx)
    L = c._lib
    lay = _layout_code(layout)
    fs, ps, rs = _packed_strides(lay, width, height, channels, frame_stride, plane_stride, row_stride)
    d = _DeviceImages(int(ptr), int(capacity), lay, _dtype_code(dtype), int(channels), int(upsampling), int(fs),
                      int(ps or 0), int(rs), (ctypes.c_float * 4)(*_vec4(scale, 1.0)),
                      (ctypes.c_float * 4)(*_vec4(bias, 0.0)))
    if n <= 0:
        raise ValueError("no frames")
    outs = (_Bytes * n)()
    _check(L.zw_encode_batch_device(c.handle, n, ctypes.byref(d), width, height, quality, method, token_partitions,
                                    outs), "encode_batch_device", EncodingError)
    return [_take_bytes(L, outs[i]) for i in range(n)]


def _tensor_images(tensor, layout, scale, bias, device):
    """(_DeviceImages, n, width, height, channels) of a 4-d torch tensor
    [N, C, H, W] or [N, H, W, C] (C = 3 or 4 tells which; `layout` breaks a
    tie) of uint8 / float16 / float32 on cuda:`device`.  Rows, planes and
    frames may be padded; any other stride is a ValueError."""
    import torch
    tdt = {torch.uint8: 0, torch.float16: 1, torch.float32: 2}
    if not isinstance(tensor, torch.Tensor) or tensor.dim() != 4:
        raise ValueError("a 4-d torch tensor [N, C, H, W] or [N, H, W, C]")
    if not tensor.is_cuda or tensor.device.index != device:
        raise ValueError(f"the tensor must be on cuda:{device}")
    if tensor.dtype not in tdt:
        raise ValueError("the tensor must be uint8, float16 or float32")
    sh, st = tuple(tensor.shape), tuple(tensor.stride())
    if min(sh) < 1:
        raise ValueError("empty tensor")
    fits_chw, fits_hwc = sh[1] in (3, 4), sh[3] in (3, 4)
    if fits_chw and fits_hwc:
        fits_chw = _layout_code(layout) == 1
    if fits_chw:
        lay, ch, h, w, fs, ps, rs, unit = 1, sh[1], sh[2], sh[3], st[0], st[1], st[2], (st[3],)
    elif fits_hwc:
        lay, ch, h, w, fs, ps, rs, unit = 0, sh[3], sh[1], sh[2], st[0], 0, st[1], (1 if st[2] == sh[3] else 0, st[3])
    else:
        raise ValueError("the tensor must be [N, C, H, W] or [N, H, W, C] with C = 3 or 4")
    if any(u != 1 for u in unit) or min(fs, ps, rs) < 0:
        raise ValueError("only rows, planes and frames may be padded (innermost stride 1)")
    capacity = tensor.untyped_storage().nbytes() // tensor.element_size() - tensor.storage_offset()
    d = _DeviceImages(tensor.data_ptr(), capacity, lay, tdt[tensor.dtype], ch, 0, fs, ps, rs,
                      (ctypes.c_float * 4)(*_vec4(scale, 1.0)), (ctypes.c_float * 4)(*_vec4(bias, 0.0)))
    return d, sh[0], w, h, ch


def encode_batch_device(tensor, quality=75, method=4, layout="chw", scale=None, bias=None, token_partitions=1,
                        ctx=None):
    """Encode the frames of a torch tensor on the context's device with no
    download, upload or host copy (zw_encode_batch_device); returns the list of
    VP8 frames.

    tensor: 4-d [N, C, H, W] or [N, H, W, C] with C = 3 or 4 (a tensor both
    shapes fit is read as `layout`), uint8, float16 or float32.  Its innermost
    stride must be 1 (and the channel stride 1 for HWC): rows, planes and
    frames may be padded, nothing else; ValueError otherwise, or for a tensor of
    another device.  The pixel rule is encode_batch_device_ptr's (scale / bias:
    None, one number, or per-channel values); the streams are encode_batch's of
    the u8 images it makes.  `capacity` is what the tensor's storage holds from
    its first element.  torch's current stream is synchronised before the call;
    the tensor is only read, and every read has completed on return.

    torch must initialise its HIP runtime before libzwebp.so loads in the
    process (see decode_batch_device)."""
    import torch
    c = _ctx(ctx)
    d, n, w, h, _ = _tensor_images(tensor, layout, scale, bias, c.device)
    torch.cuda.current_stream(torch.device("cuda", c.device)).synchronize()
    L = c._lib
    outs = (_Bytes * n)()
    _check(L.zw_encode_batch_device(c.handle, n, ctypes.byref(d), w, h, quality, method, token_partitions, outs),
           "encode_batch_device", EncodingError)
    return [_take_bytes(L, outs[i]) for i in range(n)]


def encode_webp_batch_device(tensor, quality=75, method=4, layout="chw", scale=None, bias=None, ctx=None):
    """encode_batch_device with container output: a RIFF "VP8 " file per frame,
    the bytes of encode_webp_batch over the RGB8 images the pixel rule makes.
    3 channels only (ValueError for 4: the ALPH chunk is coded on the host from
    host frames)."""
    c = _ctx(ctx)
    d, n, w, h, ch = _tensor_images(tensor, layout, scale, bias, c.device)
    if ch != 3:
        raise ValueError("container output from a device tensor takes 3 channels")
    p = Pipeline(n, w, h, ColorType.Rgb8, quality, method, ctx=c)
    try:
        p.set_container()
        p.set_input(tensor, layout, scale, bias)
        p.encode()
        return [p.output(i) for i in range(n)]
    finally:
        p.close()


def webp_frame_width(vp8):
    """Width field of a VP8 key-frame header (frame tag + start code + 14-bit width);
    0 for a frame too short to hold one (the decode then reports the error)."""
    a = _as_u8(vp8)
    return int(a[6]) | ((int(a[7]) & 0x3F) << 8) if a.size >= 10 else 0


def vp8_frame_dims(vp8):
    """(width, height) of a VP8 key-frame header (the 14-bit fields; the
    scaling bits are dropped), (0, 0) for a frame too short to hold them.
    What a caller needs to choose windows for decode_batch_device_resized."""
    a = _as_u8(vp8)
    if a.size < 10:
        return 0, 0
    return int(a[6]) | ((int(a[7]) & 0x3F) << 8), int(a[8]) | ((int(a[9]) & 0x3F) << 8)


def _decode_into(data, output, stride_bytes, bpp, ctx):
    c = _ctx(ctx)
    a = _as_u8(data)
    o = _writable_u8(output)
    w, h = ctypes.c_uint32(), ctypes.c_uint32()
    _check(c._lib.zw_webp_decode_into(c.handle, _ptr(a) if a.size else None, a.size, bpp, UpsamplingMethod.Bilinear,
                                      o.ctypes.data, o.nbytes, int(stride_bytes), ctypes.byref(w), ctypes.byref(h)),
           "decode_into", DecodingError)
    return w.value, h.value


def decode_rgba_into(data, output, stride_bytes, ctx=None):
    """decode_rgba_into (decoder/api.rs:1004): decode into `output` with row stride; (width, height)."""
    return _decode_into(data, output, stride_bytes, 4, ctx)


def decode_rgb_into(data, output, stride_bytes, ctx=None):
    """decode_rgb_into (decoder/api.rs:1067): decode into `output` with row stride; (width, height)."""
    return _decode_into(data, output, stride_bytes, 3, ctx)


def decode_rgb_kernel_ms(ctx=None):
    """Device ms of the last RGB decode batch's k_yuv2rgb / k_yuv2rgb_dev launches."""
    c = _ctx(ctx)
    ms = ctypes.c_float()
    _check(c._lib.zw_decode_rgb_kernel_ms(c.handle, ctypes.byref(ms)), "decode_rgb_kernel_ms")
    return float(ms.value)


def webp_parse(data, alpha=False, lossless=False):
    """WebPDecoder::new's container parse (decoder/api.rs:334-510): dict of the header facts.
    alpha=True (zw_webp_parse_ex with ZW_WEBP_ALPHA): a lossy file with the alpha
    flag parses too, and the dict also holds alph_offset / alph_len.
    lossless=True (ZW_WEBP_LOSSLESS): a still VP8L image parses too; vp8_offset /
    vp8_len then give its VP8L payload."""
    L = load_library()
    a = _as_u8(data)
    if alpha or lossless:
        ex = _WebpInfoEx()
        rc = L.zw_webp_parse_ex(_ptr(a) if a.size else None, a.size, _webp_flags(alpha, lossless), ctypes.byref(ex))
        _check(rc, "WebPDecoder::new", DecodingError)
        return {f: getattr(ex, f) for f, _ in _WebpInfoEx._fields_}
    info = _WebpInfo()
    rc = L.zw_webp_parse(_ptr(a) if a.size else None, a.size, ctypes.byref(info))
    _check(rc, "WebPDecoder::new", DecodingError)
    return {f: getattr(info, f) for f, _ in _WebpInfo._fields_}


def _webp_decode(data, bpp, upsampling, ctx, alpha=False, lossless=False):
    c = _ctx(ctx)
    L = c._lib
    a = _as_u8(data)
    out, w, h = _Bytes(), ctypes.c_uint32(), ctypes.c_uint32()
    if alpha or lossless:
        _check(L.zw_webp_decode_ex(c.handle, _ptr(a) if a.size else None, a.size, bpp, upsampling,
                                   _webp_flags(alpha, lossless),
                                   ctypes.byref(out), ctypes.byref(w), ctypes.byref(h)), "decode", DecodingError)
    else:
        _check(L.zw_webp_decode(c.handle, _ptr(a) if a.size else None, a.size, bpp, upsampling, ctypes.byref(out),
                                ctypes.byref(w), ctypes.byref(h)), "decode", DecodingError)
    return _take_image(L, out, w.value, h.value, bpp), w.value, h.value


def decode_rgba(data, ctx=None, alpha=False, lossless=False):
    """decode_rgba (decoder/api.rs:938): (flat RGBA bytes, width, height); lossy files.
    alpha=True: a file with an ALPH chunk decodes with its alpha (zw_webp_decode_ex).
    lossless=True: a lossless file decodes too (alpha 255 unless its has_alpha is set)."""
    img, w, h = _webp_decode(data, 4, UpsamplingMethod.Bilinear, ctx, alpha, lossless)
    return img.reshape(-1), w, h


def alph_decode(payload, width, height, ctx=None):
    """zw_alph_decode: an ALPH chunk payload to the final (height, width) alpha
    plane -- the host reader, then the device filter kernels."""
    c = _ctx(ctx)
    a = _as_u8(payload)
    out = np.empty((int(height), int(width)), np.uint8)
    _check(c._lib.zw_alph_decode(c.handle, _ptr(a) if a.size else None, a.size, int(width), int(height),
                                 out.ctypes.data), "alph_decode", DecodingError)
    return out


def dbg_alph_plane(payload, width, height):
    """zw_dbg_alph_plane (host only): ((height, width) plane before the filter is undone, filter 0..3)."""
    L = load_library()
    a = _as_u8(payload)
    out = np.empty((int(height), int(width)), np.uint8)
    flt = ctypes.c_int()
    _check(L.zw_dbg_alph_plane(_ptr(a) if a.size else None, a.size, int(width), int(height), out.ctypes.data,
                               ctypes.byref(flt)), "dbg_alph_plane", DecodingError)
    return out, flt.value


def dbg_vp8l_decode(data):
    """zw_dbg_vp8l_decode (host only): a headered VP8L stream to a (height, width) uint32 array 0xAARRGGBB."""
    L = load_library()
    a = _as_u8(data)
    w, h = ctypes.c_uint32(), ctypes.c_uint32()
    p = _ptr(a) if a.size else None
    _check(L.zw_dbg_vp8l_decode(p, a.size, None, ctypes.byref(w), ctypes.byref(h)), "dbg_vp8l_decode", DecodingError)
    out = np.empty((h.value, w.value), np.uint32)
    _check(L.zw_dbg_vp8l_decode(p, a.size, out.ctypes.data, ctypes.byref(w), ctypes.byref(h)), "dbg_vp8l_decode",
           DecodingError)
    return out


def decode_alpha_times(ctx=None):
    """zw_decode_alpha_times: (host ALPH ms, filter kernels ms, store kernel ms) of the last alpha decode."""
    c = _ctx(ctx)
    ms = (ctypes.c_float * 3)()
    _check(c._lib.zw_decode_alpha_times(c.handle, ms), "decode_alpha_times")
    return float(ms[0]), float(ms[1]), float(ms[2])


def decode_lossless_times(ctx=None):
    """zw_decode_lossless_times: (host entropy decode ms, transform kernels ms, store kernel ms) of the last
    lossless decode."""
    c = _ctx(ctx)
    ms = (ctypes.c_float * 3)()
    _check(c._lib.zw_decode_lossless_times(c.handle, ms), "decode_lossless_times")
    return float(ms[0]), float(ms[1]), float(ms[2])


def _vp8l_images(images):
    """[(coded (h, tw, 4) u8, [(type, bits, data u8 array or None), ...]), ...] as the C hooks take them."""
    n = len(images)
    arr = (_Vp8lImage * n)()
    keep = []
    for i, (coded, tfs) in enumerate(images):
        c = np.ascontiguousarray(coded, np.uint8)
        keep.append(c)
        arr[i].coded = c.ctypes.data
        arr[i].ntransforms = len(tfs)
        for k, (typ, bits, data) in enumerate(tfs):
            d = np.ascontiguousarray(data if data is not None else np.zeros(0, np.uint8), np.uint8)
            keep.append(d)
            arr[i].t[k].type = int(typ)
            arr[i].t[k].bits = int(bits)
            arr[i].t[k].data = d.ctypes.data if d.size else None
            arr[i].t[k].len = d.size
    return arr, keep


def dbg_vp8l_inverse_host(images, width, height):
    """zw_dbg_vp8l_inverse_host (host only): the inverse transforms of n coded images of one canvas size;
    images = [(coded pixels u8 R, G, B, A of tw * height pixels, [(type, bits, data), ...] in bitstream
    order), ...].  Returns (n, height, width, 4) u8."""
    L = load_library()
    arr, keep = _vp8l_images(images)
    out = np.empty((len(images), int(height), int(width), 4), np.uint8)
    _check(L.zw_dbg_vp8l_inverse_host(len(images), arr, int(width), int(height), out.ctypes.data),
           "dbg_vp8l_inverse_host", DecodingError)
    return out


def dbg_vp8l_inverse_device(images, width, height, ctx=None):
    """zw_dbg_vp8l_inverse_device: the same through the transform kernels, all images in one chunk."""
    c = _ctx(ctx)
    arr, keep = _vp8l_images(images)
    out = np.empty((len(images), int(height), int(width), 4), np.uint8)
    _check(c._lib.zw_dbg_vp8l_inverse_device(c.handle, len(images), arr, int(width), int(height), out.ctypes.data),
           "dbg_vp8l_inverse_device", DecodingError)
    return out


def dbg_vp8l_read_coded(data):
    """zw_dbg_vp8l_read_coded (host only): a headered VP8L stream read up to its transforms:
    (width, height, coded (height, tw, 4) u8, [(type, bits, data u8), ...] in bitstream order)."""
    L = load_library()
    a = _as_u8(data)
    b = _Bytes()
    _check(L.zw_dbg_vp8l_read_coded(_ptr(a) if a.size else None, a.size, ctypes.byref(b)), "dbg_vp8l_read_coded",
           DecodingError)
    blob = _take_bytes(L, b)
    blob = np.frombuffer(blob, np.uint8)
    head = blob[:32].view("<u4")
    w, h, tw, ntf = (int(v) for v in head[:4])
    pos, tfs = 32, []
    for _ in range(ntf):
        typ, bits, nb, _pad = (int(v) for v in blob[pos:pos + 16].view("<u4"))
        pos += 16
        tfs.append((typ, bits, blob[pos:pos + nb].copy()))
        pos += (nb + 3) & ~3
    coded = blob[pos:pos + tw * h * 4].reshape(h, tw, 4).copy()
    return w, h, coded, tfs


def decode_rgb(data, ctx=None, lossless=False):
    """decode_rgb (decoder/api.rs:973): (flat RGB bytes, width, height); lossy files,
    and with lossless=True lossless ones (their alpha dropped)."""
    img, w, h = _webp_decode(data, 3, UpsamplingMethod.Bilinear, ctx, False, lossless)
    return img.reshape(-1), w, h


class WebPDecoder:
    """WebPDecoder (decoder/api.rs:306-906), lossy subset: new / dimensions / has_alpha /
    is_lossy / output_buffer_size / set_lossy_upsampling / read_image."""

    def __init__(self, data, ctx=None, alpha=False, lossless=False):
        self._data = _as_u8(data)
        self._ctx = ctx
        self._alpha = bool(alpha)  # lossy files with an ALPH chunk open and decode to RGBA (api.rs:672-700)
        self._lossless = bool(lossless)  # lossless files open and decode to RGB or RGBA (api.rs:648-660)
        self._info = webp_parse(self._data, alpha=self._alpha, lossless=self._lossless)
        self._up = UpsamplingMethod.Bilinear

    def dimensions(self):
        return self._info["width"], self._info["height"]

    def has_alpha(self):
        return bool(self._info["has_alpha"])

    def is_lossy(self):
        return bool(self._info["is_lossy"])

    def output_buffer_size(self):
        w, h = self.dimensions()
        return w * h * (4 if self.has_alpha() else 3)

    def set_lossy_upsampling(self, method):
        self._up = method

    def read_image(self, buf=None):
        """Decodes into `buf` (a writable u8 buffer of output_buffer_size()) or returns a new array."""
        bpp = 4 if self.has_alpha() else 3
        img, _, _ = _webp_decode(self._data, bpp, self._up, self._ctx, self._alpha and bpp == 4, self._lossless)
        flat = img.reshape(-1)
        if buf is None:
            return flat
        dst = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf.reshape(-1)
        if dst.size != flat.size:
            raise DecodingError(3, "read_image: buffer size")  # ImageTooLarge / InvalidParameter in the reference
        dst[:] = flat
        return dst


def yuv_to_rgb(y, u, v, width, height, y_stride, uv_stride, bpp=3, upsampling=UpsamplingMethod.Bilinear, ctx=None):
    """fill_rgb_buffer_fancy / _simple (decoder/yuv.rs:82 / :402) on the device: (h, w, bpp) u8."""
    c = _ctx(ctx)
    y, u, v = _as_u8(y), _as_u8(u), _as_u8(v)
    out = np.zeros(width * height * bpp, np.uint8)
    _check(c._lib.zw_yuv_to_rgb(c.handle, _ptr(y), _ptr(u), _ptr(v), width, height, y_stride, uv_stride, bpp,
                                upsampling, _ptr(out)), "yuv_to_rgb")
    return out.reshape(height, width, bpp)


def rgb_to_yuv420(img, width, height, bpp, ctx=None):
    """convert_image_yuv (decoder/yuv.rs:656): MB-padded Y, U, V planes."""
    c = _ctx(ctx)
    mbw, mbh = (width + 15) // 16, (height + 15) // 16
    y = np.zeros(mbw * 16 * mbh * 16, np.uint8)
    u = np.zeros(mbw * 8 * mbh * 8, np.uint8)
    v = np.zeros(mbw * 8 * mbh * 8, np.uint8)
    a = _as_u8(img)
    if a.size != width * height * bpp:
        raise EncodingError(2, "rgb_to_yuv420")
    _check(c._lib.zw_rgb_to_yuv420(c.handle, _ptr(a), width, height, bpp, _ptr(y), _ptr(u), _ptr(v)),
           "rgb_to_yuv420")
    return y, u, v


def quant_blocks(coeffs, ctx0, ctype, first, use_trellis, lambda_, q_dc, q_ac, matrix_type, probs=None, ctx=None):
    """Quantise (n,16) natural-order coefficient blocks on the GPU.

    Returns (levels zigzag (n,16) int32, dequantised natural (n,16) int32)."""
    c = _ctx(ctx)
    co = np.ascontiguousarray(coeffs, dtype=np.int32).reshape(-1, 16)
    n = co.shape[0]
    cx = np.ascontiguousarray(np.broadcast_to(np.asarray(ctx0, np.uint8), (n,)))
    pr = None if probs is None else np.ascontiguousarray(probs, dtype=np.uint8).reshape(-1)
    lv = np.zeros((n, 16), np.int32)
    dq = np.zeros((n, 16), np.int32)
    ut = 2 if use_trellis == 2 else (1 if use_trellis else 0)  # 2: lane-parallel trellis kernel
    _check(c._lib.zw_quant_blocks(c.handle, n, _ptr(co), _ptr(cx), ctype, first, ut, lambda_,
                                  q_dc, q_ac, matrix_type, _ptr(pr), _ptr(lv), _ptr(dq)), "quant_blocks")
    return lv, dq


def transform_quant_blocks(src, pred, q_dc, q_ac, matrix_type=0, first=0, ctx=None):
    """Streaming DCT+quant pass on (n,16) u8 source/prediction blocks.

    Returns (levels (n,16) int16 zigzag, recon (n,16) uint8)."""
    c = _ctx(ctx)
    s = np.ascontiguousarray(src, dtype=np.uint8).reshape(-1, 16)
    p = np.ascontiguousarray(pred, dtype=np.uint8).reshape(-1, 16)
    assert s.shape == p.shape
    n = s.shape[0]
    lv = np.zeros((n, 16), np.int16)
    rc = np.zeros((n, 16), np.uint8)
    _check(c._lib.zw_transform_quant_blocks(c.handle, n, _ptr(s), _ptr(p), q_dc, q_ac, matrix_type, first,
                                            _ptr(lv), _ptr(rc)), "transform_quant_blocks")
    return lv, rc


def transform_quant_blocks_device(n, d_src, d_pred, q_dc, q_ac, matrix_type, first, d_levels, d_recon, stream=None,
                                  ctx=None):
    """Device-pointer form (e.g. torch tensor .data_ptr()); asynchronous on `stream` (int handle or None)."""
    c = _ctx(ctx)
    _check(c._lib.zw_transform_quant_blocks_device(c.handle, stream, n, d_src, d_pred, q_dc, q_ac, matrix_type, first,
                                                   d_levels, d_recon), "transform_quant_blocks_device")


def transform_quant_mbs(y, u, v, recs, seg_qi, nframes, mbw, mbh, ctx=None):
    """Streaming DCT+quant pass over per-MB records (zw_transform_quant_mbs):
    the encoder's final transform with the trellis off, every MB independent.

    y/u/v: MB-padded source planes of nframes frames; recs: (nframes*mbw*mbh, 96)
    uint8 records (zwebp.xmb.build_records); seg_qi: (nframes, 4) quantizer
    indices.  Returns (levels (nframes*nmb, 25, 16) int16 zigzag, ry, ru, rv)."""
    c = _ctx(ctx)
    nmb = mbw * mbh
    y, u, v = (np.ascontiguousarray(a, dtype=np.uint8).reshape(-1) for a in (y, u, v))
    r = np.ascontiguousarray(recs, dtype=np.uint8).reshape(-1)
    q = np.ascontiguousarray(seg_qi, dtype=np.int32).reshape(-1)
    if y.size != nframes * nmb * 256 or u.size != nframes * nmb * 64 or v.size != u.size:
        raise ValueError("planes must be MB-padded, nframes frames")
    if r.size != nframes * nmb * 96 or q.size != nframes * 4:
        raise ValueError("one 96-byte record per MB and 4 quantizer indices per frame")
    lv = np.zeros((nframes * nmb, 25, 16), np.int16)
    ry, ru, rv = np.zeros_like(y), np.zeros_like(u), np.zeros_like(v)
    _check(c._lib.zw_transform_quant_mbs(c.handle, nframes, mbw, mbh, _ptr(y), _ptr(u), _ptr(v), _ptr(r), _ptr(q),
                                         _ptr(lv), _ptr(ry), _ptr(ru), _ptr(rv)), "transform_quant_mbs")
    return lv, ry, ru, rv


def xmb_seg_table(seg_qi):
    """Host quantiser table of zw_transform_quant_mbs_device for (nframes, 4) indices (uint8 bytes)."""
    L = load_library()
    q = np.ascontiguousarray(seg_qi, dtype=np.int32).reshape(-1, 4)
    n = q.shape[0]
    out = np.zeros(L.zw_xmb_seg_table_bytes(n), np.uint8)
    _check(L.zw_xmb_seg_table(n, _ptr(q), _ptr(out)), "xmb_seg_table")
    return out


def transform_quant_mbs_device(nframes, mbw, mbh, d_y, d_u, d_v, d_recs, d_segs, d_levels, d_ry, d_ru, d_rv,
                               stream=None, ctx=None):
    """Device-pointer form of transform_quant_mbs; asynchronous on `stream` (int handle or None)."""
    c = _ctx(ctx)
    _check(c._lib.zw_transform_quant_mbs_device(c.handle, stream, nframes, mbw, mbh, d_y, d_u, d_v, d_recs, d_segs,
                                                d_levels, d_ry, d_ru, d_rv), "transform_quant_mbs_device")


def transform_quant_mbs_rgb(img, width, height, bpp, recs, seg_qi, nframes, ctx=None):
    """The streaming pass fused with convert_image_yuv (zw_transform_quant_mbs_rgb):
    nframes RGB (bpp 3) / RGBA (bpp 4) frames of width x height pixels in, the
    same (levels, ry, ru, rv) as transform_quant_mbs on the encoder's MB-padded
    planes of those frames."""
    c = _ctx(ctx)
    mbw, mbh = (width + 15) // 16, (height + 15) // 16
    nmb = mbw * mbh
    im = np.ascontiguousarray(img, dtype=np.uint8).reshape(-1)
    r = np.ascontiguousarray(recs, dtype=np.uint8).reshape(-1)
    q = np.ascontiguousarray(seg_qi, dtype=np.int32).reshape(-1)
    if im.size != nframes * width * height * bpp:
        raise ValueError("nframes frames of width x height x bpp bytes")
    if r.size != nframes * nmb * 96 or q.size != nframes * 4:
        raise ValueError("one 96-byte record per MB and 4 quantizer indices per frame")
    lv = np.zeros((nframes * nmb, 25, 16), np.int16)
    ry = np.zeros(nframes * nmb * 256, np.uint8)
    ru, rv = np.zeros(nframes * nmb * 64, np.uint8), np.zeros(nframes * nmb * 64, np.uint8)
    _check(c._lib.zw_transform_quant_mbs_rgb(c.handle, nframes, width, height, bpp, _ptr(im), _ptr(r), _ptr(q),
                                             _ptr(lv), _ptr(ry), _ptr(ru), _ptr(rv)), "transform_quant_mbs_rgb")
    return lv, ry, ru, rv


def transform_quant_mbs_rgb_device(nframes, width, height, bpp, d_img, img_stride, d_recs, d_segs, d_levels, d_ry,
                                   d_ru, d_rv, stream=None, ctx=None):
    """Device-pointer form of transform_quant_mbs_rgb; asynchronous on `stream`."""
    c = _ctx(ctx)
    _check(c._lib.zw_transform_quant_mbs_rgb_device(c.handle, stream, nframes, width, height, bpp, d_img, img_stride,
                                                    d_recs, d_segs, d_levels, d_ry, d_ru, d_rv),
           "transform_quant_mbs_rgb_device")


def loop_filter_frame(y, u, v, mbw, mbh, mb_flags, filter_type, filter_level, sharpness, segments_enabled=0,
                      seg_delta_values=0, seg_lf_level=(0, 0, 0, 0), lf_adj_enabled=0, ref_delta0=0, mode_delta0=0,
                      ctx=None):
    """In-place VP8 loop filter (decoder/vp8.rs:1172-1345) of MB-aligned planes.

    mb_flags: (mbw*mbh, 4) uint8 rows of (luma_mode, segment, skip, non_zero_dct)."""
    c = _ctx(ctx)
    fl = np.ascontiguousarray(mb_flags, dtype=np.uint8).reshape(-1)
    assert fl.size == mbw * mbh * 4
    for p, n in ((y, mbw * mbh * 256), (u, mbw * mbh * 64), (v, mbw * mbh * 64)):
        assert p.dtype == np.uint8 and p.flags.c_contiguous and p.size == n
    lf = np.asarray(seg_lf_level, dtype=np.int8)
    _check(c._lib.zw_loop_filter_frame(c.handle, _ptr(y), _ptr(u), _ptr(v), mbw, mbh, _ptr(fl), filter_type,
                                       filter_level, sharpness, segments_enabled, seg_delta_values, _ptr(lf),
                                       lf_adj_enabled, ref_delta0, mode_delta0), "loop_filter_frame")


class Pipeline:
    """Device-resident batch encoder (zw_pipe): n frames of one size in HBM."""

    def __init__(self, nframes, width, height, color=ColorType.Rgba8, quality=75, method=4, ctx=None):
        self.ctx = _ctx(ctx)
        L = self._lib = self.ctx._lib
        h = ctypes.c_void_p()
        _check(L.zw_pipe_create(self.ctx.handle, nframes, width, height, color, quality, method, ctypes.byref(h)),
               "zw_pipe_create", EncodingError)
        self._h = h
        self.n, self.width, self.height, self.color = nframes, width, height, color
        self.mbw, self.mbh = (width + 15) // 16, (height + 15) // 16

    @property
    def input_ptr(self):
        """Device pointer of the packed input frames (n * w*h*bpp bytes)."""
        return self._lib.zw_pipe_input_device_ptr(self._h)

    def upload(self, i, img):
        a = _as_u8(img)
        _check(self._lib.zw_pipe_upload(self._h, i, _ptr(a), a.size), "zw_pipe_upload")

    def set_container(self, host_frames=None, enable=True):
        """Outputs become WebP containers (WebPEncoder::encode, lossy params);
        for LA8 / RGBA8 the ALPH chunk is encoded from host_frames[i], which the
        pipeline keeps referenced."""
        self._host_frames = [_as_u8(f) for f in host_frames] if host_frames is not None else None
        ptrs = None
        if self._host_frames is not None:
            ptrs = (ctypes.c_void_p * len(self._host_frames))(*[f.ctypes.data for f in self._host_frames])
        _check(self._lib.zw_pipe_set_container(self._h, 1 if enable else 0, ptrs), "zw_pipe_set_container",
               EncodingError)

    def set_input(self, tensor, layout="chw", scale=None, bias=None):
        """Read the n frames from a torch tensor on the pipeline's device
        (zw_pipe_set_input_device; the tensor and pixel rule of
        encode_batch_device) in encode / encode_repeat / run_pass1 /
        run_device, instead of the packed buffer; set_input(None) switches
        back.  The pipeline must be Rgb8 for 3 channels, Rgba8 for 4.  It keeps
        the tensor referenced; torch's current stream is synchronised here, and
        work queued on the tensor later is the caller's to order."""
        if tensor is None:
            _check(self._lib.zw_pipe_set_input_device(self._h, None), "zw_pipe_set_input_device", EncodingError)
            self._input = None
            return
        import torch
        d, n, w, h, _ = _tensor_images(tensor, layout, scale, bias, self.ctx.device)
        if (n, w, h) != (self.n, self.width, self.height):
            raise ValueError(f"the tensor must hold {self.n} frames of {self.width}x{self.height}")
        torch.cuda.current_stream(torch.device("cuda", self.ctx.device)).synchronize()
        _check(self._lib.zw_pipe_set_input_device(self._h, ctypes.byref(d)), "zw_pipe_set_input_device",
               EncodingError)
        self._input = tensor

    def set_token_partitions(self, n):
        """Token partitions (1, 2, 4, 8) of every frame (zw_pipe_set_token_partitions)."""
        _check(self._lib.zw_pipe_set_token_partitions(self._h, n), "zw_pipe_set_token_partitions", EncodingError)

    def encode(self):
        _check(self._lib.zw_pipe_encode(self._h), "zw_pipe_encode", EncodingError)

    def encode_repeat(self, n):
        """Encode the batch n times back to back with batch k+1's GPU passes
        overlapping batch k's host token emission (streaming throughput)."""
        _check(self._lib.zw_pipe_encode_repeat(self._h, int(n)), "zw_pipe_encode_repeat", EncodingError)

    def encode_host(self, batches):
        """PCIe-inclusive streaming encode (zw_pipe_encode_host): batches is a list
        of nb lists of n host frames; batch b+1 is uploaded while batch b encodes.
        Outputs (output(i)) are the last batch's."""
        nb = len(batches)
        arrs = [_as_u8(im) for bt in batches for im in bt]
        if nb == 0 or len(arrs) != nb * self.n:
            raise ValueError("nb batches of n frames")
        want = self.width * self.height * (1, 2, 3, 4)[self.color]
        if any(a.size != want for a in arrs):
            raise ValueError("every frame must be width*height*bpp bytes")
        ptrs = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        _check(self._lib.zw_pipe_encode_host(self._h, nb, ptrs), "zw_pipe_encode_host", EncodingError)

    def run_pass1(self, write_recon=True):
        _check(self._lib.zw_pipe_run_pass1(self._h, 1 if write_recon else 0), "zw_pipe_run_pass1", EncodingError)

    def run_device(self):
        _check(self._lib.zw_pipe_run_device(self._h), "zw_pipe_run_device", EncodingError)

    def output(self, i):
        b = _Bytes()
        _check(self._lib.zw_pipe_output(self._h, i, ctypes.byref(b)), "zw_pipe_output")
        return _take_bytes(self._lib, b)

    def planes(self, i, which=0):
        ys, cs = self.mbw * self.mbh * 256, self.mbw * self.mbh * 64
        y, u, v = np.zeros(ys, np.uint8), np.zeros(cs, np.uint8), np.zeros(cs, np.uint8)
        _check(self._lib.zw_pipe_read_planes(self._h, i, which, _ptr(y), _ptr(u), _ptr(v)), "zw_pipe_read_planes")
        return y, u, v

    def mbinfo(self, i, pass_=2):
        nmb = self.mbw * self.mbh
        modes = np.zeros((nmb, 20), np.uint8)
        levels = np.zeros((nmb, 25, 16), np.int16)
        _check(self._lib.zw_pipe_read_mbinfo(self._h, i, pass_, _ptr(modes), _ptr(levels)), "zw_pipe_read_mbinfo")
        return modes, levels

    def alpha(self, i):
        a = np.zeros(self.mbw * self.mbh, np.uint8)
        _check(self._lib.zw_pipe_read_alpha(self._h, i, _ptr(a)), "zw_pipe_read_alpha")
        return a

    def enable_debug(self):
        _check(self._lib.zw_pipe_enable_debug(self._h), "zw_pipe_enable_debug")

    def i4_dump(self, i):
        d = np.zeros(self.mbw * self.mbh * 16 * 34, np.int32)
        _check(self._lib.zw_pipe_read_debug(self._h, i, _ptr(d)), "zw_pipe_read_debug")
        return d.reshape(self.mbw * self.mbh, 16, 34)

    def segments(self, i):
        """(4,) int32 quantizer index of each segment of frame i (last encode)."""
        q = np.zeros(4, np.int32)
        _check(self._lib.zw_pipe_read_segments(self._h, i, _ptr(q)), "read_segments")
        return q

    def probs(self, i):
        pr = np.zeros(4 * 8 * 3 * 11, np.uint8)
        sp = ctypes.c_int()
        _check(self._lib.zw_pipe_read_probs(self._h, i, _ptr(pr), ctypes.byref(sp)), "zw_pipe_read_probs")
        return pr, sp.value

    @property
    def lanes(self):
        return self._lib.zw_pipe_lanes(self._h)

    @property
    def launch_frames(self):
        return self._lib.zw_pipe_launch_frames(self._h)

    def kernel_times(self):
        ms = (ctypes.c_float * 9)()
        n = self._lib.zw_pipe_kernel_times(self._h, ms, 9)
        _check(n, "zw_pipe_kernel_times")
        # ms: rgb2yuv, analysis+segments, pass1, pass2 (device); fetch1, stats, fetch2, emit (host wall);
        # emission CPU ms per batch (all lanes' workers)
        return list(ms)

    def close(self):
        if self._h:
            self._lib.zw_pipe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
