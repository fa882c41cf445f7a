"""numpy restatement of the reference's alpha filter (get_alpha_predictor,
decoder/extended.rs:151-211, and the loop of read_image, decoder/api.rs:684-700),
the forward filters the tests build ALPH payloads with, and a few helpers the
alpha tests share.  A checker only: nothing of the product is used here."""
import hashlib

import numpy as np


def predictor(x, y, filt, img):
    """get_alpha_predictor: the prediction of pixel (x, y) from the final plane `img` so far."""
    if filt == 0:
        return 0
    if filt == 1:
        if x == 0 and y == 0:
            return 0
        return int(img[y - 1, 0]) if x == 0 else int(img[y, x - 1])
    if filt == 2:
        if x == 0 and y == 0:
            return 0
        return int(img[0, x - 1]) if y == 0 else int(img[y - 1, x])
    if x == 0 and y == 0:
        left = top = top_left = 0
    elif x == 0:
        left = top = top_left = int(img[y - 1, 0])
    elif y == 0:
        left = top = top_left = int(img[0, x - 1])
    else:
        left, top, top_left = int(img[y, x - 1]), int(img[y - 1, x]), int(img[y - 1, x - 1])
    return min(max(left + top - top_left, 0), 255)


def unfilter(residual, filt):
    """The final alpha plane of a (h, w) u8 residual plane: out = predictor + residual (mod 256),
    pixel by pixel in raster order as read_image does."""
    res = np.asarray(residual, np.uint8)
    if filt == 0:
        return res.copy()
    h, w = res.shape
    out = np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            out[y, x] = (predictor(x, y, filt, out) + int(res[y, x])) & 255
    return out


def forward_filter(plane, filt):
    """The residual plane an encoder stores for the final plane `plane`: residual = plane - predictor."""
    p = np.asarray(plane, np.uint8).astype(np.int32)
    h, w = p.shape
    pred = np.zeros((h, w), np.int32)
    if filt == 1:
        pred[:, 1:] = p[:, :-1]
        pred[1:, 0] = p[:-1, 0]
    elif filt == 2:
        pred[1:, :] = p[:-1, :]
        pred[0, 1:] = p[0, :-1]
    elif filt == 3:
        pred[1:, 1:] = np.clip(p[1:, :-1] + p[:-1, 1:] - p[:-1, :-1], 0, 255)
        pred[0, 1:] = p[0, :-1]
        pred[1:, 0] = p[:-1, 0]
    return ((p - pred) & 255).astype(np.uint8)


def raw_alph(plane, filt, preprocessing=0, compression=0):
    """An ALPH payload with raw (uncompressed) data: the header byte, then the filtered plane."""
    head = bytes([(preprocessing << 4) | (filt << 2) | compression])
    return head + forward_filter(plane, filt).tobytes()


def riff_chunks(data):
    """[(fourcc, payload offset, payload length)] of a RIFF/WEBP file's chunks."""
    out, pos = [], 12
    while pos + 8 <= len(data):
        size = int.from_bytes(data[pos + 4:pos + 8], "little")
        out.append((bytes(data[pos:pos + 4]), pos + 8, size))
        pos += 8 + size + (size & 1)
    return out


def chunk(data, fourcc):
    """The payload of the file's first `fourcc` chunk, or None."""
    for cc, off, size in riff_chunks(data):
        if cc == fourcc:
            return bytes(data[off:off + size])
    return None


def webp_with_alph(vp8, alph, width, height):
    """A VP8X file with the alpha flag: VP8X, ALPH (omitted when None), "VP8 "."""
    def ch(cc, payload):
        return cc + len(payload).to_bytes(4, "little") + payload + (b"\0" if len(payload) & 1 else b"")
    vp8x = bytes([0x10, 0, 0, 0]) + (width - 1).to_bytes(3, "little") + (height - 1).to_bytes(3, "little")
    body = b"WEBP" + ch(b"VP8X", vp8x) + (ch(b"ALPH", alph) if alph is not None else b"") + ch(b"VP8 ", vp8)
    return b"RIFF" + len(body).to_bytes(4, "little") + body


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_planes(w, h, seed):
    """Planes for the filter tests: noise (every running sum wraps mod 256), a
    ramp with steps (the gradient rule's L + T - TL leaves [0, 255] on both
    sides), and blocks of 0 / 255."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
    steps = ((xx * 37 + yy * 91) & 255).astype(np.uint8)
    steps[(xx // 3 + yy // 2) % 2 == 0] ^= 0xFF
    blocks = np.where(((xx // 5) + (yy // 3)) % 2 == 0, 255, 0).astype(np.uint8)
    blocks[rng.integers(0, 8, (h, w)) == 0] = 128
    return {"noise": noise, "steps": steps, "blocks": blocks}


test_planes.__test__ = False  # (a helper, not a test)
