"""A restatement of the four VP8L inverse transforms and their chaining, pixel by
pixel in plain loops, written from the format's rules (the reference's
decoder/lossless_transform.rs states the same): the yardstick for the product's
host inverses and transform kernels.  A checker only: nothing of the product is
used here.  Also the case list both hook tests run.

Pixels are (R, G, B, A) bytes.  An image is (coded, transforms): `coded` a
(height, tw, 4) u8 array and `transforms` a list of (type, bits, data) in
bitstream order -- type 0 predictor, 1 cross-colour, 2 subtract-green, 3 colour
indexing; bits = size_bits (types 0, 1) or table_size (type 3); data = the
sub-image (rows, cols, 4) u8 or the table (table_size, 4) u8, None for type 2."""
import functools
import hashlib

import numpy as np

PREDICTOR, COLOR, SUBTRACT_GREEN, INDEXING = 0, 1, 2, 3


def subsample(size, bits):
    return (size + (1 << bits) - 1) >> bits


def index_bits(table_size):
    """log2 of the indices packed into one pixel's green byte."""
    return 3 if table_size <= 2 else 2 if table_size <= 4 else 1 if table_size <= 16 else 0


def _tdiv2(v):
    """v / 2 truncated towards zero."""
    return v // 2 if v >= 0 else -((-v) // 2)


def _clamp(v):
    return 0 if v < 0 else 255 if v > 255 else v


def _avg(a, b):
    return tuple((x + y) // 2 for x, y in zip(a, b))


def _predict(mode, L, T, TL, TR):
    if mode == 0:
        return (0, 0, 0, 255)
    if mode == 1:
        return L
    if mode == 2:
        return T
    if mode == 3:
        return TR
    if mode == 4:
        return TL
    if mode == 5:
        return _avg(_avg(L, TR), T)
    if mode == 6:
        return _avg(L, TL)
    if mode == 7:
        return _avg(L, T)
    if mode == 8:
        return _avg(TL, T)
    if mode == 9:
        return _avg(T, TR)
    if mode == 10:
        return _avg(_avg(L, TL), _avg(T, TR))
    if mode == 11:
        est = [l + t - tl for l, t, tl in zip(L, T, TL)]
        dist_l = sum(abs(e - l) for e, l in zip(est, L))
        dist_t = sum(abs(e - t) for e, t in zip(est, T))
        return L if dist_l < dist_t else T
    if mode == 12:
        return tuple(_clamp(l + t - tl) for l, t, tl in zip(L, T, TL))
    if mode == 13:
        out = []
        for l, t, tl in zip(L, T, TL):
            a = (l + t) // 2
            out.append(_clamp(a + _tdiv2(a - tl)))
        return tuple(out)
    return (0, 0, 0, 0)  # modes 14 and 15 (and anything above) leave the residual


def inverse_predictor(px, w, h, bits, sub):
    """px: flat list of w * h pixel tuples in raster order, changed in place.
    The neighbours are taken by flat index, so the last column's top-right is
    the pixel that follows the row above: the same row's column 0."""
    bxs = subsample(w, bits)
    for y in range(h):
        for x in range(w):
            i = y * w + x
            if y == 0:
                pred = (0, 0, 0, 255) if x == 0 else px[i - 1]
            elif x == 0:
                pred = px[i - w]
            else:
                mode = sub[(y >> bits) * bxs + (x >> bits)][1]
                pred = _predict(mode, px[i - 1], px[i - w], px[i - w - 1], px[i - w + 1])
            px[i] = tuple((r + p) & 255 for r, p in zip(px[i], pred))


def _s8(v):
    return v - 256 if v >= 128 else v


def _delta(t, c):
    return ((_s8(t) * _s8(c)) >> 5) & 255


def inverse_color(px, w, h, bits, sub):
    bxs = subsample(w, bits)
    for y in range(h):
        for x in range(w):
            red_to_blue, green_to_blue, green_to_red, _ = sub[(y >> bits) * bxs + (x >> bits)]
            r, g, b, a = px[y * w + x]
            r = (r + _delta(green_to_red, g)) & 255
            b = (b + _delta(green_to_blue, g) + _delta(red_to_blue, r)) & 255  # (red already updated)
            px[y * w + x] = (r, g, b, a)


def inverse_subtract_green(px):
    for i, (r, g, b, a) in enumerate(px):
        px[i] = ((r + g) & 255, g, (b + g) & 255, a)


def inverse_indexing(px, tw, width, h, table):
    wbits = index_bits(len(table))
    per, bpe = 1 << wbits, 8 >> wbits
    out = []
    for y in range(h):
        for x in range(width):
            k = (px[y * tw + x // per][1] >> ((x % per) * bpe)) & ((1 << bpe) - 1)
            out.append(table[k] if k < len(table) else (0, 0, 0, 0))
    return out


def _tuples(a):
    return [tuple(int(v) for v in p) for p in np.asarray(a, np.uint8).reshape(-1, 4)]


def inverse(coded, transforms, width, height):
    """The final (height, width, 4) image: the transforms undone in reverse order,
    the working width the coded one until the indexing inverse has run."""
    coded = np.asarray(coded, np.uint8)
    w = coded.shape[1]
    px = _tuples(coded)
    for typ, bits, data in reversed(transforms):
        if typ == PREDICTOR:
            inverse_predictor(px, w, height, bits, _tuples(data))
        elif typ == COLOR:
            inverse_color(px, w, height, bits, _tuples(data))
        elif typ == SUBTRACT_GREEN:
            inverse_subtract_green(px)
        else:
            px = inverse_indexing(px, w, width, height, _tuples(data))
            w = width
    assert w == width
    return np.array(px, np.uint8).reshape(height, width, 4)


# ---------------------------------------------------------------------------
# The case list.  A spec is a list, in bitstream order, of
#   ("pred", size_bits, mode)   mode None: random 0..15 per block, else that mode everywhere
#   ("color", size_bits, mult)  mult None: random multipliers, else that byte for all three
#   ("green",)
#   ("index", table_size)
def make_image(rng, width, height, spec, fill=None):
    """(coded, transforms) for a canvas of width x height: random transform data
    and residuals over the full byte range (fill: every residual byte that value)."""
    w, tfs = width, []
    for s in spec:
        if s[0] == "pred":
            sub = rng.integers(0, 256, (subsample(height, s[1]), subsample(w, s[1]), 4), dtype=np.uint8)
            sub[..., 1] = rng.integers(0, 16, sub.shape[:2]) if s[2] is None else s[2]
            tfs.append((PREDICTOR, s[1], sub))
        elif s[0] == "color":
            sub = rng.integers(0, 256, (subsample(height, s[1]), subsample(w, s[1]), 4), dtype=np.uint8)
            if s[2] is not None:
                sub[..., :3] = s[2]
            tfs.append((COLOR, s[1], sub))
        elif s[0] == "green":
            tfs.append((SUBTRACT_GREEN, 0, None))
        else:
            tfs.append((INDEXING, s[1], rng.integers(0, 256, (s[1], 4), dtype=np.uint8)))
            w = subsample(w, index_bits(s[1]))
    if fill is None:
        coded = rng.integers(0, 256, (height, w, 4), dtype=np.uint8)
    else:
        coded = np.full((height, w, 4), fill, np.uint8)
    return coded, tfs


WIDTHS = (1, 2, 3, 63, 64, 65, 97)
HEIGHTS = (1, 2, 64, 65, 130)  # one row, a full band of 64 rows, a band boundary, three bands


def _cases():
    """name -> (width, height, [(spec, fill), ...]): the images of one call."""
    c = {}
    for w in WIDTHS:  # the predictor alone: every width with every height, size_bits 2, 5 and 9 (a block past the image)
        for h in HEIGHTS:
            c[f"pred_{w}x{h}"] = (w, h, [([("pred", b, None)], None) for b in (2, 5, 9)])
    c["pred_fills_65x65"] = (65, 65, [([("pred", 2, None)], 0), ([("pred", 2, None)], 255)])
    # each mode undiluted; 37 columns, so the last column's top-right (column 0) differs from column 36
    for m in range(14):
        c[f"pred_mode{m}_37x70"] = (37, 70, [([("pred", 3, m)], None)])
    c["color_random_65x66"] = (65, 66, [([("color", b, None)], None) for b in (2, 5, 9)])
    c["color_fixed_33x9"] = (33, 9, [([("color", 2, m)], None) for m in (0x80, 0x7F, 0)])
    c["color_fills_33x9"] = (33, 9, [([("color", 2, None)], 0), ([("color", 2, None)], 255)])
    c["green_97x5"] = (97, 5, [([("green",)], None), ([("green",)], 0), ([("green",)], 255)])
    for w in (1, 7, 8, 9, 97):  # indexing: every table size at widths around the pack counts; random indices run past the table
        c[f"index_w{w}"] = (w, 5, [([("index", t)], None) for t in (1, 2, 3, 4, 5, 16, 17, 256)])
    c["index_fills_9x3"] = (9, 3, [([("index", 3)], 0), ([("index", 3)], 255)])
    orders = [[("pred", 2, None), ("color", 3, None), ("green",)],
              [("green",), ("pred", 3, None), ("color", 2, None)],
              [("color", 2, None), ("green",), ("pred", 4, None)]]
    c["chains_67x70"] = (67, 70, [(o, None) for o in orders])
    c["index_then_pred_67x70"] = (67, 70, [([("index", t), ("pred", 2, None)], None) for t in (2, 4, 16, 200)])
    c["empty_9x4"] = (9, 4, [([], None)])
    # nine images with different lists in one call: the per-transform frame lists
    c["nine_lists_41x67"] = (41, 67, [(s, None) for s in (
        orders[0], [], [("pred", 2, None)], [("index", 4), ("pred", 2, None)], [("green",)], orders[1],
        [("pred", 3, None), ("index", 16)], [("color", 2, None)], [("index", 256), ("green",), ("color", 3, None)])])
    return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def case(name):
    """(width, height, images, expected): the images of the named call and the
    restatement's (n, height, width, 4) result, computed once."""
    w, h, specs = CASES[name]
    rng = np.random.default_rng(int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little"))  # a fixed seed per case
    images = [make_image(rng, w, h, spec, fill) for spec, fill in specs]
    want = np.stack([inverse(coded, tfs, w, h) for coded, tfs in images])
    return w, h, images, want


def hook_images(images):
    """The images as zwebp.dbg_vp8l_inverse_* take them."""
    return [(coded, [(t, b, None if d is None else d) for t, b, d in tfs]) for coded, tfs in images]
