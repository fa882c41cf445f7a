"""Extreme-contrast encoder inputs (helper module, not a test).

Deterministic RGB frames (h, w, 3) built from numpy formulas, 48 x 48 unless
noted: 3 x 3 MBs, so every MB edge class (top-left, top, left, interior)
exists.  "grey" means R = G = B.  What each is for:

  black, white   grey 0 / 255: the 127/129 borders against a saturated source,
                 Y2 levels near 900 at Q100 with almost every MB skipped
  checker1       grey ((x + y) & 1) * 255: I4 rates past 65 535, so the
                 reference's `rate as u16` wraps and the wrap picks the modes
  vstripe1       grey (x & 1) * 255, hstripe1 grey (y & 1) * 255: the wrap in
                 trials that lose (method 4) and that win (method 6)
  checker16      grey (((x >> 4) + (y >> 4)) & 1) * 255: Y2 levels past 1 024
  binnoise       grey, each pixel 0 or 255 by zwebp.synth._hash32
  diag45         grey ((x + y) % 12 < 6) * 255: LD sub-blocks, Y levels past 256
  diag135        grey ((x - y) % 12 < 6) * 255: RD sub-blocks
  tm             grey clip((9x) % 200 + (13y) % 150 - 40, 0, 255): TM sub-blocks
  sat8           R ((x >> 3) & 1) * 255, B ((y >> 3) & 1) * 255,
                 G (((x + y) >> 4) & 1) * 255: chroma levels past 256
  sat2           R (x & 2 ? 255 : 0), B (y & 2 ? 255 : 0),
                 G ((x + y) & 4 ? 255 : 0): every chroma mode
  uvtm           R clip((x // 2 * 11) % 120 + (y // 2 * 7) % 100, 0, 255),
                 B 255 - R, G 100: every luma and chroma MB mode
  quilt          150 x 100 (ragged both ways): 32-pixel tiles taken cyclically
                 from the fixtures above, a 0..255 ramp and a 128 tile, so that
                 unlike contents are neighbours and contexts, non-zero flags
                 and borders cross between them

SETTINGS[name] lists the (quality, method) pairs a fixture is encoded at; every
fixture keeps Q100, Q75 and Q0.  oracle(name, q, m) caches the oracle's debug
encode, which the census, the validity tests and the GPU comparisons share.
"""
import functools

import numpy as np

import oracle_lib as O
from zwebp.synth import _hash32

RGB8 = 2  # ColorType.Rgb8
SIZE = 48
BINNOISE_SEED = 0x5EEDB100


def _grey(a):
    a = np.asarray(a).astype(np.uint8)
    return np.ascontiguousarray(np.stack([a, a, a], axis=-1))


def _rgb(r, g, b):
    return np.ascontiguousarray(np.stack([np.asarray(c).astype(np.uint8) for c in (r, g, b)], axis=-1))


def _binnoise(x, y):
    idx = y.astype(np.uint64) * np.uint64(65536) + x.astype(np.uint64)
    return (_hash32((np.uint64(BINNOISE_SEED) << np.uint64(32)) + idx) >> np.uint64(31)).astype(np.int64) * 255


def _uvtm(x, y):
    r = np.clip((x // 2 * 11) % 120 + (y // 2 * 7) % 100, 0, 255)
    return _rgb(r, np.full_like(r, 100), 255 - r)


# name -> f(x, y) with x, y int64 coordinate grids -> (h, w, 3) uint8
_FORMULAS = {
    "black": lambda x, y: _grey(np.zeros_like(x)),
    "white": lambda x, y: _grey(np.full_like(x, 255)),
    "checker1": lambda x, y: _grey(((x + y) & 1) * 255),
    "vstripe1": lambda x, y: _grey((x & 1) * 255 + 0 * y),
    "hstripe1": lambda x, y: _grey((y & 1) * 255 + 0 * x),
    "checker16": lambda x, y: _grey((((x >> 4) + (y >> 4)) & 1) * 255),
    "binnoise": lambda x, y: _grey(_binnoise(x, y)),
    "diag45": lambda x, y: _grey(((x + y) % 12 < 6) * 255),
    "diag135": lambda x, y: _grey(((x - y) % 12 < 6) * 255),
    "tm": lambda x, y: _grey(np.clip((9 * x) % 200 + (13 * y) % 150 - 40, 0, 255)),
    "sat8": lambda x, y: _rgb(((x >> 3) & 1) * 255 + 0 * y, (((x + y) >> 4) & 1) * 255, ((y >> 3) & 1) * 255 + 0 * x),
    "sat2": lambda x, y: _rgb(((x & 2) != 0) * 255 + 0 * y, (((x + y) & 4) != 0) * 255, ((y & 2) != 0) * 255 + 0 * x),
    "uvtm": _uvtm,
}
# the quilt's two extra tiles
_TILES = dict(_FORMULAS, ramp=lambda x, y: _grey((x * 255) // 31 + 0 * y), mid=lambda x, y: _grey(np.full_like(x, 128)))
QUILT_W, QUILT_H, QUILT_TILE = 150, 100, 32

NAMES = list(_FORMULAS) + ["quilt"]


def _quilt():
    out = np.zeros((QUILT_H, QUILT_W, 3), np.uint8)
    ly, lx = np.mgrid[0:QUILT_TILE, 0:QUILT_TILE].astype(np.int64)
    tiles = [f(lx, ly) for f in _TILES.values()]
    k = 0
    for ty in range(0, QUILT_H, QUILT_TILE):
        for tx in range(0, QUILT_W, QUILT_TILE):
            t = tiles[k % len(tiles)]
            k += 1
            hh, ww = min(QUILT_TILE, QUILT_H - ty), min(QUILT_TILE, QUILT_W - tx)
            out[ty:ty + hh, tx:tx + ww] = t[:hh, :ww]
    return out


@functools.lru_cache(maxsize=None)
def _frame(name):
    if name == "quilt":
        a = _quilt()
    else:
        y, x = np.mgrid[0:SIZE, 0:SIZE].astype(np.int64)
        a = _FORMULAS[name](x, y)
    a.setflags(write=False)
    return a


def frame(name):
    """(h, w, 3) uint8, read-only (shared between tests)."""
    return _frame(name)


def dims(name):
    h, w, _ = frame(name).shape
    return w, h


ALL_SETTINGS = [(100, 4), (100, 6), (98, 2), (98, 5), (75, 4), (50, 5), (0, 4), (0, 6)]
_BASE = [(100, 4), (100, 6), (75, 4), (0, 4)]
SETTINGS = {n: list(_BASE) for n in NAMES}
SETTINGS["checker1"] = list(ALL_SETTINGS)
SETTINGS["quilt"] = list(ALL_SETTINGS)
SETTINGS["binnoise"] = list(ALL_SETTINGS)
for _n in ("diag45", "diag135", "tm", "uvtm", "sat2"):
    SETTINGS[_n] = _BASE + [(98, 2), (50, 5), (0, 6)]
for _n in ("vstripe1", "hstripe1", "checker16", "sat8"):
    SETTINGS[_n] = _BASE + [(98, 5), (0, 6)]

CASES = [(n, q, m) for n in NAMES for (q, m) in SETTINGS[n]]


@functools.lru_cache(maxsize=None)
def oracle(name, q, m, nparts=1):
    """(vp8 bytes, debug dict) of the oracle's encode, computed once and shared; do not modify."""
    w, h = dims(name)
    rc, vp8, dbg = O.encode(frame(name), w, h, RGB8, q, m, debug=True, nparts=nparts)
    assert rc == 0
    return vp8, dbg


def modes(dbg, nmb, which="p2_info"):
    """(nmb, 18) uint8: luma mode, chroma mode, then the 16 sub-block modes (zero unless luma mode is B)."""
    info = dbg[which]
    m = np.array([[info[i].luma_mode, info[i].chroma_mode] + list(info[i].bpred) for i in range(nmb)], np.uint8)
    m[m[:, 0] != 4, 2:] = 0
    return m
