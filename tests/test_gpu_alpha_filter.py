"""The alpha filter kernels (csrc/zw_alpha_kernels.hip) through zw_alph_decode:
raw-compression ALPH payloads built here with the forward filter in numpy, for
each of the four filtering methods, decoded on the device and compared bit for
bit with the numpy restatement of get_alpha_predictor (tests/alpha_ref.py).

Planes (alpha_ref.test_planes): noise, whose running sums wrap mod 256 many
times per row and column; a stepped ramp and 0 / 255 blocks, on which the
gradient rule's L + T - TL leaves [0, 255] on both sides (asserted below).

Sizes (width x height): 1x1 one pixel, 1x70 one column over a band edge, 70x1
one row over the 64-lane edge, 33x17, 65x65 (one past the band and the lane
edge), 130x67 (a third 64-lane step of a row, a second band), 257x3 wide and
short; then the sizes at which the kernels take another path: 64x5 and 516x66
(w % 4 == 0: the vertical filter's word columns and word-aligned rows; 516: a
second LDS tile of the gradient kernel, 4 columns wide) and 1030x3 (three
tiles, rows that start at every byte phase)."""
import numpy as np
import pytest

import alpha_ref as R
import zwebp

SIZES = [(1, 1), (1, 70), (70, 1), (33, 17), (65, 65), (130, 67), (257, 3), (64, 5), (516, 66), (1030, 3)]


@pytest.fixture(scope="module")
def ctx():
    c = zwebp.Context(0)
    yield c
    c.close()


def test_planes_hit_both_clamps():
    """The inputs do what the docstring says (no GPU needed, but it guards the GPU cases' meaning)."""
    for w, h in ((33, 17), (130, 67)):
        for name in ("steps", "blocks"):
            p = R.test_planes(w, h, w * 1000 + h)[name].astype(np.int32)
            g = p[1:, :-1] + p[:-1, 1:] - p[:-1, :-1]
            assert (g < 0).any() and (g > 255).any(), (w, h, name)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_gpu_alpha_filters(ctx, w, h):
    planes = R.test_planes(w, h, w * 1000 + h)
    for name, plane in planes.items():
        for filt in range(4):
            payload = R.raw_alph(plane, filt)
            residual = np.frombuffer(payload[1:], np.uint8).reshape(h, w)
            want = R.unfilter(residual, filt)
            assert np.array_equal(want, plane)  # (the checker's two halves)
            got = zwebp.alph_decode(payload, w, h, ctx=ctx)
            assert got.shape == (h, w) and got.dtype == np.uint8
            bad = np.argwhere(got != want)
            assert bad.size == 0, (name, filt, "first differing (y, x):", bad[:4].tolist())


@pytest.mark.gpu
def test_gpu_alph_decode_errors(ctx):
    body = bytes(15)
    for payload, code in ((b"", 15), (bytes([0x20]) + body, 23), (bytes([0x02]) + body, 24), (bytes([0x04]) + body[:-1], 15)):
        with pytest.raises(zwebp.DecodingError) as e:
            zwebp.alph_decode(payload, 5, 3, ctx=ctx)
        assert e.value.code == code
