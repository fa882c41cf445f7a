#!/usr/bin/env python3
"""Generate tests/golden/synth_*.vp8 and tests/golden/decode_synth.json (CPU only).

Key frames written by tests/vp8_synth.py for the header paths no encoder at hand
emits: sharpness, loop-filter deltas, delta-mode segment values and their
clamps, a segment map that is not updated or only partly given, quantiser index
deltas with their floor and cap, an absent skip flag, several token partitions
beside other header blocks, and coefficient probability updates.  Per stream the
manifest keeps the full `params`, the arguments of random_mbs (seeds are fixed:
running this again reproduces every file) and the SHA-256 of the cropped Y, U
and V planes from the system libwebp (WebPDecodeYUV), the independent decoder.
The oracle's decode must give the same digests, or the stream is listed in
ORACLE_PINNED below with the line of the reference's decoder that decides it.

A second family, tests/golden/wide_*.vp8 with tests/golden/decode_wide.json,
holds the coefficients past +-2047 (vp8_synth.wide_mbs: bands wrap, sat, dconly,
cat6).  libwebp differs from the reference there and is not consulted; every
entry is pinned by the oracle.  tests/test_wide_coeffs.py states what the
family must keep holding.

Needs oracle/liboracle.so (make -C oracle) and the system libwebp (`--wide`
writes the second family alone and needs no libwebp).
"""
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "image-webp_amd")]
import oracle_lib as O  # noqa: E402
import vp8_synth as S  # noqa: E402

import numpy as np  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MAX_BYTES = 8192
MAX_ORACLE_PINNED = 3

# Streams on which the reference knowingly departs from libwebp: the oracle's digests, and why.
ORACLE_PINNED = {
    "synth_lfd_first_clamp": "decoder/vp8.rs:1487 clamps the segment's filter level to 0..63 before the ref/mode "
                             "deltas are added (:1489-1496); libwebp clamps once, after them",
}


def seg(update_map=True, update_data=True, absolute=True, quant=(None,) * 4, lf=(None,) * 4, map_probs=(120, 90, 160)):
    return dict(update_map=update_map, update_data=update_data, absolute=absolute, quant=list(quant), lf=list(lf),
                map_probs=list(map_probs))


def lfd(ref0, mode0, update=True):
    # entries 1..3 belong to inter frames; written so that a parser reading the wrong one shows
    return dict(update=update, ref=[ref0, -3, None, 5], mode=[mode0, 7, -2, None])


def random_probs(seed):
    return [int(v) for v in np.random.default_rng(seed).integers(1, 256, S.COEFF_PROBS.size)]


# name, (width, height), header fields that differ from default_params, random_mbs arguments
MAIN = (80, 48)
STREAMS = [
    ("default", MAIN, dict(filter_level=20, skip_prob=128), {}),
    # sharpness 1, 4, 7 x both filters; segment levels that put the interior limit on its floor and on its cap
    ("sharp1_normal", MAIN, dict(filter_level=30, sharpness=1, skip_prob=100,
                                 segments=seg(quant=(20, 40, 60, 90), lf=(1, 2, 40, 63))), {}),
    ("sharp1_simple_p2", MAIN, dict(filter_type=1, filter_level=30, sharpness=1, skip_prob=100, log2_nparts=1,
                                    segments=seg(quant=(20, 40, 60, 90), lf=(1, 2, 40, 63))), {}),
    ("sharp4_normal", MAIN, dict(filter_level=20, sharpness=4, skip_prob=60, yac=50,
                                 segments=seg(absolute=False, quant=(-20, None, 9, 30), lf=(-19, -17, 10, 43))), {}),
    ("sharp4_simple_p4", MAIN, dict(filter_type=1, filter_level=20, sharpness=4, skip_prob=60, yac=50, log2_nparts=2,
                                    segments=seg(absolute=False, quant=(-20, None, 9, 30), lf=(-19, -17, 10, 43))),
     {}),
    ("sharp7_normal_p8", MAIN, dict(filter_level=11, sharpness=7, skip_prob=200, log2_nparts=3,
                                    segments=seg(quant=(35, 35, 70, 12), lf=(3, 8, 20, 63))), {}),
    ("sharp7_simple", MAIN, dict(filter_type=1, filter_level=11, sharpness=7,
                                 segments=seg(quant=(35, 35, 70, 12), lf=(3, 8, 20, 63))), {}),
    # loop-filter deltas: each sign, with and without the update block, against both clamps
    ("lfd_pos", MAIN, dict(filter_level=30, skip_prob=128, lf_delta=lfd(8, 6)), {}),
    ("lfd_neg_simple", MAIN, dict(filter_type=1, filter_level=30, skip_prob=128, lf_delta=lfd(-9, -12)), {}),
    ("lfd_mixed_p2", MAIN, dict(filter_level=10, sharpness=2, skip_prob=128, log2_nparts=1, lf_delta=lfd(20, -25)),
     {}),
    ("lfd_noupdate", MAIN, dict(filter_level=25, skip_prob=128, lf_delta=dict(update=False, ref=[], mode=[])), {}),
    ("lfd_clamp63", MAIN, dict(filter_level=50, skip_prob=128, lf_delta=lfd(10, 5),
                               segments=seg(absolute=False, quant=(None, 5, -5, 10), lf=(10, 13, None, -5))), {}),
    ("lfd_clamp0_simple", MAIN, dict(filter_type=1, filter_level=12, skip_prob=128, lf_delta=lfd(-6, -8),
                                     segments=seg(absolute=False, quant=(None, 5, -5, 10), lf=(-10, -4, None, 5))),
     {}),
    ("lfd_first_clamp", MAIN, dict(filter_level=20, skip_prob=128, lf_delta=lfd(10, -20),
                                   segments=seg(absolute=False, quant=(None, 5, -5, 10), lf=(-30, 50, 55, -25))),
     {}),
    ("level0_abs_seg", MAIN, dict(filter_level=0, skip_prob=128, segments=seg(quant=(30, 50, 70, 90),
                                                                              lf=(None, 30, None, 63))), {}),
    # segment values: delta mode with its clamps at 0 / 63 (filter) and 0 / 127 (quantiser), no filter deltas
    ("seg_delta_clamps", MAIN, dict(filter_level=10, yac=70, skip_prob=128,
                                    segments=seg(absolute=False, quant=(-127, 127, -10, 10), lf=(-20, 60, -3, 7))),
     {}),
    ("seg_nomap", MAIN, dict(filter_level=15, skip_prob=128,
                             segments=seg(update_map=False, quant=(90, 20, 30, 40), lf=(35, 5, 6, 7),
                                          map_probs=(None,) * 3)), {}),
    ("seg_nodata_simple", MAIN, dict(filter_type=1, filter_level=15, skip_prob=128, yac=60,
                                     segments=seg(update_data=False)), dict(density=0.12)),
    ("seg_map1", MAIN, dict(filter_level=18, skip_prob=128,
                            segments=seg(quant=(25, 45, 65, 85), lf=(10, 20, 30, 40), map_probs=(200, None, None))),
     {}),
    ("seg_map2_simple", MAIN, dict(filter_type=1, filter_level=18, skip_prob=128,
                                   segments=seg(quant=(25, 45, 65, 85), lf=(10, 20, 30, 40),
                                                map_probs=(None, 90, 30))), {}),
    # quantiser index deltas: the extremes, the y2ac floor of 8 at base 0, the uvdc cap of 132 from base 120
    ("qd_pos", MAIN, dict(filter_level=20, skip_prob=128, yac=50, ydc_delta=15, y2dc_delta=15, y2ac_delta=15,
                          uvdc_delta=15, uvac_delta=15), {}),
    ("qd_neg_p4", MAIN, dict(filter_level=20, skip_prob=128, yac=50, log2_nparts=2, ydc_delta=-15, y2dc_delta=-15,
                             y2ac_delta=-15, uvdc_delta=-15, uvac_delta=-15), {}),
    ("qd_base0_allprobs", MAIN, dict(filter_level=8, skip_prob=128, yac=0, ydc_delta=-15, y2dc_delta=-3,
                                     y2ac_delta=-15, uvdc_delta=-7, uvac_delta=-15, coeff_probs=random_probs(41)),
     dict(density=0.2)),
    ("qd_cap_simple", MAIN, dict(filter_type=1, filter_level=40, skip_prob=128, yac=120, ydc_delta=15, y2dc_delta=-15,
                                 y2ac_delta=15, uvdc_delta=15, uvac_delta=-8), {}),
    # the skip flag: absent, and present at both ends of its range, under both filters
    ("skip_absent", MAIN, dict(filter_level=28), dict(empty_frac=0.4)),
    ("skip_absent_simple", MAIN, dict(filter_type=1, filter_level=28, sharpness=3), dict(empty_frac=0.4)),
    ("skip_p1_simple", MAIN, dict(filter_type=1, filter_level=33, skip_prob=1), dict(skip_frac=0.5)),
    ("skip_p255", MAIN, dict(filter_level=33, skip_prob=255), dict(skip_frac=0.5)),
    # other shapes: partial MBs on both axes, one MB column, more MB rows than the decoder keeps in flight
    ("33x17", (33, 17), dict(filter_level=22, sharpness=3, skip_prob=90, lf_delta=lfd(-4, 9), ydc_delta=4,
                             uvac_delta=-6, segments=seg(absolute=False, quant=(-8, 8, None, 20),
                                                         lf=(4, -6, None, 12), map_probs=(90, None, 140))), {}),
    ("16x48_simple", (16, 48), dict(filter_type=1, filter_level=26, sharpness=5, skip_prob=70,
                                    lf_delta=lfd(6, -9)), {}),
    ("48x288", (48, 288), dict(filter_level=24, sharpness=2, skip_prob=110, lf_delta=lfd(5, -7), y2ac_delta=-5,
                               segments=seg(quant=(30, 55, 75, 100), lf=(6, 18, 33, 50))), dict(density=0.15)),
    ("48x288_simple_p8", (48, 288), dict(filter_type=1, filter_level=24, sharpness=6, log2_nparts=3,
                                         lf_delta=lfd(-5, 11), uvdc_delta=6,
                                         segments=seg(absolute=False, quant=(-12, None, 14, 40),
                                                      lf=(-9, None, 12, 30), map_probs=(None, None, 77))),
     dict(density=0.15)),
]


# The second family, wide_*: levels by band of |level * dequantiser| beyond
# LEVEL_BUDGET (vp8_synth.wide_mbs).  libwebp is known to differ there, so it is
# not consulted: the oracle pins every one of them.
WIDE_REASON = ("coefficients past +-2047: decoder/vp8.rs:326, :951 keep and dequantise them as i32; the iWHT "
               "(common/transform.rs:82-114), the DC-only shortcut (transform.rs:13-16, chosen at vp8.rs:1110-1117) and "
               "the residue's addition (common/prediction.rs:138-152) are i32; only the full iDCT "
               "(common/transform_simd_intrinsics.rs:478-632) saturates its input to i16 and wraps")
I127 = dict(yac=127)  # all six dequantisers at index 127: 157, 284, 314, 440, 132, 284
DC_FORM = dict(ymode=0, bmodes=[0] * 16, uvmode=0)        # one MB: prediction 128 throughout
BDC_FORM = dict(ymode=4, bmodes=[0] * 16, uvmode=0)       # one MB: B_DC sub-blocks under 127 above, 129 left
WIDE = [
    # 80 x 48: per band no filter / the normal filter at 30 or more / the simple filter
    ("wrap_lf0", MAIN, dict(yac=60, skip_prob=128), dict(band="wrap")),
    # (segment quantisers 87, 113, 57, 27: yac 128, 217, 64, 31 give products of exactly -32768 and +-32767)
    ("wrap_normal_seg", MAIN, dict(filter_level=32, sharpness=2, skip_prob=100,
                                   segments=seg(quant=(87, 113, 57, 27), lf=(30, 40, 50, 63))), dict(band="wrap")),
    ("wrap_simple_p4", MAIN, dict(filter_type=1, filter_level=35, yac=90, log2_nparts=2, ydc_delta=-6, uvac_delta=9),
     dict(band="wrap")),
    ("sat_lf0", MAIN, dict(skip_prob=128, **I127), dict(band="sat")),
    ("sat_normal", MAIN, dict(filter_level=40, sharpness=1, **I127), dict(band="sat")),
    ("sat_simple_seg", MAIN, dict(filter_type=1, filter_level=30, skip_prob=90, ydc_delta=-2,
                                  segments=seg(quant=(127, 113, 87, 57), lf=(20, 30, 45, 63))), dict(band="sat")),
    ("dconly_lf0", MAIN, I127, dict(band="dconly", hand=[[0, 0], [7, 1], [14, 2]])),
    ("dconly_normal", MAIN, dict(filter_level=45, skip_prob=128, **I127), dict(band="dconly")),
    ("dconly_simple_seg", MAIN, dict(filter_type=1, filter_level=30, skip_prob=128,
                                     segments=seg(quant=(127, 110, 90, 70), lf=(10, 25, 40, 63))), dict(band="dconly")),
    ("cat6_lf0", MAIN, dict(yac=0, skip_prob=128), dict(band="cat6")),
    ("cat6_normal", MAIN, dict(filter_level=30, yac=10, y2dc_delta=5, y2ac_delta=-10, uvdc_delta=10, uvac_delta=-5),
     dict(band="cat6")),
    ("cat6_simple_seg_p4", MAIN, dict(filter_type=1, filter_level=33, skip_prob=128, log2_nparts=2,
                                      segments=seg(quant=(0, 5, 12, 20), lf=(15, 30, 45, 60))), dict(band="cat6")),
    # partial MBs; the hand-built Y2 MBs through the device token parse (two columns, one partition)
    ("sat_37x21", (37, 21), dict(filter_level=36, sharpness=3, skip_prob=128, uvdc_delta=-4,
                                 segments=seg(quant=(127, 115, 125, 80), lf=(30, 36, 50, 63))), dict(band="sat")),
    ("hand_32x16", (32, 16), I127, dict(band="dconly", hand=[[0, 0], [1, 1]])),
]
# 16 x 16, one MB, no filter: the three hand-built MBs, then band x form x quantiser index
WIDE += [(f"mb_hand{n}", (16, 16), I127, dict(band="dconly", hand=[[0, n]])) for n in range(3)]
MB_YAC = dict(wrap=(30, 50, 70, 87, 113, 127), sat=(127, 125, 115, 100, 80, 60), dconly=(127, 127, 120, 110, 100, 90),
              cat6=(0, 4, 8, 12, 16, 20))
WIDE += [(f"mb_{band}_{fname}{i}", (16, 16), dict(yac=yac), dict(band=band, force=form, density=0.4))
         for band in S.WIDE_BANDS for fname, form in (("dc", DC_FORM), ("bdc", BDC_FORM))
         for i, yac in enumerate(MB_YAC[band])]


def build(name, size, fields, gen, seed):
    params = S.default_params(*size)
    assert set(fields) <= set(params), name
    params.update(copy.deepcopy(fields))
    gen = dict(seed=seed, **gen)
    mbs = S.wide_mbs(params, **gen) if "band" in gen else S.random_mbs(params, **gen)
    return params, gen, S.write_keyframe(params, mbs)


def main_wide():
    entries = []
    for k, (name, size, fields, gen) in enumerate(WIDE):
        name = "wide_" + name
        params, gen, vp8 = build(name, size, fields, gen, 0x51DE0000 + k)
        assert len(vp8) <= MAX_BYTES, (name, len(vp8))
        rc, r = O.decode(vp8)
        assert rc == 0, (name, rc)
        mbw = r["mbw"]
        digests = S.plane_digests(r["y"], r["u"], r["v"], size[0], size[1], mbw * 16, mbw * 8)
        with open(os.path.join(OUT, name + ".vp8"), "wb") as f:
            f.write(vp8)
        entries.append(dict(name=name, width=size[0], height=size[1], params=params, gen=gen, yuv_sha256=digests,
                            pinned_by="oracle", reason=WIDE_REASON))
        print(f"{name}: {len(vp8)} bytes")
    with open(os.path.join(OUT, "decode_wide.json"), "w") as f:
        json.dump({"generator": "tools/make_synth_golden.py", "streams": entries}, f, indent=1)
        f.write("\n")
    print("wrote", len(entries), "wide streams")


def main():
    os.makedirs(OUT, exist_ok=True)
    entries, rejected = [], []
    for k, (name, size, fields, gen) in enumerate(STREAMS):
        name = "synth_" + name
        params, gen, vp8 = build(name, size, fields, gen, 0x5EED5000 + k)
        assert len(vp8) <= MAX_BYTES, (name, len(vp8))
        rc, r = O.decode(vp8)
        assert rc == 0, (name, rc)
        mbw = r["mbw"]
        ours = S.plane_digests(r["y"], r["u"], r["v"], size[0], size[1], mbw * 16, mbw * 8)
        theirs = S.libwebp_yuv_digests(vp8)
        entry = dict(name=name, width=size[0], height=size[1], params=params, gen=gen)
        if name in ORACLE_PINNED:
            assert theirs != ours, f"{name}: libwebp agrees after all; pin it on libwebp"
            entry.update(yuv_sha256=ours, pinned_by="oracle", reason=ORACLE_PINNED[name])
        elif theirs is None:
            rejected.append(name)
            continue
        else:
            assert theirs == ours, f"{name}: the oracle and libwebp differ: {ours} {theirs}"
            entry.update(yuv_sha256=theirs, pinned_by="libwebp")
        with open(os.path.join(OUT, name + ".vp8"), "wb") as f:
            f.write(vp8)
        entries.append(entry)
        print(f"{name}: {len(vp8)} bytes, pinned by {entry['pinned_by']}")
    assert not rejected, f"libwebp rejects {rejected}"
    assert sum(e["pinned_by"] == "oracle" for e in entries) <= MAX_ORACLE_PINNED
    with open(os.path.join(OUT, "decode_synth.json"), "w") as f:
        json.dump({"generator": "tools/make_synth_golden.py", "streams": entries}, f, indent=1)
        f.write("\n")
    print("wrote", len(entries), "streams")


if __name__ == "__main__":
    if "--wide" not in sys.argv[1:]:  # --wide: the second family alone (needs no libwebp)
        main()
    main_wide()
