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

Needs oracle/liboracle.so (make -C oracle) and the system libwebp.
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


def build(name, size, fields, gen, seed):
    params = S.default_params(*size)
    assert set(fields) <= set(params), name
    params.update(copy.deepcopy(fields))
    gen = dict(seed=seed, **gen)
    return params, gen, S.write_keyframe(params, S.random_mbs(params, **gen))


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
    main()
