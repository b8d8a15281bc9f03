#!/usr/bin/env python3
"""Fixture for encode() / compress() of integer images outside 0..255 (tests/test_wide_blocks_cpu.py / _gpu.py): the frames of
tests/wide_blocks.py (its docstring names the families) and what the UNMODIFIED REFERENCE makes of every one of them - encode()'s dc / ac,
and for the `streams` family compress()'s bytes or the name of its exception, and decompress()'s pixels.  Stand-ins for the two absent
pure-container packages as in the other generators; no arithmetic of the codec is restated here.

    python tests/golden/gen/make_goldens_wide_blocks.py

RuntimeWarning is an error while the reference runs: a rounded quotient that leaves int32 is numpy's invalid cast (a warning, and
INT32_MIN for either sign where this was tried), which is outside the contract of tic_encode_wide, so such a frame cannot get into the
fixture.

wide_blocks.npz: <frame>_dc int32 [N], <frame>_ac int32 [N, 63]; <frame>_bs, <frame>_dec for the streams the reference wrote; <frame>_pix
for wide_blocks.DECODE_FRAMES: the reference's decode() of its own dictionary (scaled_dct = False).  wide_blocks.json: per frame its family,
size, quality and the sha256 of its int32 pixels (the builder rebuilds them), and a census per family."""
import json
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "standins"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(GOLD))

import numpy as np  # noqa: E402

import tinyimgcodec as ref  # noqa: E402  (the unmodified reference)

import wide_blocks as WB  # noqa: E402


def dump(doc):
    """The manifest as text, a line per frame and per census entry, so that a change shows as the lines it changes."""
    def one(x):
        return json.dumps(x, sort_keys=True)

    frames = ",\n".join("  %s: %s" % (one(k), one(v)) for k, v in doc["frames"].items())
    census = ",\n".join("  %s: %s" % (one(k), one(v)) for k, v in doc["census"].items())
    return "{\n \"census\": {\n%s\n },\n \"frames\": {\n%s\n },\n \"generator\": %s\n}\n" % (census, frames, one(doc["generator"]))


def main():
    warnings.simplefilter("error", RuntimeWarning)
    out, doc = {}, {"generator": "tests/golden/gen/make_goldens_wide_blocks.py", "frames": {}, "census": {}}
    census = {fam: {"frames": 0, "blocks": 0, "max_abs_ac": 0, "max_abs_dc_diff": 0} for fam in WB.FAMILIES}
    for f in WB.build_frames():
        assert f.img.dtype == np.int32
        info = ref.encode(f.img, f.quality)
        dc, ac = info["dc"], info["ac"]
        assert dc.dtype == np.int32 and ac.dtype == np.int32
        out[f.name + "_dc"], out[f.name + "_ac"] = np.ascontiguousarray(dc), np.ascontiguousarray(ac)  # (ac comes out of the reference F-ordered)
        h, w = f.img.shape
        entry = {"family": f.family, "h": h, "w": w, "quality": f.quality, "sha256": WB.sha(f.img)}
        c = census[f.family]
        c["frames"] += 1
        c["blocks"] += len(dc)
        c["max_abs_ac"] = max(c["max_abs_ac"], int(np.abs(ac.astype(np.int64)).max()))
        c["max_abs_dc_diff"] = max(c["max_abs_dc_diff"], int(np.abs(dc.astype(np.int64)).max()))
        if f.family == "streams":
            try:
                bs = ref.compress(f.img, f.quality)
                dec = ref.decompress(bs)
                assert dec.shape == f.img.shape and dec.dtype == np.uint8
                out[f.name + "_bs"], out[f.name + "_dec"] = np.frombuffer(bs, np.uint8), dec
                entry["stream"] = "bytes"
                what = "%d bytes" % len(bs)
            except KeyError as e:
                entry["stream"] = type(e).__name__
                what = entry["stream"]
            c.setdefault("streams", {})[f.name] = {"result": what, "max_abs_running_dc": int(np.abs(np.cumsum(dc.astype(np.int64))).max()),
                                                   "max_abs_dc_diff": int(np.abs(dc).max()), "max_abs_ac": int(np.abs(ac).max())}
        if f.name in WB.DECODE_FRAMES:
            d = dict(info, scaled_dct=False)
            out[f.name + "_pix"] = ref.decode(d)
        if f.family == "extremes":
            c["pixels_that_wrap"] = c.get("pixels_that_wrap", 0) + int((f.img.astype(np.int64) - 128 < WB.I32_MIN).sum())
            if f.name == WB.PAIR_FRAME:
                c["pair_dc"] = [int(x) for x in dc]
            if f.name == "ext_flat_min_q10":
                c["flat_min_q10_dc0"] = int(dc[0])
        if f.family == "ties":
            u, v = int(f.name[4]), int(f.name[5])
            twice = WB.tie_exact_twice(u, v, f.img)
            assert (twice % 2 != 0).all()
            k = int(np.flatnonzero(WB.ZIGZAG == u * 8 + v)[0])
            got = np.cumsum(dc.astype(np.int64)) if k == 0 else ac[:, k - 1].astype(np.int64)
            up = 2 * got > twice
            assert (np.abs(2 * got - twice) == 1).all()
            half_even = np.where(((twice - 1) // 2) % 2 == 0, (twice - 1) // 2, (twice + 1) // 2)
            c["%d%d" % (u, v)] = {"up": int(up.sum()), "down": int((~up).sum()), "unlike_half_even": int((got != half_even).sum())}
        doc["frames"][f.name] = entry
        print("%-28s %-9s %3d x %-3d q=%-5g blocks=%-4d max|AC|=%-10d max|dDC|=%d" % (f.name, f.family, h, w, f.quality, len(dc),
                                                                                     int(np.abs(ac.astype(np.int64)).max()), int(np.abs(dc.astype(np.int64)).max())))
    doc["census"] = census
    np.savez_compressed(os.path.join(GOLD, "wide_blocks.npz"), **out)
    text = dump(doc)
    assert json.loads(text) == doc
    with open(os.path.join(GOLD, "wide_blocks.json"), "w") as fo:
        fo.write(text)
    size = os.path.getsize(os.path.join(GOLD, "wide_blocks.npz")) + os.path.getsize(os.path.join(GOLD, "wide_blocks.json"))
    print(json.dumps(census, indent=1, sort_keys=True))
    print("wrote wide_blocks.npz + wide_blocks.json: %d bytes" % size)


if __name__ == "__main__":
    main()
