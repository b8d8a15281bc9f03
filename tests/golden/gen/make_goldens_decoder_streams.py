#!/usr/bin/env python3
"""Golden fixture for the device decoder's Huffman walk on BUILT coefficients (tests/decoder_streams.py builds the frames): what the
UNMODIFIED reference writes for each frame under each header variant and what it reads back, in the build container (same import recipe
as make_goldens_entropy_blocks.py: stand-ins on the path, the reference imported, only the reference's outputs stored).

    python tests/golden/gen/make_goldens_decoder_streams.py     ->  tests/golden/decoder_streams.json

Streams: compress() with its encode() replaced for the call by a function that returns the built dictionary (as in
make_goldens_entropy_blocks.py); for the scaled variant the header's quality field is the exponent and the flag word is patched to
1 << 30 (codec.py:127-128 reads it; codec.py:102-114 never writes it).  Pixels: decompress() of the first variant's stream, with decode()
wrapped for the call so that the parsed dictionary is kept; the other variants are decode() of that dictionary with their quality and
scaled_dct (the payload is the same) - and, asserted, what decompress() of the whole stream gives for the first variant.  Every stream
must equal the oracle's byte for byte and every pixel array the oracle's.  Stored besides: the census, the visibility figures
(decoder_streams.visibility, bars asserted for the value-bearing frames), and the digest of decode() of every frame of
tests/entropy_blocks.py that has a stream with its own tables (tests/test_entropy_blocks_gpu.py::test_adaptive_kernels: the reference's
own decompress() misreads that flag, so decode() of the dictionary is the expectation).
"""
import json
import os
import struct
import sys
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLD))
sys.path.insert(0, os.path.join(HERE, "standins"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import tinyimgcodec as ref  # noqa: E402  (the unmodified reference)
import tinyimgcodec.codec as ref_codec  # noqa: E402

import decoder_streams as DS  # noqa: E402
import entropy_blocks as EB  # noqa: E402
import inverse_edges as IE  # noqa: E402
from oracle import pyoracle as O  # noqa: E402


def reference_stream(fr, dc, ac, variant):
    flag, q = variant
    built = {"height": fr["h"], "width": fr["w"], "quality": q, "dc": dc, "ac": ac}
    original = ref_codec.encode
    ref_codec.encode = lambda image, quality: {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in built.items()}
    try:
        s = bytearray(ref.compress(None, q))
    finally:
        ref_codec.encode = original
    if flag:
        assert s[12:16] == bytes(4)
        s[12:16] = struct.pack("<I", flag)
    return bytes(s)


def reference_decompress(stream):
    """(pixels, the dictionary decompress() parsed) of the reference."""
    kept = {}
    original = ref_codec.decode

    def keeping(info):
        kept.update(info)
        return original(info)

    ref_codec.decode = keeping
    try:
        px = ref.decompress(stream)
    finally:
        ref_codec.decode = original
    return px, kept


def main():
    t0 = time.perf_counter()
    L = EB.Lengths(O.dump_tables())
    fx = IE.Fixture()
    frames = DS.build_frames(L)
    meta = {"generator": "tests/golden/gen/make_goldens_decoder_streams.py", "frames": {}, "adaptive_pixels": {}}
    for name, fr in frames.items():
        c = DS.census(name, fr, L)
        dc, ac = DS.dc_ac(fr["zz"])
        payload = DS.payload_stream(O, fr)
        info, streams = None, {}
        for variant in fr["variants"]:
            s = reference_stream(fr, dc, ac, variant)
            assert s == DS.with_header(payload, fr, variant) and len(s) == c["stream_bytes"], (name, variant)
            if info is None:
                px, info = reference_decompress(s)
                assert np.array_equal(info["dc"], dc) and np.array_equal(info["ac"], ac), name
                assert np.array_equal(px, ref_codec.decode(dict(info))), name
            else:
                px = ref_codec.decode(dict(info, quality=variant[1], scaled_dct=bool(variant[0])))
            assert px.shape == (fr["h"], fr["w"]) and px.dtype == np.uint8
            assert np.array_equal(px, O.decompress(s)), (name, variant)
            streams[DS.key(variant)] = {"bytes": len(s), "sha256": EB.sha(s), "pixels_sha256": IE.px_sha(px)}
        e = {"family": fr["family"], "h": fr["h"], "w": fr["w"], "coeffs_sha256": EB.sha(np.ascontiguousarray(fr["zz"], dtype="<i4").tobytes()),
             "variants": fr["variants"], "streams": streams, "census": c}
        if fr["zz"][:, 1:].any():
            e["visibility"] = DS.visibility(fx, O, fr)
            if name in DS.VALUE_FRAMES:
                DS.check_bars(name, e["visibility"])
        if name in DS.DC_ONLY:
            e["dc_visibility"] = DS.dc_visibility(fx, O, fr)
        meta["frames"][name] = e
        print("%-24s %6.1f s  %d bytes  %s %s" % (name, time.perf_counter() - t0, c["stream_bytes"], e.get("visibility", ""), e.get("dc_visibility", "")), flush=True)
    with open(EB.FIXTURE) as f:
        eb_fx = json.load(f)["frames"]
    for name, fr in EB.build_frames(L).items():
        if "raises" in eb_fx[name]["adaptive"]:
            continue
        dc, ac = EB.dc_ac(fr["zz"])
        px = ref_codec.decode({"height": fr["h"], "width": fr["w"], "quality": fr["quality"], "scaled_dct": False, "dc": dc, "ac": ac})
        meta["adaptive_pixels"][name] = IE.px_sha(px)
        if name in frames:
            assert meta["frames"][name]["streams"]["q%d" % fr["quality"]]["pixels_sha256"] == meta["adaptive_pixels"][name], name
    with open(DS.FIXTURE, "w") as f:
        json.dump(meta, f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("wrote decoder_streams.json: %d frames, %d bytes, %.0f s" % (len(frames), os.path.getsize(DS.FIXTURE), time.perf_counter() - t0))


if __name__ == "__main__":
    main()
