#!/usr/bin/env python3
"""Fixture for the integer encoder's arithmetic (tests/test_scaled_blocks_cpu.py / _gpu.py): the built pixel blocks of tests/scaled_blocks.py
(its docstring names the families and the search) in frames 72 pixels wide, and what the UNMODIFIED REFERENCE makes of every frame at the
four settings - the stream make_goldens_scaled_enc.py defines and obtains (reference_case: the C program compiled into
oracle/_ref/ref_c_encode, read back with the reference's own bit reader), the coefficients of that walk, and the reference's decompress()
of the stream.  No arithmetic of the encoder is restated here.

    make -C oracle ref && python tests/golden/gen/make_goldens_scaled_blocks.py

Frame `nocode_0` holds the blocks with an |AC| above 1023 at `best` (the two (1, 1) peaks and the +-1024 blocks): there the C encoder
indexes past its code table and the reference has no defined output (reference_case refuses such a frame), so it is not run.  For that frame at `best` - and for it
alone - the coefficients are the model's (tests/scaled_blocks.py: model), marked "pinned_by": "model", and there is no stream; at the other
three settings it is pinned on the reference like every other frame.  The model is compared with the reference's coefficients for
everything else here as well, so a fixture is never written from a model the reference contradicts.

scaled_blocks.npz: <frame>_img, <frame>_<setting>_zz (int16 [N, 64]), <frame>_<setting>_bs.  scaled_blocks.json: "info" (the 8 x 8 peak
tables of both polarities, the row pass's maxima, the table words no reachable value separates, block counts) and per frame its family,
size, number of built blocks (flat-128 fillers behind them), a note per built block (position, d in front of the quantiser, and for a
`word` block the single-word mutants it was built to expose) and per setting payload bits, length, sha256 of stream, coefficients and
decoded pixels."""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(GOLD))

import numpy as np  # noqa: E402

import scaled_blocks as S  # noqa: E402
from make_goldens_scaled_enc import ref, reference_case, sha  # noqa: E402


def dump(doc):
    """The manifest as text: a line per info entry, per block note and per setting of a frame, so that a change shows as the lines it changes."""
    def one(x):
        return json.dumps(x, sort_keys=True)

    def members(d, indent, fmt=one):
        return ",\n".join("%s%s: %s" % (indent, one(k), fmt(d[k])) for k in sorted(d))

    def frame(e):
        rest = {k: v for k, v in e.items() if k not in ("notes", "settings")}
        notes = "[\n" + ",\n".join("    " + one(n) for n in e["notes"]) + "\n   ]"
        return "{\n%s,\n   \"notes\": %s,\n   \"settings\": {\n%s\n   }\n  }" % (members(rest, "   "), notes, members(e["settings"], "    "))

    return "{\n \"frames\": {\n%s\n },\n \"generator\": %s,\n \"info\": {\n%s\n }\n}\n" % (members(doc["frames"], "  ", frame), one(doc["generator"]), members(doc["info"], "  "))


def main():
    families, notes, info = S.build_corpus(log=print)
    frames = S.arrange(families, notes)
    info["blocks"] = {fam: int(len(b)) for fam, b in families.items()}
    out, doc = {}, {"generator": "tests/golden/gen/make_goldens_scaled_blocks.py", "info": info, "frames": {}}
    for name, family, img, frame_notes in frames:
        h, w = img.shape
        out[name + "_img"] = img
        entry = {"family": family, "h": h, "w": w, "blocks": len(frame_notes), "notes": frame_notes, "settings": {}}
        for qf, setting in enumerate(S.SETTINGS):
            want = S.model(S.frame_blocks(img), qf).astype(np.int16)
            if family == "nocode" and setting == "best":
                # (not run through the reference: what the program writes past its table need not even walk as a stream)
                assert all(np.abs(z[1:]).max() > 1023 for z in want[: len(frame_notes)])
                out["%s_%s_zz" % (name, setting)] = want
                entry["settings"][setting] = {"pinned_by": "model", "zz_sha256": sha(want), "max_abs_ac": int(np.abs(want[:, 1:]).max())}
                print("%-12s %-5s model-pinned, max|AC|=%d" % (name, setting, entry["settings"][setting]["max_abs_ac"]))
                continue
            stream, zz, P, zrl, last63 = reference_case(img, setting, True)
            assert np.array_equal(zz, want), "%s %s: the model differs from the reference in %d coefficients" % (name, setting, int((zz != want).sum()))
            dec = ref.decompress(stream)
            assert dec.shape == img.shape
            out["%s_%s_zz" % (name, setting)] = zz
            out["%s_%s_bs" % (name, setting)] = np.frombuffer(stream, np.uint8)
            entry["settings"][setting] = {"pinned_by": "reference", "payload_bits": int(P), "bytes": len(stream), "sha256": sha(np.frombuffer(stream, np.uint8)),
                                          "zz_sha256": sha(zz), "dec_sha256": sha(dec), "max_abs_ac": int(np.abs(zz[:, 1:]).max()),
                                          "max_abs_dc_diff": int(np.abs(np.diff(zz[:, 0].astype(np.int64), prepend=0)).max())}
            print("%-12s %-5s P=%-7d %6d bytes  max|AC|=%-5d max|dDC|=%d" % (name, setting, P, len(stream), entry["settings"][setting]["max_abs_ac"],
                                                                             entry["settings"][setting]["max_abs_dc_diff"]))
        doc["frames"][name] = entry
    np.savez_compressed(os.path.join(GOLD, "scaled_blocks.npz"), **out)
    text = dump(doc)
    assert json.loads(text) == doc
    with open(os.path.join(GOLD, "scaled_blocks.json"), "w") as f:
        f.write(text)
    print("wrote scaled_blocks.npz, scaled_blocks.json: %s" % info["blocks"])


if __name__ == "__main__":
    main()
