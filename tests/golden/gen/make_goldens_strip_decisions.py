"""Writes tests/golden/strip_decisions.json and strip_decisions.npz: the cases of the strip kernel's decision tests with the counts and plans
the host model (tests/native/strip_decisions_model.cpp) predicts for them, and the planted blocks of the class frames, found by the model's
own seeded search.  Needs no GPU and nothing outside the repository:  python tests/golden/gen/make_goldens_strip_decisions.py

tests/test_strip_decisions_cpu.py recomputes every number written here, so the fixture cannot go stale against tic_math.h / tic_strip_plan.h."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import strip_decisions_common as SD  # noqa: E402

SEARCH_QUALITIES = (50, 90, 1, 37.5)  # class frames from the seeded random search (37.5: through tic_set_custom_quality)
SEARCH_TRIES = 4000000


def search(exe, q, order):
    r = subprocess.run([exe, "search", "--quality", repr(float(q)), "--order", str(order), "--seed", "20261", "--tries", str(SEARCH_TRIES)], capture_output=True, text=True,
                       check=True)
    return json.loads(r.stdout)


def tuned_rational_quality(exe, tmp, blk, cls, q_lo, q_hi):
    """The rational coefficients' quotients are multiples of 1 / (8 div): at an integer quality they sit ON a tie or far from it, and no
    random search comes within two bands.  For a block whose only energy is one rational coefficient the quotient grows with the quality:
    bisect the quality at which the distance to the tie is 1.5 bands (just accepted) in both pass orders.  q_lo: accepted and far,
    q_hi: on the tie side (tripped)."""
    def ratio(q, order):
        c = SD.classes_of(exe, tmp, blk[None], q, order)
        return c["blocks"][0]["delta"][cls] / c["beta"][cls]
    lo, hi = q_lo, q_hi
    assert ratio(lo, 1) > 2.0 and ratio(hi, 1) < 1.0, (ratio(lo, 1), ratio(hi, 1))
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        r = ratio(mid, 1)
        if 1.3 <= r <= 1.7:
            break
        if r > 1.7:
            lo = mid
        else:
            hi = mid
    for order in (0, 1):
        assert 1.0 <= ratio(mid, order) < 2.0, (mid, order, ratio(mid, order))
    return mid


def main():
    tmp = tempfile.mkdtemp()
    exe = SD.build_model(tmp)
    npz, class_frames = {}, []
    for q in SEARCH_QUALITIES:
        for order in (0, 1):
            s = search(exe, q, order)
            blocks = [np.array(e["px"], np.uint8).reshape(8, 8) for e in s["tripped"]] + [np.array(e["px"], np.uint8).reshape(8, 8) for e in s["accepted"]]
            key = "classes_q%s_o%d" % (str(q).replace(".", "p"), order)
            npz[key] = np.stack(blocks)
            class_frames.append({"blocks": key, "quality": q, "order": order, "tripped": [e["class"] for e in s["tripped"]],
                                 "accepted": [e["class"] for e in s["accepted"]]})
    # just-accepted blocks of the rational classes (lane 0 and lane 4, group {0,4}: classes 2 and 14), each at a quality tuned for it
    s4 = np.array([1, -1, -1, 1, 1, -1, -1, 1])
    only_dc = np.full((8, 8), 131, np.uint8)                                  # DC = 24: a tie at q = 16.67 (divisor 48)
    only_44 = (128 + 20 * np.outer(s4, s4)).astype(np.uint8)                  # (4,4) alone
    for name, blk, cls, q_lo, q_hi in (("dc", only_dc, 2, 16.0, 50.0 / 3.0), ("c44", only_44, 14, None, None)):
        if q_lo is None:  # (4,4) = 160 in coefficient units; its divisor is 68 * 50 / q below q = 50: a tie where 160 q / 3400 = k + 0.5
            q_hi = 0.5 * 3400.0 / 160.0 * 3  # k = 1: q = 31.875
            q_lo = q_hi - 0.5
        q = tuned_rational_quality(exe, tmp, blk, cls, q_lo, q_hi)
        for order in (0, 1):
            key = "classes_%s_o%d" % (name, order)
            npz[key] = blk[None]
            class_frames.append({"blocks": key, "quality": q, "order": order, "tripped": [], "accepted": [cls]})

    def case(name, frame, quality, order, **kw):
        c = {"name": "%s, q = %s, %s" % (name, quality, "columns first" if order else "rows first"), "frame": frame, "quality": quality, "order": order}
        c.update(kw)
        return c

    cases = []
    for order in (1, 0):
        for sc, (_, hand) in SD.SCENARIOS.items():
            fr = {"kind": "scenario", "scenario": sc, "h": SD.PLANTED_H, "w": SD.PLANTED_W}
            cases.append(case("planted: " + sc, fr, 50, order, hand=hand))
            cases.append(case("planted on 128 workgroups: " + sc, fr, 50, order, knobs={"TIC_MAX_WGS": "128"}))
            cases.append(case("planted, chunked walk of a wide frame: " + sc, {"kind": "scenario", "scenario": sc, "h": SD.WIDE_H, "w": SD.WIDE_W}, 50, order,
                              knobs={"TIC_SCHED": "1"}))
        for cf in class_frames:
            if cf["order"] == order:
                cases.append(case("class frame %s" % cf["blocks"], {"kind": "classes", "blocks": cf["blocks"]}, cf["quality"], order, mutants=True))
        cases.append(case("near_ties blocks, one per strip", {"kind": "near_ties"}, 50, order, mutants=True))
        for sched in ("0", "1"):
            for q in (50, 90, 99):
                cases.append(case("noise 1024 x 2048, TIC_SCHED=" + sched, {"kind": "noise", "seed": 2001, "h": 1024, "w": 2048}, q, order, knobs={"TIC_SCHED": sched},
                                  mutants=sched == "0"))
            for q in (50, 99):
                cases.append(case("posterised noise 1024 x 2048, TIC_SCHED=" + sched, {"kind": "posterised", "seed": 2002, "h": 1024, "w": 2048}, q, order,
                                  knobs={"TIC_SCHED": sched}, mutants=sched == "0"))
        # (1024 x 2048 is 4096 strips: at the cap of 64 workgroups exactly NOT larger than the chip - TIC_SCHED=1 leaves it strided.  Eight rows more are.)
        cases.append(case("noise 1032 x 2048 (chunked)", {"kind": "noise", "seed": 2003, "h": 1032, "w": 2048}, 90, order, knobs={"TIC_SCHED": "1"}))
        cases.append(case("ragged 200 x 333, pitch 336", {"kind": "noise", "seed": 2004, "h": 200, "w": 333}, 90, order, pitch=336))
        cases.append(case("ragged 200 x 333, pitch 333 (no strip launch)", {"kind": "noise", "seed": 2004, "h": 200, "w": 333}, 90, order, pitch=333))
        cases.append(case("3 frames of 256 x 512 (one tall frame)", {"kind": "frames", "seeds": [2005, 2006, 2007], "h": 256, "w": 512}, 90, order))
        cases.append(case("3 frames of 256 x 512, 4 KiB between them (grid planes)", {"kind": "frames", "seeds": [2005, 2006, 2007], "h": 256, "w": 512}, 90, order, gap=4096))
    SD._npz = npz  # (the cases' planted blocks: not yet on disk)
    for c in cases:
        m = SD.model_case(exe, tmp, c)
        c["stats"], c["plan"] = m["stats"], m["plan"]
        if c.pop("mutants", False):
            c["mutants"] = {mu: SD.model_case(exe, tmp, c, mutant=mu)["stats"] for mu in SD.MUTANTS}
        print(c["name"], c["stats"], c["plan"], c.get("hand", ""))

    # rational-tie strips of the config-2 frame (stats[1]: a property of the frame, the quality and the pass order - not of the schedule)
    config2 = {}
    raw = os.path.join(tmp, "config2.raw")
    SD.rand_frame(1234, 4096, 4096).tofile(raw)
    knobs = dict(SD.BASE_KNOBS)
    for q in (10, 50, 90):
        config2[str(q)] = {str(order): SD.run_model(exe, raw, 4096, 4096, 4096, 1, 4096 * 4096, q, order, knobs)["stats"][1] for order in (0, 1)}
    # the trip rates DESIGN.md section 3 quotes, modelled on the 1024 x 2048 noise frame (columns first)
    rates = {}
    raw = os.path.join(tmp, "rates.raw")
    SD.rand_frame(2001, 1024, 2048).tofile(raw)
    for q in (50, 90):
        m = SD.run_model(exe, raw, 1024, 2048, 2048, 1, 1024 * 2048, q, 1, knobs)
        rates[str(q)] = {k: m[k] for k in ("blocks", "trip_blocks", "trip_strips", "fast_strips")}
        rates[str(q)]["tie_strips"] = m["stats"][1]
    with open(SD.FIXTURE_JSON, "w") as f:
        json.dump({"base_knobs": SD.BASE_KNOBS, "info_fields": SD.INFO_FIELDS, "class_frames": class_frames, "cases": cases, "config2_tie_strips": config2,
                   "modelled_rates_noise_1024x2048": rates}, f, indent=1)
        f.write("\n")
    np.savez_compressed(SD.FIXTURE_NPZ, **npz)
    print("wrote", len(cases), "cases,", sum(len(v) for v in npz.values()), "planted blocks")


if __name__ == "__main__":
    main()
