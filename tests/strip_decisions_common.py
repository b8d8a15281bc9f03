"""Cases of the strip kernel's decision tests, shared by the fixture generator (tests/golden/gen/make_goldens_strip_decisions.py), the CPU test
(tests/test_strip_decisions_cpu.py) and the GPU test (tests/test_strip_decisions_gpu.py): the host model's build and driver
(tests/native/strip_decisions_model.cpp), the frames of every case from its JSON record, the knobs a case runs under.

Every GPU case runs with TIC_TUNE=1 TIC_SPLIT=0 TIC_MAX_WGS=<64 or 128> and an explicit TIC_SCHED / TIC_CHUNK / TIC_ORDER: the team schedule off
and the grid capped, the plan (csrc/tic_strip_plan.h) is a function of the frame alone - not of the compute units of the device the test runs on."""
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MODEL_SRC = os.path.join(ROOT, "tests", "native", "strip_decisions_model.cpp")
FIXTURE_JSON = os.path.join(GOLDEN, "strip_decisions.json")
FIXTURE_NPZ = os.path.join(GOLDEN, "strip_decisions.npz")
MUTANTS = ("swap_groups", "lane_xor1", "other_table", "rat_thr_all")
BASE_KNOBS = {"TIC_TUNE": "1", "TIC_SPLIT": "0", "TIC_MAX_WGS": "64", "TIC_SCHED": "0", "TIC_CHUNK": "4"}
KNOB_NAMES = ("TIC_TUNE", "TIC_SPLIT", "TIC_MAX_WGS", "TIC_SCHED", "TIC_CHUNK", "TIC_ORDER")
# what tic_last_strip_launch reports (include/tinyimgcodec_hip.h)
INFO_FIELDS = ("order", "kind", "team_count", "grid_x", "grid_y", "tstep", "fast_tx", "fast_ty")
ORDER_NONE, ORDER_ROWS, ORDER_COLS = 0, 1, 2
KIND_ROWS, KIND_CHUNK, KIND_ROUND = 0, 1, 2

# The planted frame: 64 pixels wide (one strip per row), 520 strips high.  On 64 workgroups (256 waves) the strided walk gives wave 3 the
# strips 3, 259 and 515 - the smallest frame in which a wave walks three strips.  scenario -> ([(strip, number of tripping blocks, tie block?)],
# the four stats the rules of DESIGN.md 5.1 give BY HAND under that walk)
PLANTED_H, PLANTED_W = 4160, 64
WIDE_H, WIDE_W = 512, 32832  # the same strips (3, 259, 515 of the row-by-row numbering) in a frame of 513 strips per row: multi-round, chunked
SCENARIOS = {
    "nothing planted": ([], [0, 0, 0, 0]),
    "one irrational trip": ([(3, 1, False)], [1, 0, 0, 1]),
    "a rational tie only": ([(3, 0, True)], [0, 1, 0, 0]),
    "both in one strip": ([(3, 1, True)], [1, 1, 0, 1]),
    "seven of eight blocks": ([(3, 7, False)], [7, 0, 0, 7]),
    "all eight": ([(3, 8, False)], [0, 0, 1, 0]),
    "4 in strip 3 and 4 in strip 259": ([(3, 4, False), (259, 4, False)], [8, 0, 0, 8]),
    "5 and 5": ([(3, 5, False), (259, 5, False)], [5, 0, 1, 5]),
    "all eight in strip 3, then 3 in strip 259": ([(3, 8, False), (259, 3, False)], [3, 0, 1, 3]),
}


def true_tie_block():
    """A .5 tie of the IRRATIONAL coefficient (2,2) at q = 50 (tests/test_gpu_parity.py _true_tie_block): trips in either pass order, no rational tie."""
    blk = np.full((8, 8), 128, np.int32)
    blk[0, 0] += 64
    blk[0, 1] -= 64
    return blk.astype(np.uint8)


def flat_odd_block():
    """Flat grey 129: the DC sits on a .5 tie at q = 50 (8 / 16), nothing else is non-zero."""
    return np.full((8, 8), 129, np.uint8)


def rand_frame(seed, h, w):
    """conftest.rand_frame (not imported: the generator runs outside pytest)."""
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def planted_frame(h, w, plants):
    """Flat 128 with 8x8 blocks planted: plants = [(strip, slot, block)], strips numbered row by row, w // 64 per row."""
    img = np.full((h, w), 128, np.uint8)
    per_row = w // 64
    for strip, slot, blk in plants:
        y, x = (strip // per_row) * 8, (strip % per_row) * 64 + slot * 8
        img[y:y + 8, x:x + 8] = blk
    return img


def scenario_frame(name, h, w):
    plants = []
    for strip, ntrip, tie in SCENARIOS[name][0]:
        plants += [(strip, s, true_tie_block()) for s in range(ntrip)]
        if tie:
            plants.append((strip, 7, flat_odd_block()))
    return planted_frame(h, w, plants)


_npz = None


def planted_blocks(key):
    global _npz
    if _npz is None:
        _npz = np.load(FIXTURE_NPZ)
    return _npz[key]


def build_frames(frame, blocks=None):
    """A case's frames from its record: a list of equally sized uint8 images (one, except for the multi-frame cases)."""
    kind = frame["kind"]
    if kind == "scenario":
        return [scenario_frame(frame["scenario"], frame["h"], frame["w"])]
    if kind == "noise":
        return [rand_frame(frame["seed"], frame["h"], frame["w"])]
    if kind == "posterised":
        return [(rand_frame(frame["seed"], frame["h"], frame["w"]) // 8 * 8 + 1).astype(np.uint8)]
    if kind == "frames":
        return [rand_frame(s, frame["h"], frame["w"]) for s in frame["seeds"]]
    if kind == "classes":  # one planted block per strip of a 64-wide frame, slot 0
        b = planted_blocks(frame["blocks"]) if blocks is None else blocks
        return [planted_frame(8 * len(b), 64, [(k, 0, b[k]) for k in range(len(b))])]
    if kind == "near_ties":  # the blocks of tests/golden/near_ties.npz, one per strip of a 64-wide frame
        img = np.load(os.path.join(GOLDEN, "near_ties.npz"))["img"].astype(np.uint8)
        b = img.reshape(img.shape[0] // 8, 8, img.shape[1] // 8, 8).swapaxes(1, 2).reshape(-1, 8, 8)
        return [planted_frame(8 * len(b), 64, [(k, 0, b[k]) for k in range(len(b))])]
    raise ValueError(kind)


def raw_bytes(imgs, pitch, fstride):
    """The frames as they lie in device memory: `pitch` bytes per row, `fstride` between frames, padding 0xA5."""
    h, w = imgs[0].shape
    host = np.full((len(imgs) - 1) * fstride + h * pitch, 0xA5, dtype=np.uint8)
    for f, img in enumerate(imgs):
        host[f * fstride: f * fstride + h * pitch].reshape(h, pitch)[:, :w] = img
    return host


def merged_geometry(h, w, pitch, nf, fstride):
    """tic_dctq_dev_frames hands frames that follow each other without a gap and end on a block row to the launcher as ONE tall frame
    (csrc/tic_api.hip merge_frames; the coefficient buffers of the tests are contiguous too).  -> (h, nframes, frame stride) of the launch."""
    if nf > 1 and h % 8 == 0 and fstride == h * pitch and fstride * nf < (1 << 32):
        return h * nf, 1, h * nf * pitch
    return h, nf, fstride


def knobs_of(case):
    k = dict(BASE_KNOBS)
    k.update(case.get("knobs", {}))
    k["TIC_ORDER"] = str(case["order"])
    return k


def build_model(outdir, sanitize=False):
    exe = os.path.join(str(outdir), "strip_decisions_model" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Werror"] + flags + ["-o", exe, MODEL_SRC], check=True)
    return exe


def run_model(exe, raw_path, h, w, pitch, nf, fstride, quality, order, knobs, mutant=None, strips=False):
    """One run of the model on a frame file -> its JSON object."""
    cmd = [exe, "run", "--h", str(h), "--w", str(w), "--stride", str(pitch), "--nframes", str(nf), "--frame-stride", str(fstride), "--quality", repr(float(quality)),
           "--order", str(order), "--max-wgs", knobs["TIC_MAX_WGS"], "--sched", knobs["TIC_SCHED"], "--chunk", knobs["TIC_CHUNK"], "--split", knobs["TIC_SPLIT"],
           "--raw", str(raw_path)]
    if mutant:
        cmd += ["--mutant", mutant]
    if strips:
        cmd.append("--strips")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (cmd, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(r.stdout)


def model_case(exe, tmpdir, case, mutant=None, blocks=None, strips=False, _cache={}):
    """The model's prediction for a case record."""
    imgs = build_frames(case["frame"], blocks)
    h, w = imgs[0].shape
    pitch = case.get("pitch", w)
    nf = len(imgs)
    fstride = h * pitch + case.get("gap", 0)
    key = (json.dumps(case["frame"], sort_keys=True), pitch, fstride, None if blocks is None else blocks.tobytes())
    path = _cache.get(key)
    if path is None or not os.path.exists(path):
        path = os.path.join(str(tmpdir), "frame_%d.raw" % len(_cache))
        raw_bytes(imgs, pitch, fstride).tofile(path)
        _cache[key] = path
    mh, mnf, mfs = merged_geometry(h, w, pitch, nf, fstride)
    return run_model(exe, path, mh, w, pitch, mnf, mfs, case["quality"], case["order"], knobs_of(case), mutant, strips)


def classes_of(exe, tmpdir, blocks, quality, order):
    """The model's view of single blocks: {"beta": [24], "blocks": [{"tie", "trip", "delta": [24], "tripped": [24]}]}, class = 3 * lane + group."""
    path = os.path.join(str(tmpdir), "blocks.raw")
    np.ascontiguousarray(blocks, dtype=np.uint8).tofile(path)
    r = subprocess.run([exe, "classes", "--blocks", path, "--quality", repr(float(quality)), "--order", str(order)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def load_fixture():
    with open(FIXTURE_JSON) as f:
        return json.load(f)


def case_id(case):
    return case["name"]
