"""The strip kernel's DECISIONS on the device against the host model (tests/native/strip_decisions_model.cpp; fixture
tests/golden/strip_decisions.json, checked and recomputed on the CPU by tests/test_strip_decisions_cpu.py): which strips met a rational tie,
how many blocks joined a wave's batch of eight, which strips went to the whole-strip exact redo, the largest batch - the four numbers of
tic_last_rare_path_stats, exactly - and the plan tic_last_strip_launch reports, exactly.  The coefficients are compared with the exact
kernel's and the oracle's as everywhere else; they would be right even if every decision were wrong, which is why the counts are pinned.

Every case: tic_set_stats(1), ONE tic_dctq_dev (or tic_dctq_dev_frames), tic_last_rare_path_stats, tic_set_stats(0).  The knobs
(TIC_TUNE=1 TIC_SPLIT=0 TIC_MAX_WGS=64 or 128, TIC_SCHED, TIC_CHUNK=4, TIC_ORDER) make the plan a function of the frame alone.  Also here: the
regression test of the knob latch (a TIC_TUNE set after the first launch of the process used to be ignored)."""
import ctypes as C

import numpy as np
import pytest

import strip_decisions_common as SD
import strip_prologue_common as SP
import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

pytestmark = pytest.mark.gpu
FIXTURE = SD.load_fixture()


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


def expected_zz(oracle, img, q):
    """oracle.encode_zz16; for a non-integral quality the same coefficients from oracle.encode (DC integrated again)."""
    if q == int(q):
        return oracle.encode_zz16(img, int(q))
    dc, ac = oracle.encode(img, float(q))
    return np.concatenate([np.cumsum(dc, dtype=np.int64)[:, None], ac], axis=1).astype(np.int16)


_wanted = {}


def wanted(oracle, case, imgs):
    """The oracle's coefficients of a case's frames: computed once per (frame, quality), shared by the orders and schedules, never written to."""
    key = (repr(sorted(case["frame"].items())), case["quality"])
    if key not in _wanted:
        w = np.stack([expected_zz(oracle, img, case["quality"]) for img in imgs])
        w.setflags(write=False)
        _wanted[key] = w
    return _wanted[key]


def launch_info(ctx):
    info = (C.c_int * 8)()
    ctx.check(N.load().tic_last_strip_launch(ctx.handle, info))
    return list(info)


def rare_path_stats(ctx):
    st = (C.c_ulonglong * 4)()
    ctx.check(N.load().tic_last_rare_path_stats(ctx.handle, st))
    return list(st)


def test_knobs_set_after_the_first_launch_take(ctx, monkeypatch):
    """The latch: with no schedule knob and no TIC_TUNE in the environment, launch once; then set TIC_TUNE=1 TIC_ORDER=0 and launch a frame whose
    grid runs columns first by itself.  The launcher used to keep what the environment held at the first strip launch of the process (TIC_TUNE
    was looked up once): the second launch stayed columns first.  And back: without TIC_TUNE the launcher returns to what it read first."""
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    for k in SD.KNOB_NAMES:
        monkeypatch.delenv(k, raising=False)
    img = SP.frame(7, 512, 512)
    d = SP.Dev(ctx, L, [img], 512)
    try:
        exact = d.run(N.KERNEL_EXACT)
        assert np.array_equal(d.run(N.KERNEL_HYBRID), exact)
        first = launch_info(ctx)
        assert first[0] != SD.ORDER_NONE and first[6:] == [8, 64]
        monkeypatch.setenv("TIC_TUNE", "1")
        assert np.array_equal(d.run(N.KERNEL_HYBRID), exact)
        assert launch_info(ctx)[0] == SD.ORDER_COLS  # 512 strips: resident at once on any device - columns first by grid
        monkeypatch.setenv("TIC_ORDER", "0")
        assert np.array_equal(d.run(N.KERNEL_HYBRID), exact)
        assert launch_info(ctx)[0] == SD.ORDER_ROWS, "TIC_TUNE set after the first launch of the process was ignored"
        monkeypatch.setenv("TIC_MAX_WGS", "64")
        monkeypatch.setenv("TIC_SPLIT", "0")
        assert np.array_equal(d.run(N.KERNEL_HYBRID), exact)
        assert launch_info(ctx) == [SD.ORDER_ROWS, SD.KIND_ROWS, 0, 64, 1, 256, 8, 64]
        monkeypatch.delenv("TIC_TUNE")  # the other knobs still set: not read any more
        assert np.array_equal(d.run(N.KERNEL_HYBRID), exact)
        assert launch_info(ctx) == first
        assert np.array_equal(d.run(N.KERNEL_EXACT), exact)
        assert launch_info(ctx) == [0] * 8  # the exact kernel alone: no strip launch
    finally:
        d.free()


@pytest.mark.parametrize("case", FIXTURE["cases"], ids=SD.case_id)
def test_decisions_are_the_model_s(ctx, oracle, monkeypatch, case):
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    imgs = SD.build_frames(case["frame"])
    want = wanted(oracle, case, imgs)
    for k in SD.KNOB_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in SD.knobs_of(case).items():
        monkeypatch.setenv(k, v)
    q = case["quality"]
    if q != int(q):
        ctx.check(L.tic_set_custom_quality(ctx.handle, float(q)))
    qarg = int(q) if q == int(q) else N.QUALITY_CUSTOM
    d = SP.Dev(ctx, L, imgs, case.get("pitch", imgs[0].shape[1]), case.get("gap", 0))
    if d.nf > 1 and not case.get("gap"):
        d.ostride = d.n * 128  # frames without a gap: coefficients without a gap too (the library then launches one tall frame)
    try:
        exact = d.run(N.KERNEL_EXACT, qarg)
        ctx.check(L.tic_set_stats(ctx.handle, 1))
        try:
            rare_path_stats(ctx)  # (reading resets the counters)
            got = d.run(N.KERNEL_HYBRID, qarg)
            stats = rare_path_stats(ctx)
        finally:
            ctx.check(L.tic_set_stats(ctx.handle, 0))
        info = launch_info(ctx)
    finally:
        d.free()
    print(case["name"], "stats", stats, "model", case["stats"], "plan", info, "model", case["plan"])
    assert info == case["plan"], dict(zip(SD.INFO_FIELDS, zip(info, case["plan"])))
    assert stats == case["stats"], (case["name"], "device", stats, "model", case["stats"])
    assert np.array_equal(exact, want), (case["name"], "exact kernel against the oracle")
    assert np.array_equal(got, want), (case["name"], "strip kernel against the oracle", int((got != want).any(axis=2).sum()), "blocks differ")
