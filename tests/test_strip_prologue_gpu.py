"""The strip kernel's start - preloaded schedule words, the host-planned cursor (csrc/tic_strip_plan.h), pixel loads ahead of every scalar wait -
on the frames that reach its branches (tests/strip_prologue_common.py; the same list is walked on the CPU by tests/native/strip_plan_selftest.cpp):
the shipped library in a fresh process, and the test-hooks build under both pass orders and the forced schedules.  Everywhere the strip kernel
is compared with the exact kernel and with the oracle, coefficient for coefficient."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import strip_prologue_common as SP
import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB_NAMES = ("TIC_SPLIT", "TIC_SCHED", "TIC_CHUNK", "TIC_MAX_WGS", "TIC_ORDER")
# forced schedules (csrc/tic_hooks.h).  A persistent grid capped at 64 workgroups makes 2048x1536 "larger than the chip" (chunked under
# TIC_SCHED=1, round-interleaved under 2, strided under 0) and leaves 512x512 strided under all three; capped at 16, 1920x1080 is too.
KNOBS = [
    {},
    {"TIC_SPLIT": "0"},
    {"TIC_SPLIT": "1,1,1,1,1,1"},
    {"TIC_MAX_WGS": "64", "TIC_SCHED": "0"},
    {"TIC_MAX_WGS": "64", "TIC_SCHED": "1"},
    {"TIC_MAX_WGS": "64", "TIC_SCHED": "2"},
    {"TIC_MAX_WGS": "16", "TIC_SCHED": "1", "TIC_CHUNK": "3"},
    {"TIC_MAX_WGS": "16", "TIC_SCHED": "2", "TIC_CHUNK": "3"},
    {"TIC_MAX_WGS": "2048"},
]


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(ctx, oracle):
    """Every frame on the device, with the oracle's coefficients and the exact kernel's (computed once, compared here)."""
    L = N.load()
    out = []
    for name, imgs, pitch, gap in SP.all_cases():
        d = SP.Dev(ctx, L, imgs, pitch, gap)
        want = np.stack([oracle.encode_zz16(img, SP.QUALITY) for img in imgs])
        exact = d.run(N.KERNEL_EXACT)
        assert np.array_equal(exact, want), (name, "exact kernel against the oracle")
        out.append((name, d, want))
    yield out
    for _, d, _ in out:
        d.free()


def test_shipped_library_runs_every_start_of_the_strip_kernel():
    """The product (no hooks, no environment) in a fresh process: every frame of the list, strip kernel == exact kernel == oracle."""
    code = r'''
import os, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N
from oracle import pyoracle
import strip_prologue_common as SP
pyoracle.build()
L = N.load()
assert L.tic_build_has_test_hooks() == 0 and N._lib_path() == N.LIB_PATH
ctx = T.Context(0)
n = SP.check_all(ctx, L, N, lambda img: pyoracle.encode_zz16(img, SP.QUALITY), "shipped library")
ctx.close()
print("shipped library ok:", n, "cases")
'''
    env = {k: v for k, v in os.environ.items() if not k.startswith("TIC_")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "shipped library ok: %d cases" % (len(SP.SHAPES) + 1) in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize("order", ["by grid", "1", "0"])
@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: ",".join("%s=%s" % kv for kv in k.items()) or "default")
def test_hooks_build_schedules_and_orders(cases, monkeypatch, knobs, order):
    """Test-hooks build: each forced schedule under the pass order the grid picks, columns first (1) and rows first (0)."""
    assert N.load().tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_TUNE", "1")  # re-read the knobs at every launch
    for k in KNOB_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    if order != "by grid":
        monkeypatch.setenv("TIC_ORDER", order)
    ctx = cases[0][1].ctx
    for name, d, want in cases:
        got = d.run(N.KERNEL_HYBRID)
        assert np.array_equal(got, want), (name, knobs, order, int((got != want).any(axis=2).sum()), "blocks differ")
        # what the launcher decided (tic_last_strip_launch): the order forced is the order launched, and the frames built for a schedule got it
        info = (C.c_int * 8)()
        ctx.check(N.load().tic_last_strip_launch(ctx.handle, info))
        launched, kind, teams = info[0], info[1], info[2]
        if "no fast rectangle" in name:
            assert list(info) == [0] * 8, (name, list(info))
            continue
        assert launched == ({"1": 2, "0": 1}[order] if order != "by grid" else launched) and launched in (1, 2), (name, knobs, order, list(info))
        cap, sched = knobs.get("TIC_MAX_WGS"), int(knobs.get("TIC_SCHED", "1"))
        if name.startswith("512x512"):
            assert (kind, teams, info[4]) == (0, 0, 1), (name, knobs, list(info))  # strided under every cap here
        if name.startswith("2048x1536") and cap in ("64", "16"):
            assert (kind, teams) == (sched, 0), (name, knobs, list(info))  # larger than the chip: strided, chunked, round-interleaved as asked
        if name.startswith("1920x1080") and cap == "16":
            assert (kind, teams) == (sched, 0), (name, knobs, list(info))
        if kind == 1:
            assert info[5] == 4, (name, knobs, list(info))
        if name.startswith("2048x1536") and cap is None:  # the smallest team schedule - unless the weights are off
            assert (teams > 0 and info[4] > 1) == (knobs.get("TIC_SPLIT") != "0") and kind == 0, (name, knobs, list(info))
        if name.startswith("2048x1528") and cap is None:
            assert teams == 0 and kind == 0, (name, knobs, list(info))
