"""Batch transcoding without a GPU: the bindings of include/tinyimgcodec_hip_transcode_batch.h, the calls without a context, the host plan
(tinyimgcodec_amd/csrc/tic_transcode_plan.h) swept under the sanitizers by tests/native/transcode_plan_selftest.cpp, and the Python checks
that run before a context exists."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "tinyimgcodec_hip_transcode_batch.h")
NAMES = ("tic_entropy_decode_batch", "tic_retable_adaptive_batch", "tic_retable_default_batch", "tic_last_transcode_batch")


def test_symbols_are_declared_exported_and_bound():
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(tic_\w+)\s*\(", text))
    assert declared == set(N.TRANSCODE_BATCH_SIGNATURES) == set(NAMES)
    for other in (N.SIGNATURES, N.RATE_ADAPTIVE_SIGNATURES, N.TRANSCODE_SIGNATURES):
        assert not declared & set(other)
    assert '#include "tinyimgcodec_hip_transcode.h"' in text
    for path in (N.LIB_PATH, N.HOOKS_LIB_PATH):
        lib = C.CDLL(path)
        for name in declared:
            assert hasattr(lib, name), (path, name)
    L = N.load()
    for name in declared:
        assert getattr(L, name).argtypes == N.TRANSCODE_BATCH_SIGNATURES[name][1]
    for name in ("entropy_decode_zz_batch", "retable_adaptive_batch", "retable_default_batch"):
        assert callable(getattr(T, name)), name
    # nobody but tic_api.hip includes the new header, and the two older headers do not know it
    for root, _, files in os.walk(os.path.join(ROOT, "tinyimgcodec_amd", "csrc")):
        for fn in files:
            if fn.endswith((".h", ".hip", ".cpp")) and fn != "tic_api.hip":
                with open(os.path.join(root, fn)) as f:
                    assert "tinyimgcodec_hip_transcode_batch.h" not in f.read(), fn
    with open(os.path.join(ROOT, "tinyimgcodec_amd", "csrc", "tic_api.hip")) as f:
        assert "tinyimgcodec_hip_transcode_batch.h" in f.read()
    for older in ("tinyimgcodec_hip.h", "tinyimgcodec_hip_transcode.h"):
        with open(os.path.join(ROOT, "include", older)) as f:
            assert "transcode_batch" not in f.read(), older


def test_every_call_is_an_argument_error_without_a_context():
    L = N.load()
    s = np.zeros(64, np.uint8)
    out = np.zeros(4096, np.uint8)
    ptr = (C.c_void_p * 1)(s.ctypes.data)
    optr = (C.c_void_p * 1)(out.ctypes.data)
    lens, caps, olens, rcs = (C.c_size_t * 1)(64), (C.c_size_t * 1)(8), (C.c_size_t * 1)(0), (C.c_int * 1)(77)
    a = C.c_int(-5)
    assert L.tic_entropy_decode_batch(None, ptr, lens, 1, optr, caps, None, None, None, None, rcs) == N.TIC_E_ARG
    assert L.tic_retable_adaptive_batch(None, ptr, lens, 1, optr, caps, olens, rcs) == N.TIC_E_ARG
    assert L.tic_retable_default_batch(None, ptr, lens, 1, optr, caps, olens, rcs) == N.TIC_E_ARG
    assert L.tic_last_transcode_batch(None, C.byref(a), None, None) == N.TIC_E_ARG
    assert (out == 0).all() and olens[0] == 0 and rcs[0] == 77 and a.value == -5


def test_the_plan_under_the_sanitizers(tmp_path):
    """tests/native/transcode_plan_selftest.cpp: frame counts 0..130, block counts around 255 / 256 / 257 and 1,024 / 1,025, frames without
    blocks, frames not taken, limits that force chunks of one - against a plain recomputation; and the form that shows the sweep can fail."""
    assert shutil.which("g++") is not None, "the plan sweep needs a host compiler: it is not skipped"
    exe = tmp_path / "transcode_plan_selftest"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-pthread", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "transcode_plan_selftest.cpp"), os.path.join(ROOT, "tinyimgcodec_amd", "csrc", "tic_entropy.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "transcode_plan_selftest ok 917 cases" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([str(exe), "--break-gap"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "FAILED" in r.stdout and "Sanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def test_the_plan_header_is_free_of_hip_and_of_the_context():
    with open(os.path.join(ROOT, "tinyimgcodec_amd", "csrc", "tic_transcode_plan.h")) as f:
        text = f.read()
    assert "hip_runtime" not in text and "tic_ctx" not in text and "hipStream" not in text


def head(h, w, q, flag):
    return struct.pack("<IIII", h & 0xFFFFFFFF, w & 0xFFFFFFFF, q & 0xFFFFFFFF, flag) + bytes(40)


class NoContext:
    """Stands where a context would: a check that reaches it has not run before _ctx(ctx)."""

    def __getattr__(self, name):
        raise AssertionError("the call reached the device (ctx.%s) before its header checks" % name)


BATCHES = (T.entropy_decode_zz_batch, T.retable_adaptive_batch, T.retable_default_batch)


def test_python_argument_checks():
    nc = NoContext()
    for fn in BATCHES:
        assert fn([], ctx=nc) == []
        with pytest.raises(ValueError):
            fn([], ctx=nc, errors="ignore")
    # frames that fail the single call's own checks, in the single call's classes, without a device; the message names the frame
    cases = {
        T.entropy_decode_zz_batch: [(bytes(15), struct.error), (head(8, 8, 50, 1 << 31), ValueError), (head(-8, 8, 50, 0), ValueError), (head(8, 8, 0, 0), N.NativeError),
                                    (head(8, 8, 63, 1 << 30), N.NativeError)],
        T.retable_adaptive_batch: [(bytes(15), struct.error), (head(8, 8, 50, 1 << 31), ValueError), (head(8, 8, 3, 1 << 30), ValueError), (head(8, 8, 100, 0), ValueError),
                                   (head(0, 8, 50, 0), IndexError)],
        T.retable_default_batch: [(bytes(15), ValueError), (head(-8, 8, 50, 1 << 31), ValueError), (head(8, 8, 0, 1 << 31), ValueError)],
    }
    for fn, frames in cases.items():
        got = fn([s for s, _ in frames], ctx=nc, errors="return")
        assert len(got) == len(frames)
        for i, ((s, cls), e) in enumerate(zip(frames, got)):
            assert type(e) is cls, (fn.__name__, i, e)
            if cls is not struct.error:
                assert "frame %d: " % i in str(e), (fn.__name__, i, str(e))
        for i, (s, cls) in enumerate(frames):
            with pytest.raises(cls) as ei:
                fn([s], ctx=nc)
            if cls is N.NativeError:
                assert ei.value.code == N.TIC_E_QUALITY
        with pytest.raises(frames[0][1]):  # errors="raise": the lowest failing index
            fn([s for s, _ in frames], ctx=nc)
