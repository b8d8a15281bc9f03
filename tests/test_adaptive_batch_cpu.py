"""CPU side of the adaptive batch encoder: its host plan under the sanitizers (tests/native/adaptplan_selftest.cpp), the exported symbols, and
the Python mirror's argument checks that need no GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N


def test_adaptive_plan_under_the_sanitizers(tmp_path):
    """adaptive_chunk_table, assign_adaptive_streams and adaptive_slot_layout (csrc/tic_adaptive_frames.h, compiled by g++ alone) over the
    fixture's frame list, the 294-frame benchmark loop and 300 random lists at several chunk limits: every frame exactly once; workgroups
    tiling the grid without gap or overlap and none spanning two frames; statistics, table and stream-area records tiling their buffers;
    stream areas at multiples of 16.  A stand-alone program, built with the address and undefined-behaviour sanitizers."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = tmp_path / "adaptplan_selftest"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-pthread", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "adaptplan_selftest.cpp"), os.path.join(ROOT, "tinyimgcodec_amd", "csrc", "tic_entropy.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "adaptplan_selftest ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stdout[-2000:] + r.stderr[-2000:]


def test_adaptive_batch_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "tinyimgcodec_hip.h")).read()
    for name in ("tic_compress_batch_adaptive_v", "tic_entropy_encode_adaptive_batch", "tic_last_compress_batch_adaptive"):
        assert name + "(" in hdr and name in N.SIGNATURES
        for path in (N.LIB_PATH, N.HOOKS_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), name), (path, name)
    assert callable(T.compress_batch_adaptive) and callable(T.entropy_encode_adaptive_batch)
    # the chunk hooks are compiled out of the library that ships
    for hook in (b"TIC_BATCH_CHUNK_BYTES", b"TIC_BATCH_CHUNK\0"):
        assert hook in open(N.HOOKS_LIB_PATH, "rb").read() and hook not in open(N.LIB_PATH, "rb").read()
    # without a context every call is an argument error, and it touches nothing
    L = N.load()
    assert L.tic_compress_batch_adaptive_v(None, None, 0, None, None, None, None, None, None, None) == N.TIC_E_ARG
    assert L.tic_entropy_encode_adaptive_batch(None, None, 0, None, None, None, None, None, None) == N.TIC_E_ARG
    assert L.tic_last_compress_batch_adaptive(None, None, None, None) == N.TIC_E_ARG


def test_python_argument_checks_need_no_gpu():
    """What compress_batch_adaptive() refuses before it asks for a context: a quality list of the wrong length, a bad quality (what
    compress_adaptive() raises for it), pixels outside 0..255, a frame without blocks (IndexError, as the reference); [] gives []."""
    a, b = np.zeros((8, 8), np.uint8), np.zeros((16, 8), np.uint8)
    with pytest.raises(ValueError, match="2 entries for 3 frames"):
        T.compress_batch_adaptive([a, b, a], [50, 60])
    with pytest.raises(ValueError, match="entries"):
        T.compress_batch_adaptive([a], [])
    assert T.compress_batch_adaptive([], []) == [] and T.compress_batch_adaptive([], 50) == [] and T.compress_batch_adaptive([]) == []
    assert T.entropy_encode_adaptive_batch([], [], []) == []
    for bad in (0, 100, 101, -3, 50.0):
        with pytest.raises(Exception) as single:
            T.compress_adaptive(a, bad)
        assert not isinstance(single.value, T.NativeUnavailable)
        with pytest.raises(type(single.value)):
            T.compress_batch_adaptive([a, b, a], [50, bad, 50])
        with pytest.raises(type(single.value)):
            T.compress_batch_adaptive([a, b], bad)
    with pytest.raises(ValueError, match="0..255"):
        T.compress_batch_adaptive([a, np.full((8, 8), 300)], [50, 60])
    for shape in ((0, 0), (0, 8), (8, 0)):
        with pytest.raises(IndexError):
            T.compress_batch_adaptive([a, np.zeros(shape, np.uint8)], 50)
    # the first offending frame's exception: frame 0 is empty, frame 1 has a bad quality
    with pytest.raises(IndexError):
        T.compress_batch_adaptive([np.zeros((0, 8), np.uint8), a], [50, 0])
    with pytest.raises(ZeroDivisionError):
        T.compress_batch_adaptive([a, np.zeros((0, 8), np.uint8)], [0, 50])
    with pytest.raises(ValueError, match="do not match"):
        T.entropy_encode_adaptive_batch([np.zeros((2, 64), np.int16)], [(8, 8)], [50])
    with pytest.raises(ValueError, match="shapes"):
        T.entropy_encode_adaptive_batch([np.zeros((1, 64), np.int16)], [], [50])
