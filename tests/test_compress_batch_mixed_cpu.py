"""CPU side of the mixed batch: the plan under the sanitizers (tests/native/batchplan_selftest.cpp), the exported symbols, and the Python mirror's
argument checks that need no GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N


def test_batch_plan_under_the_sanitizers(tmp_path):
    """plan_mixed_batch and mixed_chunk_table (csrc/tic_host_pipeline.h, csrc/tic_entropy_frames.h) on the frame list of the GPU test, on the reference's
    benchmark loop and on 300 random lists, at several chunk limits and in both packing modes: every caller's index exactly once; the order
    (quality, width, height), stable; pixels, coefficients and stream areas tiling their buffers, every stream area holding tic_compress_bound(h, w);
    maximal runs of equal width and quality with heights that are multiples of 8; the entropy stage's records tiling the coefficient buffer and
    both grids without gap or overlap.  A stand-alone program, built with the address and undefined-behaviour sanitizers."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = tmp_path / "batchplan_selftest"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-pthread", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "batchplan_selftest.cpp"), os.path.join(ROOT, "tinyimgcodec_amd", "csrc", "tic_entropy.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "batchplan_selftest ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stdout[-2000:] + r.stderr[-2000:]


def test_mixed_batch_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "tinyimgcodec_hip.h")).read()
    for name in ("tic_compress_batch_v", "tic_last_compress_batch_v"):
        assert name + "(" in hdr and name in N.SIGNATURES
        for path in (N.LIB_PATH, N.HOOKS_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), name), (path, name)
    # the byte budget's hook is compiled out of the library that ships
    assert b"TIC_BATCH_CHUNK_BYTES" in open(N.HOOKS_LIB_PATH, "rb").read() and b"TIC_BATCH_CHUNK_BYTES" not in open(N.LIB_PATH, "rb").read()
    # without a context the call is an argument error, and it touches nothing
    assert N.load().tic_compress_batch_v(None, None, 0, None, None, None, None, None, None, None) == N.TIC_E_ARG
    assert N.load().tic_last_compress_batch_v(None, None, None, None, None) == N.TIC_E_ARG


def test_python_argument_checks_need_no_gpu():
    """What compress_batch() refuses before it asks for a context: a quality list of the wrong length, a bad quality in the list (what compress()
    raises for it), pixels outside 0..255, and a mixed call with threads > 0 or devices=."""
    a, b = np.zeros((8, 8), np.uint8), np.zeros((16, 8), np.uint8)
    with pytest.raises(ValueError, match="2 entries for 3 frames"):
        T.compress_batch([a, b, a], [50, 60])
    with pytest.raises(ValueError, match="entries"):
        T.compress_batch([a], [])
    assert T.compress_batch([], []) == [] and T.compress_batch([], 50) == []
    for bad in (0, 100, -3):
        with pytest.raises(Exception) as single:
            T.compress(a, bad)
        assert not isinstance(single.value, T.NativeUnavailable)
        with pytest.raises(type(single.value)):
            T.compress_batch([a, b, a], [50, bad, 50])
    with pytest.raises(ValueError, match="not supported"):
        T.compress_batch([a, b], 50, threads=2)
    with pytest.raises(ValueError, match="not supported"):
        T.compress_batch([a, a], [50, 60], threads=1)
    with pytest.raises(ValueError, match="not supported"):
        T.compress_batch([a, b], 50, devices=[0])
    with pytest.raises(ValueError, match="not supported"):
        T.compress_batch([a, a], [50, 60], devices=[0, 0])
    with pytest.raises(ValueError, match="0..255"):
        T.compress_batch([a, np.full((8, 8), 300)], [50, 60])
