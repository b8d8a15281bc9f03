"""CPU side of the batch forms of rate-distortion control: the host plan under the sanitizers (tests/native/rdplan_selftest.cpp), the
exported symbols, and the Python mirror's argument checks that need no GPU."""
import ctypes
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tic_rd_points_v", "tic_compress_batch_to_psnr", "tic_last_rd_batch", "tic_distortion_v_dev", "tic_distortion_v_dev_timed")


def test_rd_plan_under_the_sanitizers(tmp_path):
    """fill_sse_probe_table and the lockstep search by distortion (csrc/tic_rd_plan.h, compiled by g++ alone): probe tables of 1..64 probes
    of 1..300,000 blocks at group caps 1, 2, 3 and 1,024 tile the grid, no group spans two probes, trailing entries 0xffffffff, every tile
    of a probe walked exactly once by the probe's own stride; the search equals the plain bisection on monotone, saw-toothed, null-topped,
    never-meeting and always-meeting error tables at depths 1..3, probes no quality twice and stays within 1 + ceil(7 / depth) rounds.  A
    stand-alone program, built with the address and undefined-behaviour sanitizers."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = tmp_path / "rdplan_selftest"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-pthread", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "rdplan_selftest.cpp"), os.path.join(ROOT, "tinyimgcodec_amd", "csrc", "tic_entropy.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rdplan_selftest ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stdout[-2000:] + r.stderr[-2000:]


def test_rd_batch_symbols_are_declared_exported_and_bound():
    """The five new calls: declared in the public header, exported by the product and by the test-hooks build, bound by _native; the two
    Python functions importable from the package, whose __all__ stays the reference's four names."""
    with open(os.path.join(ROOT, "include", "tinyimgcodec_hip.h")) as f:
        header = f.read()
    for path in (N.LIB_PATH, N.HOOKS_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in NEW:
            assert hasattr(lib, name), (path, name)
    for name in NEW:
        assert "int %s(" % name in header, name
        assert name in N.SIGNATURES, name
    assert callable(T.rd_points_batch) and callable(T.compress_batch_to_psnr)
    assert T.__all__ == ["encode", "decode", "compress", "decompress"]


def test_rd_batch_null_context():
    L = N.load()
    assert L.tic_rd_points_v(None, None, 0, None, None, None, None, 0, None, None, None) == N.TIC_E_ARG
    assert L.tic_compress_batch_to_psnr(None, None, 0, None, None, None, None, 1, 99, None, None, None, None, None, None) == N.TIC_E_ARG
    assert L.tic_last_rd_batch(None, None) == N.TIC_E_ARG
    assert L.tic_distortion_v_dev(None, None, None, 0, None, None, None, None, None) == N.TIC_E_ARG
    assert L.tic_distortion_v_dev_timed(None, None, None, 0, None, None, None, None, 0, 1, None) == N.TIC_E_ARG


def test_rd_batch_arguments_fail_before_any_gpu_work():
    """What compress_to_psnr / rd_points raise for the same arguments, without touching a device."""
    img = np.zeros((16, 16), np.uint8)
    for fn in (lambda q: T.rd_points_batch([img, img], [50, q]), lambda q: T.compress_batch_to_psnr([img, img], 30.0, q, 99),
               lambda q: T.compress_batch_to_psnr([img], [30.0], 1, q)):
        with pytest.raises(ZeroDivisionError):
            fn(0)
        with pytest.raises(KeyError):
            fn(100)
        with pytest.raises(ValueError):
            fn(101)
        with pytest.raises(struct.error):
            fn(-3)
        with pytest.raises(struct.error):
            fn(50.0)
    with pytest.raises(ValueError, match="2 entries for 3 frames"):
        T.compress_batch_to_psnr([img, img, img], [30.0, 30.0])
    with pytest.raises(ValueError, match="not a number"):
        T.compress_batch_to_psnr([img, img], [30.0, math.nan])
    with pytest.raises(ValueError, match="not a number"):
        T.compress_batch_to_psnr([img], math.nan)
    with pytest.raises(ValueError, match="above max_quality"):
        T.compress_batch_to_psnr([img], 30.0, 60, 20)
    with pytest.raises(ValueError):
        T.compress_batch_to_psnr([img, np.full((8, 8), 300, np.int32)], 30.0)  # 8-bit images only
    with pytest.raises(ValueError):
        T.rd_points_batch([np.full((8, 8), -1, np.int32)], [50])
    assert T.compress_batch_to_psnr([], 30.0) == [] and T.compress_batch_to_psnr([], []) == []
    got = T.rd_points_batch([], [5, 50])
    assert [a.shape for a in got] == [(0, 2)] * 3 and [a.dtype for a in got] == [np.int64, np.uint64, np.uint64]
    got = T.rd_points_batch([img], [])
    assert [a.shape for a in got] == [(1, 0)] * 3 and [a.dtype for a in got] == [np.int64, np.uint64, np.uint64]
