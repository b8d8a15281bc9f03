"""CPU side of the batch forms of rate control: the host plan under the sanitizers (tests/native/rateplan_selftest.cpp), the exported
symbols, and the Python mirror's argument checks that need no GPU."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tic_stream_sizes_v", "tic_compress_batch_to_size", "tic_last_rate_batch")


def test_rate_plan_under_the_sanitizers(tmp_path):
    """fill_size_probe_table, plan_rate_batch, layout_rate_submission, rate_transform_run and the lockstep search (csrc/tic_rate_plan.h,
    compiled by g++ alone): probe tables of 1..64 probes of 1..300,000 blocks tile grid and workspace, no group spans two probes, trailing
    entries 0xffffffff; the search equals the plain bisection on monotone, null-topped, saw-toothed, all-fit and none-fit tables at depths
    1..3, probes no quality twice and stays within its round bound.  A stand-alone program, built with the address and
    undefined-behaviour sanitizers."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = tmp_path / "rateplan_selftest"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-pthread", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "rateplan_selftest.cpp"), os.path.join(ROOT, "tinyimgcodec_amd", "csrc", "tic_entropy.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rateplan_selftest ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stdout[-2000:] + r.stderr[-2000:]


def test_rate_batch_symbols_are_declared_exported_and_bound():
    """The three new calls: declared in the public header, exported by the product and by the test-hooks build, bound by _native."""
    with open(os.path.join(ROOT, "include", "tinyimgcodec_hip.h")) as f:
        header = f.read()
    for path in (N.LIB_PATH, N.HOOKS_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in NEW:
            assert hasattr(lib, name), (path, name)
    for name in NEW:
        assert "int %s(" % name in header, name
        assert name in N.SIGNATURES, name


def test_rate_batch_null_context():
    L = N.load()
    assert L.tic_stream_sizes_v(None, None, 0, None, None, None, None, 0, None) == N.TIC_E_ARG
    assert L.tic_compress_batch_to_size(None, None, 0, None, None, None, None, 1, 99, None, None, None, None, None) == N.TIC_E_ARG
    assert L.tic_last_rate_batch(None, None, None, None, None, None, None) == N.TIC_E_ARG


def test_rate_batch_arguments_fail_before_any_gpu_work():
    """What compress_to_size / compressed_sizes raise for the same arguments, without touching a device."""
    img = np.zeros((16, 16), np.uint8)
    for fn in (lambda q: T.compressed_sizes_batch([img, img], [50, q]), lambda q: T.compress_batch_to_size([img, img], 1000, q, 99),
               lambda q: T.compress_batch_to_size([img], [1000], 1, q)):
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
        T.compress_batch_to_size([img, img, img], [1000, 1000])
    with pytest.raises(ValueError, match="negative"):
        T.compress_batch_to_size([img, img], [1000, -1])
    with pytest.raises(ValueError, match="negative"):
        T.compress_batch_to_size([img], -5)
    with pytest.raises(ValueError, match="above max_quality"):
        T.compress_batch_to_size([img], 1000, 60, 20)
    with pytest.raises(ValueError):
        T.compress_batch_to_size([img, np.full((8, 8), 300, np.int32)], 1000)  # 8-bit images only
    with pytest.raises(ValueError):
        T.compressed_sizes_batch([np.full((8, 8), -1, np.int32)], [50])
    assert T.compress_batch_to_size([], 1000) == [] and T.compress_batch_to_size([], []) == []
    got = T.compressed_sizes_batch([], [5, 50])
    assert got.shape == (0, 2) and got.dtype == np.int64
    assert T.compressed_sizes_batch([img], []).shape == (1, 0)
