"""CPU side of the adaptive batch decoder (tic_decompress_batch_adaptive, decompress_batch_adaptive): its host plan under the sanitizers
(tests/native/adecplan_selftest.cpp), the exported symbols, and the Python mirror's argument checks that need no GPU."""
import ctypes
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

NEW = ("tic_decompress_batch_adaptive", "tic_last_decompress_batch_adaptive", "tic_adaptive_decode_geometry")


def test_adaptive_decode_plan_under_the_sanitizers(tmp_path):
    """Everything tic_decompress_batch_adaptive works out from geometries, stream lengths and payload starts alone lives in
    csrc/tic_adaptive_decode_plan.h, and tests/native/adecplan_selftest.cpp (a stand-alone program, g++ -fsanitize=address,undefined) sweeps it:
    seeded batches of 0..300 frames against the library's limits and random ones.  Every taken frame is in exactly one chunk, in order; no two
    frames' words, ranges, blocks, workgroups, pixel or table slots overlap; every offset is aligned as promised; the totals are the sums; every
    workgroup -> frame entry (filled by the function the library calls) points at the frame that owns the workgroup; the upload layout's pieces
    do not overlap; a chunk passes a limit only when it holds a single frame; one case is derived by hand.  With --break-cut the sweep runs
    on a cut that tests the limits after the frame joined and must find its counterexamples: the sweep can fail."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = tmp_path / "adecplan_selftest"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "adecplan_selftest.cpp"), os.path.join(ROOT, "tinyimgcodec_amd", "csrc", "tic_entropy.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("adecplan_selftest ok") and ", 0 counterexamples" in r.stdout and \
        "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    b = subprocess.run([str(exe), "--break-cut"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 1 and "adecplan_selftest FAILED (broken cut)" in b.stdout and "counterexample: only a single frame passes a byte limit" in b.stdout and \
        "Sanitizer" not in b.stderr and "runtime error" not in b.stderr, b.stdout[-2000:] + b.stderr[-2000:]


def test_adaptive_decode_batch_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "tinyimgcodec_hip.h")).read()
    for name in NEW:
        assert name + "(" in hdr and name in N.SIGNATURES
        for path in (N.LIB_PATH, N.HOOKS_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), name), (path, name)
    assert callable(T.decompress_batch_adaptive) and "decompress_batch_adaptive" in T.codec.__doc__
    # the chunk hook is compiled out of the library that ships
    assert b"TIC_ADBATCH_CHUNK" in open(N.HOOKS_LIB_PATH, "rb").read() and b"TIC_ADBATCH_CHUNK" not in open(N.LIB_PATH, "rb").read()
    # without a context every call is an argument error, and it touches nothing
    L = N.load()
    assert L.tic_decompress_batch_adaptive(None, None, None, 0, None, None, None, None) == N.TIC_E_ARG
    assert L.tic_last_decompress_batch_adaptive(None, None, None, None) == N.TIC_E_ARG


def test_geometry_query_is_the_decoders_rule():
    """tic_adaptive_decode_geometry needs no context: two average blocks per range, 256 bits at least and 4,096 at most, and the ranges that
    start in front of the stream's end."""
    L = N.load()
    rb, nr = ctypes.c_int(), ctypes.c_size_t()
    for length, payload_bit, nblocks in [(2649, 1500, 96), (201, 700, 6), (30001, 2000, 255), (865763, 3000, 32400), (100, 300, 1), (1 << 20, 999, 3)]:
        assert L.tic_adaptive_decode_geometry(length, payload_bit, nblocks, ctypes.byref(rb), ctypes.byref(nr)) == 0
        payload = length * 8 - payload_bit
        want = min(max(2 * payload // nblocks, 256), 4096)
        assert rb.value == want and nr.value == -(-payload // want), (length, payload_bit, nblocks, rb.value, nr.value)
    assert L.tic_adaptive_decode_geometry(2649, 1500, 96, None, None) == 0
    assert L.tic_adaptive_decode_geometry(100, 800, 4, ctypes.byref(rb), ctypes.byref(nr)) == N.TIC_E_ARG  # no payload
    assert L.tic_adaptive_decode_geometry(100, 300, 0, ctypes.byref(rb), ctypes.byref(nr)) == N.TIC_E_ARG  # no block
    assert L.tic_adaptive_decode_geometry(1 << 29, 300, 4, ctypes.byref(rb), ctypes.byref(nr)) == N.TIC_E_ARG  # bit positions beyond 32 bits


def test_python_argument_checks_need_no_gpu():
    """What decompress_batch_adaptive() answers before it asks for a context: [] for an empty list, ValueError naming the frame for a stream
    shorter than its 16-byte header."""
    assert T.decompress_batch_adaptive([]) == [] and T.decompress_batch_adaptive(()) == []
    with pytest.raises(ValueError, match="frame 0: stream shorter than its 16-byte header"):
        T.decompress_batch_adaptive([b"\0" * 15])
    good = bytes(16)  # (a 0 x 0 header: its turn never comes)
    with pytest.raises(ValueError, match="frame 1: stream shorter"):
        T.decompress_batch_adaptive([good, b"", good])
