"""CPU side of the integer encoder's batch forms (compress_batch_scaled, rd_points_scaled_batch): the table of the transform's descriptor
form and a host model of its walk under the sanitizers (tests/native/scaledplan_selftest.cpp), the exported symbols, the test hook, the
fixture's own consistency, and the Python mirror's argument checks that need no GPU."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tic_compress_batch_scaled_v", "tic_last_compress_batch_scaled", "tic_dctq_scaled_v_dev", "tic_rd_points_scaled_v", "tic_last_rd_scaled_batch")
SETTINGS = ("best", "high", "med", "low")


def test_scaled_table_and_walk_under_the_sanitizers(tmp_path):
    """fill_scaled_table (csrc/tic_scaled_frames.h, compiled by g++ alone) for 1..64 records of 1..70,000 blocks, widths that are and are
    not multiples of 8 blocks: strips tile the launch, no strip belongs to two records, trailing entries 0xffffffff; a host model of the
    kernel's walk at grids of 1, 3 and 8,192 waves writes every block of every record exactly once and nothing else.  A stand-alone
    program, built with the address and undefined-behaviour sanitizers."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = tmp_path / "scaledplan_selftest"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-pthread", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "scaledplan_selftest.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "scaledplan_selftest ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stdout[-2000:] + r.stderr[-2000:]


def test_scaled_batch_symbols_are_declared_exported_and_bound():
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
    assert callable(T.compress_batch_scaled) and callable(T.rd_points_scaled_batch)
    assert T.__all__ == ["encode", "decode", "compress", "decompress"]


def test_scaled_batch_null_context():
    L = N.load()
    assert L.tic_compress_batch_scaled_v(None, None, 0, None, None, None, None, None, None, None) == N.TIC_E_ARG
    assert L.tic_last_compress_batch_scaled(None, None, None, None, None) == N.TIC_E_ARG
    assert L.tic_dctq_scaled_v_dev(None, None, 0, None, None, None, None, None) == N.TIC_E_ARG
    assert L.tic_rd_points_scaled_v(None, None, 0, None, None, None, None, 0, None, None, None) == N.TIC_E_ARG
    assert L.tic_last_rd_scaled_batch(None, None, None, None, None, None, None) == N.TIC_E_ARG


def test_groups_hook_is_in_the_hooks_library_only():
    """TIC_SCALED_V_GROUPS lowers the descriptor form's workgroup count in the test-hooks build; the product reads no environment."""
    with open(N.HOOKS_LIB_PATH, "rb") as f:
        assert b"TIC_SCALED_V_GROUPS" in f.read()
    with open(N.LIB_PATH, "rb") as f:
        assert b"TIC_SCALED_V_GROUPS" not in f.read()


def test_fixture_agrees_with_the_single_frame_fixture():
    """scaled_batch.json: the whole benchmark set at four settings, recorded results only; Lenna's entries are scaled_encode.json's."""
    with open(os.path.join(ROOT, "tests", "golden", "scaled_batch.json")) as f:
        doc = json.load(f)
    with open(os.path.join(ROOT, "tests", "golden", "scaled_encode.json")) as f:
        pinned = json.load(f)["cases"]
    npix = np.load(os.path.join(ROOT, "tests", "golden", "benchmark_set.npz"))["pixels"].shape[0]
    assert doc["subset"] == "all" and sorted(int(k) for k in doc["bench"]) == list(range(npix)) and npix == 49
    for entry in list(doc["bench"].values()) + [doc["lenna"]]:
        assert sorted(entry) == sorted(SETTINGS)
        sizes = [entry[s]["bytes"] for s in SETTINGS]
        assert all(len(entry[s]["sha256"]) == 64 for s in SETTINGS) and sizes == sorted(sizes, reverse=True) and sizes[-1] > 17
    for s in SETTINGS:
        assert doc["lenna"][s] == {"bytes": pinned["lenna512_" + s]["bytes"], "sha256": pinned["lenna512_" + s]["sha256"]}


def test_arguments_fail_before_any_gpu_work():
    """What compress_scaled raises for the same arguments, without touching a device."""
    img = np.zeros((16, 16), np.uint8)
    with pytest.raises(ValueError, match="2 entries for 3 frames"):
        T.compress_batch_scaled([img, img, img], ["med", "low"])
    for bad in ("medium", 4, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="scaled-DCT quality"):
            T.compress_batch_scaled([img, img], bad)
        with pytest.raises(ValueError, match="scaled-DCT quality"):
            T.compress_batch_scaled([img, img], ["med", bad])
        with pytest.raises(ValueError, match="scaled-DCT quality"):
            T.rd_points_scaled_batch([img], ["best", bad])
    for frame in (np.zeros((12, 16), np.uint8), np.zeros((16, 20), np.uint8)):
        with pytest.raises(ValueError, match="multiples of 8"):
            T.compress_batch_scaled([img, frame])
        with pytest.raises(ValueError, match="multiples of 8"):
            T.rd_points_scaled_batch([img, frame])
    with pytest.raises(ValueError):
        T.compress_batch_scaled([img, np.full((8, 8), 300, np.int32)])  # 8-bit images only
    with pytest.raises(ValueError):
        T.rd_points_scaled_batch([np.full((8, 8), -1, np.int32)])
    assert T.compress_batch_scaled([]) == [] and T.compress_batch_scaled([], []) == []
    got = T.rd_points_scaled_batch([])
    assert [a.shape for a in got] == [(0, 4)] * 3 and [a.dtype for a in got] == [np.int64, np.uint64, np.uint64]
    got = T.rd_points_scaled_batch([img], [])
    assert [a.shape for a in got] == [(1, 0)] * 3 and [a.dtype for a in got] == [np.int64, np.uint64, np.uint64]


def test_cli_refuses_also_with_a_search(tmp_path):
    """--also with --scaled is one compress_batch_scaled call now; with --max-bytes or --min-psnr it stays an argparse error."""
    from tinyimgcodec_amd import encode_cli

    a = str(tmp_path / "a.npy")
    np.save(a, np.zeros((8, 8), np.uint8))
    for extra in (["--max-bytes", "100"], ["--min-psnr", "30"]):
        with pytest.raises(SystemExit) as e:
            encode_cli.main([a, str(tmp_path / "a.img"), "--also", a, str(tmp_path / "b.img")] + extra)
        assert e.value.code == 2
