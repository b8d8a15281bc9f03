"""entropy_decode and lossless re-tabling without a GPU: the bindings of include/tinyimgcodec_hip_transcode.h, the Python checks that run
before a context exists, the fixture tests/golden/retable_damaged.json (the unmodified reference's reader followed by its writer over the
damaged default-table corpus, tests/golden/gen/make_goldens_retable.py), and the host reader + host writer under the sanitizers
(tests/native/transcode_host_selftest.cpp), whose default re-writes must be the fixture's."""
import ctypes as C
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

import damaged_streams as D
from conftest import ROOT

NEW_HEADER = os.path.join(ROOT, "include", "tinyimgcodec_hip_transcode.h")
FIXTURE = os.path.join(D.GOLDEN, "retable_damaged.json")
NAMES = ("tic_entropy_decode", "tic_entropy_decode_dev", "tic_entropy_decode_dev_timed", "tic_entropy_decode_adaptive", "tic_retable_adaptive",
         "tic_retable_default")


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_new_symbols_are_declared_exported_and_bound():
    with open(NEW_HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(tic_\w+)\s*\(", text))
    assert declared == set(N.TRANSCODE_SIGNATURES) == set(NAMES)
    assert not declared & set(N.SIGNATURES) and not declared & set(N.RATE_ADAPTIVE_SIGNATURES)
    assert '#include "tinyimgcodec_hip.h"' in text
    for path in (N.LIB_PATH, N.HOOKS_LIB_PATH):
        lib = C.CDLL(path)
        for name in declared:
            assert hasattr(lib, name), (path, name)
    L = N.load()
    for name in declared:
        assert getattr(L, name).argtypes is not None
    for name in ("entropy_decode", "entropy_decode_zz", "entropy_decode_adaptive", "retable_adaptive", "retable_default"):
        assert callable(getattr(T, name)), name
    # nobody but tic_api.hip includes the new header, and the main header does not know it
    for root, _, files in os.walk(os.path.join(ROOT, "tinyimgcodec_amd", "csrc")):
        for fn in files:
            if fn.endswith((".h", ".hip", ".cpp")) and fn != "tic_api.hip":
                with open(os.path.join(root, fn)) as f:
                    assert "tinyimgcodec_hip_transcode.h" not in f.read(), fn
    with open(os.path.join(ROOT, "include", "tinyimgcodec_hip.h")) as f:
        assert "transcode" not in f.read()


def test_every_call_is_an_argument_error_without_a_context():
    L = N.load()
    s = np.zeros(64, np.uint8)
    out = np.zeros(4096, np.uint8)
    n, ms = C.c_size_t(0), C.c_float(0)
    assert L.tic_entropy_decode(None, s.ctypes.data, s.size, out.ctypes.data, 8, None, None, None, None) == N.TIC_E_ARG
    assert L.tic_entropy_decode_dev(None, None, 64, None, 8, None, None, None, None) == N.TIC_E_ARG
    assert L.tic_entropy_decode_dev_timed(None, None, 64, None, 8, 1, 1, C.byref(ms)) == N.TIC_E_ARG
    assert L.tic_entropy_decode_adaptive(None, s.ctypes.data, s.size, out.ctypes.data, 8, None, None, None) == N.TIC_E_ARG
    assert L.tic_retable_adaptive(None, s.ctypes.data, s.size, out.ctypes.data, out.size, C.byref(n)) == N.TIC_E_ARG
    assert L.tic_retable_default(None, s.ctypes.data, s.size, out.ctypes.data, out.size, C.byref(n)) == N.TIC_E_ARG
    assert (out == 0).all() and n.value == 0


def head(h, w, q, flag):
    return struct.pack("<IIII", h & 0xFFFFFFFF, w & 0xFFFFFFFF, q & 0xFFFFFFFF, flag) + bytes(40)


class NoContext:
    """Stands where a context would: a check that reaches it has not run before _ctx(ctx)."""

    def __getattr__(self, name):
        raise AssertionError("the call reached the device (ctx.%s) before its header checks" % name)


def test_python_checks_come_before_the_device():
    nc = NoContext()
    for fn in (T.entropy_decode, T.entropy_decode_zz, T.retable_adaptive):
        with pytest.raises(struct.error):
            fn(bytes(15), ctx=nc)
        with pytest.raises(ValueError):  # the little-endian bit 31
            fn(head(8, 8, 50, 1 << 31), ctx=nc)
        with pytest.raises(ValueError):  # negative sizes
            fn(head(-8, 8, 50, 0), ctx=nc)
        with pytest.raises(ValueError):
            fn(head(8, -8, 50, 0), ctx=nc)
    for q in (0, 100, -1):  # what decompress() raises for such a header: the library's quality error
        with pytest.raises(N.NativeError) as e:
            T.entropy_decode(head(8, 8, q, 0), ctx=nc)
        assert e.value.code == N.TIC_E_QUALITY
        with pytest.raises(ValueError):
            T.retable_adaptive(head(8, 8, q, 0), ctx=nc)
    with pytest.raises(N.NativeError):
        T.entropy_decode(head(8, 8, 63, 1 << 30), ctx=nc)
    with pytest.raises(ValueError):  # scaled_dct into retable_adaptive: the flag word has room for one family
        T.retable_adaptive(head(8, 8, 3, 1 << 30), ctx=nc)
    with pytest.raises(IndexError):  # no blocks: no symbols to build a table from
        T.retable_adaptive(head(0, 8, 50, 0), ctx=nc)
    for fn in (T.entropy_decode_adaptive, T.retable_default):
        with pytest.raises(ValueError):
            fn(bytes(15), ctx=nc)
        with pytest.raises(ValueError):
            fn(head(-8, 8, 50, 1 << 31), ctx=nc)
        with pytest.raises(ValueError):
            fn(head(8, 8, 0, 1 << 31), ctx=nc)
        with pytest.raises(ValueError):
            fn(head(8, 8, 100, 1 << 31), ctx=nc)


def test_copy_out_banks():
    """The copy-out of dec_decode_coef_kernel replayed: lane j of round r reads dwords 4 (j & 7) + d of image 8 r + (j >> 3), the images
    kImgStrideB / 4 dwords apart; 4-byte LDS reads are served in lane groups {0-31}, {32-63} on bank = dword address mod 32.  No two lanes
    of a group share a bank in any of the 8 x 4 reads, every lane's 16 bytes lie inside its image's 128, and a round covers 1 KiB of the
    output contiguously.  Phase 1's two-byte stores at one scan position hit 32 banks per group as well."""
    with open(os.path.join(ROOT, "tinyimgcodec_amd", "csrc", "tic_entropy_dec_gpu.hip")) as f:
        src = f.read()
    stride = int(re.search(r"constexpr int kImgStrideB = (\d+);", src).group(1))
    assert stride % 4 == 0 and "(8u * r + sub) * (uint32_t)(kImgStrideB / 4) + 4u * piece" in src and "o[blk * 8u + piece]" in src
    sd = stride // 4
    for r in range(8):
        out = sorted(((8 * r + (j >> 3)) * 8 + (j & 7)) * 16 for j in range(64))
        assert out == list(range(r * 1024, (r + 1) * 1024, 16))
        for d in range(4):
            for group in (range(0, 32), range(32, 64)):
                dwords = [(8 * r + (j >> 3)) * sd + 4 * (j & 7) + d for j in group]
                assert len({x % 32 for x in dwords}) == 32, (r, d)
                assert all(x - (8 * r + (j >> 3)) * sd < 32 for x, j in zip(dwords, group))
    for k in range(64):
        for group in (range(0, 32), range(32, 64)):
            assert len({(lane * sd + k // 2) % 32 for lane in group}) == 32, k


def test_fixture_covers_exactly_the_corpus():
    fx = load_fixture()
    assert fx["generator"] == "tests/golden/gen/make_goldens_retable.py"
    with open(D.FIXTURE) as f:
        damaged = json.load(f)["entries"]
    assert len(fx["entries"]) == len(damaged) == 472
    assert [(e["name"], e["bytes"], e["sha256"]) for e in fx["entries"]] == [(e["name"], e["bytes"], e["sha256"]) for e in damaged]
    scaled = [e for e in fx["entries"] if e.get("scaled_dct")]
    assert len(scaled) == 2 and all(e["name"].split("/")[1] == "flag_scaled" for e in scaled)
    for e in fx["entries"]:
        assert "read_raises" not in e and "dc_outside_int16" not in e, e["name"]  # the reference read every entry, inside int16
        if not e.get("scaled_dct"):
            assert set(e["default"]) == set(e["adaptive"]) == {"bytes", "sha256"}, e["name"]  # no exception in either re-write
    assert not any(k in json.dumps(fx) for k in ("\"stream\":", "\"data\":"))  # no stream bytes


def test_host_reader_and_writer_under_sanitizers(oracle, tmp_path):
    """tests/native/transcode_host_selftest.cpp over the 470 non-scaled corpus streams: host entropy_decode, the DC differences again, host
    entropy_encode, compiled as HOST code with AddressSanitizer + UBSan and run as a program.  Every default re-write is the fixture's (the
    unmodified reference's reader followed by its writer), and a fixed point of reader + writer."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    fx = {e["name"]: e for e in load_fixture()["entries"]}
    entries = [e for e in D.corpus(oracle, D.base_streams(oracle)) if not fx[e[0]].get("scaled_dct")]
    assert len(entries) == 470
    cases = tmp_path / "cases.bin"
    with open(cases, "wb") as f:
        f.write(b"TICT" + struct.pack("<I", len(entries)))
        for name, base, kind, params, s in entries:
            assert D.sha(s) == fx[name]["sha256"], name
            f.write(struct.pack("<I", len(s)) + bytes(s))
    exe, out = tmp_path / "transcode_host_selftest", tmp_path / "out.bin"
    csrc = os.path.join(ROOT, "tinyimgcodec_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(rocm, "include"), "-o", str(exe), os.path.join(ROOT, "tests", "native", "transcode_host_selftest.cpp"),
                    os.path.join(csrc, "tic_entropy.cpp"), "-lpthread"], check=True)
    r = subprocess.run([str(exe), str(cases), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "transcode_host_selftest ok 470 cases, 0 refused, 470 re-written twice" in r.stdout and not r.stderr, r.stdout + r.stderr
    blob = out.read_bytes()
    at = 0
    for name, base, kind, params, s in entries:
        (n,) = struct.unpack_from("<I", blob, at)
        got = blob[at + 4:at + 4 + n]
        at += 4 + n
        assert (len(got), D.sha(got)) == (fx[name]["default"]["bytes"], fx[name]["default"]["sha256"]), name
    assert at == len(blob)
