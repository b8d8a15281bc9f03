"""Requantisation without a GPU: the fixture tests/golden/requantize.json against the plain numpy model of tests/requantize_common.py and its
two mutants, the bindings of include/tinyimgcodec_hip_requantize.h, the calls without a context, the host plan
(tinyimgcodec_amd/csrc/tic_requant_plan.h) swept under the sanitizers by tests/native/requant_plan_selftest.cpp, and the Python checks that
run before a context exists."""
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

import requantize_common as RC
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "tinyimgcodec_hip_requantize.h")
NAMES = ("tic_requantize_zz", "tic_requantize_zz_dev", "tic_requantize_zz_v_dev", "tic_requantize", "tic_requantized_sizes", "tic_requantize_to_size",
         "tic_requant_kernels_timed", "tic_last_requantize")


def test_fixture_is_whole():
    fx = RC.load_fixture()
    zz = RC.corpus()
    RC.check_corpus(zz)
    assert fx["corpus_sha256"] == RC.digest(zz)
    assert [(p["from"], p["to"]) for p in fx["pairs"]] == RC.pairs() and len(fx["pairs"]) == 5 * 99 + 94
    by = {(p["from"], p["to"]): p for p in fx["pairs"]}
    assert by[(50, 25)]["ties"] > 0  # 50 -> 25 halves every coefficient: every odd one is an exact tie
    assert fx["totals"]["rational_differs"] > 0 and fx["totals"]["away_differs"] > 0
    assert 0 < sum(p["outside_int16_latin"] > 0 for p in fx["pairs"]) < sum(p["outside_int16"] > 0 for p in fx["pairs"]) < len(fx["pairs"])
    for q in range(1, 100):
        assert by[(q, q)]["outside_int16"] == 0 and by[(q, q)]["sha256"] == fx["corpus_sha256"]  # identity
    names = sorted(RC.images())
    assert sorted({s["image"] for s in fx["streams"]}) == names and len(fx["streams"]) == len(names) * len(RC.STREAM_Q_FROM)
    for s in fx["streams"]:
        assert sorted(int(q) for q in s["to"]) == sorted(RC.STREAM_Q_TO)
        for q, rec in s["to"].items():
            assert set(rec) == {"default", "adaptive"} and all(("raises" in r) != ("sha256" in r) for r in rec.values())
            if int(q) == s["from"]:
                assert (rec["default"]["bytes"], rec["default"]["sha256"]) == (s["bytes"], s["sha256"])  # identity, as a stream
    for name, q in RC.SIZE_TABLES:
        t = fx["size_tables"]["%s@%d" % (name, q)]
        assert len(t) == 100 and all(v == -1 or v >= 16 for v in t[1:])
    assert any(v == -1 for t in fx["size_tables"].values() for v in t[1:])  # a quality without a stream is in the tables


def test_model_matches_the_reference_and_the_mutants_do_not():
    """The plain numpy model reproduces every digest and count of the fixture; the mutant that lets the table value cancel (exact
    rational arithmetic) and the one that rounds halves away from zero differ from the reference by exactly the recorded counts."""
    fx = RC.load_fixture()
    zz = RC.corpus()
    told_apart = {"rational": 0, "away": 0}
    for p in fx["pairs"]:
        q1, q2 = p["from"], p["to"]
        r = RC.model(zz, q1, q2)
        assert RC.digest(r) == p["sha256"] and RC.digest(r[:RC.N_LATIN]) == p["sha256_latin"], (q1, q2)
        assert RC.outside_int16(r) == p["outside_int16"] and RC.outside_int16(r[:RC.N_LATIN]) == p["outside_int16_latin"], (q1, q2)
        rat, tie = RC.model_rational(zz, q1, q2)
        assert int(tie.sum()) == p["ties"] and int((rat != r).sum()) == p["rational_differs"], (q1, q2)
        away = RC.model(zz, q1, q2, "away")
        assert int((away != r).sum()) == p["away_differs"], (q1, q2)
        told_apart["rational"] += RC.digest(rat) != p["sha256"]
        told_apart["away"] += RC.digest(away) != p["sha256"]
    assert told_apart["rational"] > 50 and told_apart["away"] > 50, told_apart


def test_streams_of_the_fixture_from_the_oracle(oracle):
    """The requantised default-table streams are oracle.entropy_encode of the model's arrays on the library's own host reader's input:
    the source streams are the oracle's, the coefficients the oracle's encode_zz16."""
    fx = RC.load_fixture()
    imgs = RC.images()
    for s in fx["streams"]:
        img = imgs[s["image"]]
        src = oracle.compress(img, s["from"])
        assert (len(src), RC.sha(src)) == (s["bytes"], s["sha256"])
        zz = oracle.encode_zz16(img, s["from"])
        hdr = {"height": s["h"], "width": s["w"], "quality": s["from"]}
        for q, rec in s["to"].items():
            info = RC.requantized_info(zz, hdr, int(q))
            out = oracle.entropy_encode(info["dc"], info["ac"], s["h"], s["w"], int(q))
            assert (len(out), RC.sha(out)) == (rec["default"]["bytes"], rec["default"]["sha256"]), (s["image"], s["from"], q)


def test_symbols_are_declared_exported_and_bound():
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(tic_\w+)\s*\(", text))
    assert declared == set(N.REQUANT_SIGNATURES) == set(NAMES)
    for other in (N.SIGNATURES, N.RATE_ADAPTIVE_SIGNATURES, N.TRANSCODE_SIGNATURES, N.TRANSCODE_BATCH_SIGNATURES, N.WIDE_SIGNATURES):
        assert not declared & set(other)
    assert '#include "tinyimgcodec_hip.h"' in text
    for path in (N.LIB_PATH, N.HOOKS_LIB_PATH):
        lib = C.CDLL(path)
        for name in declared:
            assert hasattr(lib, name), (path, name)
    L = N.load()
    for name in declared:
        assert getattr(L, name).argtypes == N.REQUANT_SIGNATURES[name][1]
    for name in ("requantize_zz", "requantize", "requantized_sizes", "requantize_to_size", "last_requantize"):
        assert callable(getattr(T, name)), name
    # nobody but tic_api.hip includes the new header, and the older headers do not know it
    for root, _, files in os.walk(os.path.join(ROOT, "tinyimgcodec_amd", "csrc")):
        for fn in files:
            if fn.endswith((".h", ".hip", ".cpp")) and fn != "tic_api.hip":
                with open(os.path.join(root, fn)) as f:
                    assert "tinyimgcodec_hip_requantize.h" not in f.read(), fn
    with open(os.path.join(ROOT, "tinyimgcodec_amd", "csrc", "tic_api.hip")) as f:
        assert "tinyimgcodec_hip_requantize.h" in f.read()
    for older in os.listdir(os.path.join(ROOT, "include")):
        if older != "tinyimgcodec_hip_requantize.h":
            with open(os.path.join(ROOT, "include", older)) as f:
                assert "requantize" not in f.read(), older
    with open(os.path.join(ROOT, "tinyimgcodec_amd", "csrc", "Makefile")) as f:
        assert "tic_requant_gpu.hip" in f.read()


def test_every_call_is_an_argument_error_without_a_context():
    L = N.load()
    s = np.zeros(64, np.uint8)
    zz = np.ones((2, 64), np.int16)
    out = np.zeros(4096, np.uint8)
    n, q = C.c_size_t(77), C.c_int(-5)
    one, qq, rng = (C.c_size_t * 1)(1), (C.c_int * 1)(50), (C.c_int * 1)(9)
    sizes = np.full(1, 123, np.int64)
    assert L.tic_requantize_zz(None, zz.ctypes.data, 2, 50, 25, out.ctypes.data) == N.TIC_E_ARG
    assert L.tic_requantize_zz_dev(None, zz.ctypes.data, 2, 50, 25, out.ctypes.data) == N.TIC_E_ARG
    assert L.tic_requantize_zz_v_dev(None, zz.ctypes.data, 2, 1, (C.c_size_t * 1)(0), one, qq, qq, out.ctypes.data, 2, rng) == N.TIC_E_ARG
    assert L.tic_requantize(None, s.ctypes.data, 64, 50, 0, out.ctypes.data, out.size, C.byref(n)) == N.TIC_E_ARG
    assert L.tic_requantized_sizes(None, s.ctypes.data, 64, qq, 1, sizes.ctypes.data) == N.TIC_E_ARG
    assert L.tic_requantize_to_size(None, s.ctypes.data, 64, 1000, 1, 0, out.ctypes.data, out.size, C.byref(n), C.byref(q)) == N.TIC_E_ARG
    assert L.tic_requant_kernels_timed(None, zz.ctypes.data, 2, 50, qq, 1, 1, 0, 1, C.byref(C.c_float(0)), sizes.ctypes.data) == N.TIC_E_ARG
    assert L.tic_last_requantize(None, C.byref(q), None, None, None) == N.TIC_E_ARG
    assert (out == 0).all() and n.value == 77 and q.value == -5 and rng[0] == 9 and sizes[0] == 123


def test_the_plan_under_the_sanitizers(tmp_path):
    """tests/native/requant_plan_selftest.cpp: job tables of 1..64 jobs with block counts around every chunk, round and group boundary, walked
    as the kernel walks them - every destination block written once, nothing outside the buffers -, every refusal, the passes of a quality
    list; and the form that shows the sweep can fail."""
    assert shutil.which("g++") is not None, "the plan sweep needs a host compiler: it is not skipped"
    exe = tmp_path / "requant_plan_selftest"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-pthread", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "requant_plan_selftest.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "requant_plan_selftest ok 740 cases" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([str(exe), "--break-stride"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "FAILED" in r.stdout and "Sanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def test_the_plan_header_is_free_of_hip_and_of_the_context():
    with open(os.path.join(ROOT, "tinyimgcodec_amd", "csrc", "tic_requant_plan.h")) as f:
        text = f.read()
    assert "hip_runtime" not in text and "tic_ctx" not in text and "hipStream" not in text


def head(h, w, q, flag):
    return struct.pack("<IIII", h & 0xFFFFFFFF, w & 0xFFFFFFFF, q & 0xFFFFFFFF, flag) + bytes(40)


class NoContext:
    """Stands where a context would: a check that reaches it has not run before _ctx(ctx)."""

    def __getattr__(self, name):
        raise AssertionError("the call reached the device (ctx.%s) before its checks" % name)


def test_python_checks_come_first():
    nc = NoContext()
    good = head(8, 8, 50, 0)
    calls = (lambda s: T.requantize(s, 25, ctx=nc), lambda s: T.requantize(s, 25, adaptive=True, ctx=nc), lambda s: T.requantized_sizes(s, [25], ctx=nc),
             lambda s: T.requantize_to_size(s, 100, ctx=nc))
    refused = [(bytes(15), struct.error), (head(8, 8, 50, 1 << 31), ValueError), (head(8, 8, 3, 1 << 30), ValueError), (head(-8, 8, 50, 0), ValueError),
               (head(8, -8, 50, 0), ValueError), (head(8, 8, 0, 0), ValueError), (head(8, 8, 100, 0), ValueError)]
    for call in calls:
        for s, cls in refused:
            with pytest.raises(cls):
                call(s)
    # qualities: compress()'s exceptions, before any device work
    for q, cls in ((0, ZeroDivisionError), (-1, struct.error), (100, KeyError), (101, ValueError), (50.5, struct.error), ("50", TypeError)):
        with pytest.raises(cls):
            T.requantize(good, q, ctx=nc)
        with pytest.raises(cls):
            T.requantized_sizes(good, [25, q], ctx=nc)
        with pytest.raises(cls):
            T.requantize_to_size(good, 100, min_quality=q, ctx=nc)
        with pytest.raises(cls):
            T.requantize_to_size(good, 100, max_quality=q, ctx=nc)
        with pytest.raises(cls):
            T.requantize_zz(np.zeros((1, 64), np.int16), q, 50, ctx=nc)
        with pytest.raises(cls):
            T.requantize_zz(np.zeros((1, 64), np.int16), 50, q, ctx=nc)
    with pytest.raises(ValueError):
        T.requantize_to_size(good, 100, min_quality=60, ctx=nc)  # above the stream's own quality, the default ceiling
    with pytest.raises(ValueError):
        T.requantize_to_size(good, -1, ctx=nc)
    with pytest.raises(IndexError):
        T.requantize(head(0, 8, 50, 0), 25, adaptive=True, ctx=nc)
    with pytest.raises(ValueError):
        T.requantize_zz(np.zeros((3, 63), np.int16), 50, 25, ctx=nc)
    assert T.requantize_zz(np.zeros((0, 64), np.int16), 50, 25, ctx=nc).shape == (0, 64)
    assert T.requantized_sizes(good, [], ctx=nc).shape == (0,)


def test_the_cli_parses_before_it_imports_the_device_path(capsys):
    from tinyimgcodec_amd import requantize_cli

    for argv in (["in", "out"], ["in", "out", "--quality", "5", "--max-bytes", "9"], ["in", "out", "--max-bytes", "9", "--adaptive"]):
        with pytest.raises(SystemExit) as e:
            requantize_cli.main(argv)
        assert e.value.code == 2
    capsys.readouterr()
