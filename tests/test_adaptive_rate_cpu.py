"""Rate control for per-image Huffman tables without a GPU: the host size functions (tic_entropy_size_adaptive, tic_adaptive_stream_size)
against stream lengths recorded from the unmodified reference (tests/golden/adaptive_rate.json, adaptive_streams.json), the numpy model of
the statistics the GPU tests compare the kernels with, the bisection replayed in Python, the host walk and the probe plan under the
sanitizers, and the exported symbols."""
import ctypes as C
import hashlib
import heapq
import os
import shutil
import subprocess

import numpy as np
import pytest

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

import adaptive_rate_common as A
from conftest import ROOT

NEW_HEADER = os.path.join(ROOT, "include", "tinyimgcodec_hip_adaptive_rate.h")
# (as of tic_test_live_buffers, the one declaration added since, and of the comment that states tic_encode_wide's domain: no declaration changed)
MAIN_HEADER_SHA256 = "d741e5ea2c521752073e710248c65039770ea26203d95b495e3f0c47f76d071a"


def test_fixture_is_the_references():
    fx = A.adaptive_rate()
    assert fx["generator"] == "tests/golden/gen/make_goldens_adaptive_rate.py" and sorted(fx["images"]) == sorted(A.IMAGES)
    nonnull = 0
    for name in A.IMAGES:
        e = fx["images"][name]
        assert e["source"] == "reference" and len(e["sizes"]) == 99 and A.fixture_image(name).shape == (e["h"], e["w"])
        assert all((s is None) == (str(q + 1) in e["raises"]) for q, s in enumerate(e["sizes"]))
        nonnull += sum(s is not None for s in e["sizes"])
    assert nonnull == 594


def test_the_vectorised_model_is_the_list_s():
    """model_stats (numpy) == model_stats_slow (the run-length list of huffman.py:12-33, block by block) on every built block and on noise."""
    frames = dict(A.edge_blocks())
    frames["noise"] = A.noise_blocks(11, 300)
    frames["dense"] = A.noise_blocks(12, 65, density=0.95, amp=3000)
    for name, zz in frames.items():
        a, b = A.model_stats(zz), A.model_stats_slow(zz)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], name
    assert A.model_stats(frames["ac_minus_32768"])[2] and A.model_stats(frames["dc_step_65535"])[2] and not A.model_stats(frames["sizes_1_to_15"])[2]


def _both_sizes(zz, h, w):
    """entropy_size_adaptive of the coefficients, and tic_adaptive_stream_size of the model's statistics: they must agree."""
    walk = T.entropy_size_adaptive(zz, h, w)
    count, first, err = A.model_stats(zz)
    rc, n = A.stats_size(N.load(), count, first)
    assert not err and rc == N.TIC_OK and n == walk, (walk, rc, n)
    return walk


@pytest.mark.parametrize("name", A.IMAGES)
def test_entropy_size_adaptive_equals_the_reference_size(oracle, name):
    """== len(reference compress(img, q, auto_generate_huffman_table=True)) for every recorded quality, by the walk and by the statistics."""
    e = A.adaptive_rate()["images"][name]
    img = A.fixture_image(name)
    for q in range(1, 100):
        want = e["sizes"][q - 1]
        zz = oracle.encode_zz16(img, q)
        if want is None:
            with pytest.raises(OverflowError):
                T.entropy_size_adaptive(zz, e["h"], e["w"])
        else:
            assert _both_sizes(zz, e["h"], e["w"]) == want, (name, q)


def test_entropy_size_adaptive_on_the_benchmark_table(oracle):
    """The 294 lengths of the reference's benchmark (49 images x 6 qualities) with per-image tables."""
    px, done = A.bench_pixels(), 0
    for e in A.adaptive_streams()["benchmark"]:
        img = px[e["image"] - 1]
        assert _both_sizes(oracle.encode_zz16(img, e["quality"]), img.shape[0], img.shape[1]) == e["bytes"], (e["image"], e["quality"])
        done += 1
    assert done == 294


def test_entropy_size_adaptive_on_the_small_cases(oracle):
    """Every case with blocks: 1 x 1, ragged, flat (one symbol: codes of length 0), noise up to q = 99, the 0/255 checkerboards, 1080p."""
    cases = A.cases_with_blocks()
    assert len(cases) == 30
    for name, img, q, want in cases:
        assert _both_sizes(oracle.encode_zz16(img, q), img.shape[0], img.shape[1]) == want, (name, q)


def test_crafted_tables_give_back_their_own_bit_counts():
    """The crafted tables of adaptive_streams.json: tic_adaptive_stream_size of their counts and first positions == 16 + ceil((the reference's
    serialized table bits + sum of count x (the reference's code length + value bits)) / 8)."""
    L = N.load()
    tables = A.adaptive_streams()["tables"]
    assert len(tables) == 6
    for t in tables:
        count, first = np.zeros(A.BINS, np.uint64), np.full(A.BINS, A.NEVER, np.uint64)
        for c, n, f in t["dc"]:
            count[A.DC_BIN + c], first[A.DC_BIN + c] = n, f
        for s, n, f in t["ac"]:
            count[s], first[s] = n, f
        dc_len, ac_len = {c: len(code) for c, code in t["dc_codes"]}, {s: len(code) for s, code in t["ac_codes"]}
        bits = int(t["table_bits"]) + sum(n * (dc_len[c] + c) for c, n, _ in t["dc"]) + sum(n * (ac_len[s] + (s & 15)) for s, n, _ in t["ac"])
        assert A.stats_size(L, count, first) == (N.TIC_OK, 16 + (bits + 7) // 8), t["name"]


class _Node:
    """HuffmanTree.__Node (huffman.py:110-128): ordered by frequency alone."""

    def __init__(self, freq, sym=None, left=None, right=None):
        self.freq, self.sym, self.left, self.right = freq, sym, left, right

    def __lt__(self, other):
        return self.freq < other.freq


def _code_lengths(counts_in_first_order):
    """Code length per symbol of the reference's tree (huffman.py:137-194): leaves into a heap in first-occurrence order, the two smallest
    merged until one is left."""
    heap = []
    for sym, n in counts_in_first_order:
        heapq.heappush(heap, _Node(n, sym))
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, _Node(a.freq + b.freq, None, a, b))
    out, stack = {}, [(heap[0], 0)]
    while stack:
        node, depth = stack.pop()
        if node.sym is not None:
            out[node.sym] = depth
        else:
            stack += [(node.left, depth + 1), (node.right, depth + 1)]
    return out


def _fibonacci_stats(nsyms, rarest_size):
    """AC symbols with Fibonacci counts, the rarest first and of size `rarest_size`, all others of sizes 1..4 (so that the rarest symbol's
    code and value bits are the longest); one DC category."""
    fib = [1, 1]
    while len(fib) < nsyms:
        fib.append(fib[-1] + fib[-2])
    syms = [(0 << 4) | rarest_size] + [(r << 4) | s for s in range(1, 5) for r in range(16)][: nsyms - 1]
    assert len(syms) == nsyms == len(set(syms)) and rarest_size > 4
    count, first = np.zeros(A.BINS, np.uint64), np.full(A.BINS, A.NEVER, np.uint64)
    for k, s in enumerate(syms):
        count[s], first[s] = fib[k], k
    count[A.DC_BIN + 2], first[A.DC_BIN + 2] = 5, 0
    return count, first, [(s, fib[k]) for k, s in enumerate(syms)]


def test_built_statistics():
    L = N.load()
    # one symbol each: codes of length 0, DC category 0 and the EOB carry no value bits - header and table only
    count, first = np.zeros(A.BINS, np.uint64), np.full(A.BINS, A.NEVER, np.uint64)
    count[A.DC_BIN], first[A.DC_BIN], count[0], first[0] = 9, 0, 9, 0
    table_bits = 16 + (4 + 4 + 0) + 16 + (8 + 8 + 0)
    assert A.stats_size(L, count, first) == (N.TIC_OK, 16 + (table_bits + 7) // 8)
    # ... and with value bits: 9 x category 3
    count[A.DC_BIN], first[A.DC_BIN], count[A.DC_BIN + 3], first[A.DC_BIN + 3] = 0, A.NEVER, 9, 0
    assert A.stats_size(L, count, first) == (N.TIC_OK, 16 + (table_bits + 27 + 7) // 8)
    # Fibonacci counts: the rarest symbol's code has nsyms - 1 bits; with its value bits exactly 64 is taken, 65 is not
    for nsyms, size, want in ((50, 15, N.TIC_OK), (51, 15, N.TIC_E_RANGE), (51, 14, N.TIC_OK), (52, 14, N.TIC_E_RANGE)):
        count, first, order = _fibonacci_stats(nsyms, size)
        lens = _code_lengths(order)
        longest = max(lens[s] + (s & 15) for s in lens)
        assert lens[order[0][0]] == nsyms - 1 and longest == nsyms - 1 + size and (longest <= 64) == (want == N.TIC_OK), (nsyms, size, longest)
        rc, n = A.stats_size(L, count, first)
        assert rc == want, (nsyms, size, rc)
        if rc == N.TIC_OK:  # the identity, with the model's lengths (the table: 16 + 8 + 16 + per AC symbol 16 + its code)
            tb = 16 + 8 + 16 + sum(16 + lens[s] for s in lens)
            assert n == 16 + (tb + 5 * 2 + sum(c * (lens[s] + (s & 15)) for s, c in order) + 7) // 8
    # empty histograms
    count, first = np.zeros(A.BINS, np.uint64), np.full(A.BINS, A.NEVER, np.uint64)
    assert A.stats_size(L, count, first)[0] == N.TIC_E_ARG
    count[A.DC_BIN + 1], first[A.DC_BIN + 1] = 1, 0
    assert A.stats_size(L, count, first)[0] == N.TIC_E_ARG  # no AC symbol
    n = C.c_size_t(0)
    assert L.tic_adaptive_stream_size(None, None, None, None, C.byref(n)) == N.TIC_E_ARG
    assert L.tic_adaptive_stream_size(count.ctypes.data, first.ctypes.data, count.ctypes.data, first.ctypes.data, None) == N.TIC_E_ARG


def test_entropy_size_adaptive_arguments():
    L = N.load()
    zz = np.zeros((4, 64), np.int16)
    n = C.c_size_t(0)
    assert L.tic_entropy_size_adaptive(zz.ctypes.data, 16, 16, None) == N.TIC_E_ARG
    assert L.tic_entropy_size_adaptive(None, 16, 16, C.byref(n)) == N.TIC_E_ARG
    assert L.tic_entropy_size_adaptive(zz.ctypes.data, -1, 16, C.byref(n)) == N.TIC_E_ARG
    assert L.tic_entropy_size_adaptive(zz.ctypes.data, 0, 16, C.byref(n)) == N.TIC_E_ARG  # no blocks: no table
    with pytest.raises(IndexError):
        T.entropy_size_adaptive(np.zeros((0, 64), np.int16), 0, 8)
    with pytest.raises(ValueError):
        T.entropy_size_adaptive(zz, 16, 24)  # 6 blocks expected
    with pytest.raises(ValueError):
        T.entropy_size_adaptive(zz, -16, 16)
    for name in ("ac_minus_32768", "dc_step_65535"):
        blocks = A.edge_blocks()[name]
        with pytest.raises(OverflowError):
            T.entropy_size_adaptive(blocks, 8, 8 * len(blocks))
    # a flat frame: one DC category twice... the first block's DC and zero differences behind it
    flat = np.zeros((4, 64), np.int16)
    flat[:, 0] = 77
    count, first, _ = A.model_stats(flat)
    assert T.entropy_size_adaptive(flat, 16, 16) == A.stats_size(L, count, first)[1]


def test_python_argument_checks_need_no_gpu():
    """What the Python mirror refuses before it asks for a context."""
    img = np.zeros((16, 16), np.uint8)
    for empty in (np.zeros((0, 8), np.uint8), np.zeros((8, 0), np.uint8)):
        with pytest.raises(IndexError):
            T.compressed_sizes_adaptive(empty, [50])
        with pytest.raises(IndexError):
            T.compressed_size_adaptive(empty, 50)
        with pytest.raises(IndexError):
            T.compress_adaptive_to_size(empty, 1000)
        with pytest.raises(IndexError):
            T.compressed_sizes_adaptive_batch([img, empty], [50])
    with pytest.raises(ZeroDivisionError):
        T.compressed_sizes_adaptive(img, [50, 0])
    with pytest.raises(KeyError):
        T.compressed_size_adaptive(img, 100)
    with pytest.raises(ValueError):
        T.compress_adaptive_to_size(img, 1000, 60, 10)
    with pytest.raises(ValueError):
        T.compress_adaptive_to_size(img, -1)
    with pytest.raises(ValueError):
        T.compressed_sizes_adaptive(np.full((8, 8), 300), [50])
    with pytest.raises(ValueError):
        T.compressed_sizes_adaptive_batch([img, np.full((8, 8), -1)], [50])
    assert T.compressed_sizes_adaptive_batch([], [50]).shape == (0, 1)


def test_replayed_bisection_gives_the_expected_qualities():
    """The table the GPU search test expects (adaptive_rate_common.EXPECTED) is what the bisection of the header gives on the recorded sizes."""
    fx = A.adaptive_rate()["images"]
    for name in A.IMAGES:
        sizes = fx[name]["sizes"]
        for qmin, qmax in A.RANGES:
            b = A.budgets(sizes, qmin)
            got = []
            for kind in A.BUDGET_KINDS:
                r = A.replay(sizes, b[kind], qmin, qmax)
                got.append("V" if r is ValueError else r[0])
            assert got == A.EXPECTED[name][(qmin, qmax)], (name, qmin, qmax, got)
    assert A.replay([None] * 99, 100, 1, 99) is OverflowError and A.replay(list(range(1, 100)), 50, 1, 99) == (50, 6)


def test_host_walk_and_probe_plan_under_the_sanitizers(tmp_path):
    """tests/native/adaptive_size_selftest.cpp: adaptive_host_stats, entropy_size_adaptive and adaptive_stream_size (csrc/tic_adaptive.cpp)
    on built blocks - runs of 15/16/17/31/32/47/48/62, an entry at index 63 only, all-zero blocks, DC differences of +-65535, an AC of
    -32768 - and the sweep of cap_probe_groups (csrc/tic_adaptive_rate_plan.h).  A stand-alone program, built with the address and
    undefined-behaviour sanitizers."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    if not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        pytest.skip("hip/hip_runtime.h is absent: tic_adaptive.h includes it")
    exe = tmp_path / "adaptive_size_selftest"
    csrc = os.path.join(ROOT, "tinyimgcodec_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "adaptive_size_selftest.cpp"), os.path.join(csrc, "tic_adaptive.cpp"),
                    os.path.join(csrc, "tic_entropy.cpp"), "-lpthread"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "adaptive_size_selftest ok" in r.stdout and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def test_the_plan_header_is_free_of_hip_and_the_probe_table_is_reused():
    with open(os.path.join(ROOT, "tinyimgcodec_amd", "csrc", "tic_adaptive_rate_plan.h")) as f:
        plan = f.read()
    assert "#include <hip" not in plan and '#include "tic_rate_plan.h"' in plan
    with open(os.path.join(ROOT, "tinyimgcodec_amd", "csrc", "tic_api.hip")) as f:
        api = f.read()
    assert "inline bool fill_" not in plan  # no table filler of its own: the statistics launches fill the size kernel's
    assert "fill_size_probe_table(&ctx->h_rate_tabs[t], l.count" in api


def test_new_symbols_are_declared_exported_and_bound():
    import re

    with open(NEW_HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(tic_\w+)\s*\(", text))
    assert declared == set(N.RATE_ADAPTIVE_SIGNATURES) and len(declared) == 9
    assert not declared & set(N.SIGNATURES)
    assert '#include "tinyimgcodec_hip.h"' in text
    for path in (N.LIB_PATH, N.HOOKS_LIB_PATH):
        lib = C.CDLL(path)
        for name in declared:
            assert hasattr(lib, name), (path, name)
    L = N.load()
    for name in declared:
        assert getattr(L, name).argtypes is not None
    for name in ("compressed_sizes_adaptive", "compressed_size_adaptive", "compress_adaptive_to_size", "compressed_sizes_adaptive_batch",
                 "entropy_size_adaptive"):
        assert callable(getattr(T, name)), name
    # nobody else includes the new header; without a context every call is an argument error
    for root, _, files in os.walk(os.path.join(ROOT, "tinyimgcodec_amd", "csrc")):
        for fn in files:
            if fn.endswith((".h", ".hip", ".cpp")) and fn != "tic_api.hip":
                with open(os.path.join(root, fn)) as f:
                    assert "tinyimgcodec_hip_adaptive_rate.h" not in f.read(), fn
    with open(os.path.join(ROOT, "include", "tinyimgcodec_hip.h")) as f:
        assert "adaptive_rate" not in f.read()
    assert L.tic_adaptive_sizes(None, None, 8, 8, 8, None, 0, None) == N.TIC_E_ARG
    assert L.tic_adaptive_sizes_v(None, None, 0, None, None, None, None, 0, None) == N.TIC_E_ARG
    assert L.tic_compress_adaptive_to_size(None, None, 8, 8, 8, 100, 1, 99, None, 0, None, None) == N.TIC_E_ARG
    assert L.tic_adaptive_stats_v_dev(None, None, 1, None, 0, 0, None, None, None) == N.TIC_E_ARG
    assert L.tic_last_adaptive_rate(None, None, None, None) == N.TIC_E_ARG


def test_the_main_header_is_untouched():
    with open(os.path.join(ROOT, "include", "tinyimgcodec_hip.h"), "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == MAIN_HEADER_SHA256
