"""The scaled-DCT encoder (the reference's standalone integer encoder, c/img.c + c/encode.c) - everything that needs no GPU.

Fixtures: tests/golden/scaled_encode.npz / .json, made by tests/golden/gen/make_goldens_scaled_enc.py from the unmodified reference
(its C program's output cut behind the last block, read back with its own Python bit reader).  Every byte checked here is the
reference's."""
import ctypes as C
import hashlib
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SETTINGS = ("best", "high", "med", "low")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(GOLDEN, "scaled_encode.json")) as f:
        man = json.load(f)
    return np.load(os.path.join(GOLDEN, "scaled_encode.npz")), man


def case_image(npz, key):
    if key.startswith("lenna512_"):
        return np.load(os.path.join(GOLDEN, "lenna.npz"))["img"]
    return npz[key + "_img"]


def full(npz, key, suffix):
    """The whole array of a fixture, or None when only its head is stored (then the manifest's sha256 and length pin it)."""
    name = "%s_%s" % (key, suffix)
    return npz[name] if name in npz.files else None


def test_fixture_set_is_what_the_issue_lists(fx):
    npz, man = fx
    cases = man["cases"]
    for name in ("flat8x8", "noise16x24", "noise64x96", "ramp48x48", "highfreq8x16", "lenna512", "empty0x0"):
        for s in SETTINGS:
            assert "%s_%s" % (name, s) in cases
    assert "twolevel64x64_best" in cases
    for s in SETTINGS:
        m = cases["aligned_%s_%s" % (s, s)]
        assert m["payload_bits"] % 8 == 0 and m["bytes"] == 16 + m["payload_bits"] // 8 + 1  # one byte longer than ceil(P / 8)
        assert cases["flat8x8_" + s]["payload_bits"] == 6 and cases["flat8x8_" + s]["bytes"] == 17
        assert cases["empty0x0_" + s]["bytes"] == 17
        hf = cases["highfreq8x16_" + s]
        # (at `low` the largest 63rd coefficient an 8-bit block can have quantises to 0: the generator's note)
        assert hf["zrl_symbols"] > 0 and (hf["blocks_ending_in_63"] > 0) == (s != "low")
    assert all(m["max_abs_ac"] <= 1023 for m in cases.values())
    assert sorted(npz["names"].tolist()) == sorted(cases)


def test_entropy_encode_scaled_matches_the_reference_streams(fx):
    """entropy_encode_scaled on the reference's coefficients = the reference's stream, byte for byte: header (setting, flag 00 00 00 40),
    payload, flush byte - also when the payload ends on a byte boundary (one zero byte more) and for the 17-byte empty stream."""
    npz, man = fx
    L = N.load()
    for key, m in man["cases"].items():
        zz = full(npz, key, "zz")
        if zz is None:
            continue  # (Lenna: the coefficients are pinned by digest; test_host_arithmetic_... recomputes them and goes on to the stream)
        got = T.entropy_encode_scaled(zz, m["h"], m["w"], m["setting"])
        assert len(got) == m["bytes"] == 16 + m["payload_bits"] // 8 + 1, key
        assert sha(np.frombuffer(got, np.uint8)) == m["sha256"], key
        want = full(npz, key, "bs")
        if want is not None:
            assert got == want.tobytes(), key
        assert struct.unpack("<IIII", got[:16]) == (m["h"], m["w"], SETTINGS.index(m["setting"]), 1 << 30)
        assert got == T.entropy_encode_scaled(zz, m["h"], m["w"], SETTINGS.index(m["setting"]))  # 0..3 as well
        assert L.tic_compress_scaled_bound(m["h"], m["w"]) >= len(got)
    assert T.entropy_encode_scaled(np.zeros((0, 64), np.int16), 0, 0, "best").hex() == "00000000000000000000000000000040" + "00"


def test_host_arithmetic_of_the_kernel_matches_the_reference_coefficients(fx, tmp_path):
    """tic_scaled_math.h - the butterflies, the int16 truncations, the reciprocal quantiser and the table the gfx950 kernel is built
    from - compiled for the host (with sanitizers) reproduces the reference's coefficients for every fixture, Lenna included; from
    those, entropy_encode_scaled gives Lenna's reference streams."""
    npz, man = fx
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = tmp_path / "scaled_selftest"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "scaled_selftest.cpp")], check=True)
    for key, m in man["cases"].items():
        img = case_image(npz, key)
        h, w = m["h"], m["w"]
        blocks = img.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64) if img.size else np.zeros((0, 64), np.uint8)
        fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
        fin.write_bytes(struct.pack("<ii", blocks.shape[0], SETTINGS.index(m["setting"])) + np.ascontiguousarray(blocks).tobytes())
        r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "scaled_selftest ok" in r.stdout, r.stdout + r.stderr
        zz = np.fromfile(str(fout), np.int16).reshape(-1, 64)
        assert sha(zz) == m["zz_sha256"], key
        want = full(npz, key, "zz")
        assert np.array_equal(zz, want if want is not None else zz), key
        if want is None:
            assert np.array_equal(zz[:64], npz[key + "_zz_head"]), key
            got = T.entropy_encode_scaled(zz, h, w, m["setting"])
            assert len(got) == m["bytes"] and sha(np.frombuffer(got, np.uint8)) == m["sha256"], key
            bs = full(npz, key, "bs")
            assert got == bs.tobytes() if bs is not None else np.array_equal(np.frombuffer(got[:4096], np.uint8), npz[key + "_bs_head"]), key


def test_scaled_errors_and_bound():
    L = N.load()
    zz = np.zeros((2, 64), np.int16)
    out = np.empty(1024, np.uint8)
    n = C.c_size_t()

    def enc(h, w, qf, cap, z=zz):
        return L.tic_entropy_encode_scaled(z.ctypes.data, h, w, qf, out.ctypes.data, cap, C.byref(n))

    assert enc(8, 16, 4, 1024) == N.TIC_E_QUALITY and enc(8, 16, -1, 1024) == N.TIC_E_QUALITY
    assert enc(8, 12, 2, 1024) == N.TIC_E_ARG and enc(9, 16, 2, 1024) == N.TIC_E_ARG and enc(-8, 16, 2, 1024) == N.TIC_E_ARG
    assert enc(8, 16, 2, 1024) == N.TIC_OK and n.value == 18  # 2 x (DC 00 + EOB 1010) = 12 bits: one whole byte + the flush byte
    assert enc(8, 16, 2, 17) == N.TIC_E_SPACE  # one short of the length
    assert enc(8, 16, 2, 18) == N.TIC_OK
    al = np.zeros((4, 64), np.int16)  # 4 x 6 bits = 24 bits: the payload ends on a byte boundary, the flush byte is 00
    assert enc(16, 16, 0, 1024, al) == N.TIC_OK and n.value == 16 + 3 + 1 and out[19] == 0
    assert enc(16, 16, 0, 19, al) == N.TIC_E_SPACE  # ... and is counted: one short of the length
    for h, w in ((0, 0), (8, 8), (1080, 1920), (4096, 4096)):
        assert L.tic_compress_scaled_bound(h, w) == L.tic_compress_bound(h, w) + 1
    bad = np.zeros((1, 64), np.int16)
    bad[0, 5] = 1024  # category 11: the C encoder's tables end at 10
    with pytest.raises(KeyError):
        T.entropy_encode_scaled(bad, 8, 8, "best")
    bad[0, 5] = -1023
    assert len(T.entropy_encode_scaled(bad, 8, 8, "best")) > 17
    dc = np.zeros((2, 64), np.int16)
    dc[1, 0] = 2048  # DC difference of category 12
    with pytest.raises(KeyError):
        T.entropy_encode_scaled(dc, 8, 16, "low")
    for q in ("good", 4, -1, 2.0, None, True):
        with pytest.raises(ValueError):
            T.entropy_encode_scaled(zz, 8, 16, q)
    with pytest.raises(ValueError):
        T.entropy_encode_scaled(zz, 8, 12, "med")
    with pytest.raises(ValueError):
        T.entropy_encode_scaled(zz, 8, 8, "med")  # 2 blocks of coefficients for a 1-block frame


def test_oracle_decodes_every_fixture_stream_to_the_reference_pixels(fx, oracle):
    """The existing oracle's decompress() (it reads flag 1 << 30) of every fixture stream = what the reference's decompress() gave."""
    npz, man = fx
    for key, m in man["cases"].items():
        bs = full(npz, key, "bs")
        if bs is None or m["h"] == 0:
            continue
        dec = oracle.decompress(bs.tobytes())
        assert dec.shape == (m["h"], m["w"]) and sha(dec) == m["dec_sha256"], key
        want = full(npz, key, "dec")
        if want is not None:
            assert np.array_equal(dec, want), key
