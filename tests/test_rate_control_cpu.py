"""Rate control without a GPU: the host size function (tic_entropy_size / entropy_size) against stream lengths recorded from the
unmodified reference (tests/golden/rate_control.json, written by tests/golden/gen/make_goldens_rate.py) and against the host encoder."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

from conftest import rand_frame

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IMAGES = ("lenna", "bench01", "bench17", "bench40", "bench06_crop203x317", "noise256_seed7")


def load_fixture():
    with open(os.path.join(GOLDEN, "rate_control.json")) as f:
        return json.load(f)


def fixture_image(name):
    """The pixels of a fixture entry (its "pixels" field says the same in words)."""
    if name == "lenna":
        return np.load(os.path.join(GOLDEN, "lenna.npz"))["img"]
    if name == "noise256_seed7":
        return rand_frame(7, 256, 256)
    px = np.load(os.path.join(GOLDEN, "benchmark_set.npz"))["pixels"]
    if name == "bench06_crop203x317":
        return np.ascontiguousarray(px[5][:203, :317])
    return px[int(name[5:]) - 1]


def test_fixture_is_the_references():
    """The generator is named, every entry comes from the reference, and holds what the issue asks for: 99 sizes per image, the first
    encodable, null only at the top of the range (Lenna and images 1 and 17 from q = 98, the others at q = 99)."""
    fx = load_fixture()
    assert fx["generator"] == "tests/golden/gen/make_goldens_rate.py"
    assert os.path.exists(os.path.join(os.path.dirname(GOLDEN), "..", fx["generator"]))
    assert set(fx["images"]) == set(IMAGES)
    for name, e in fx["images"].items():
        assert e["source"] == "reference", name
        img = fixture_image(name)
        assert img.shape == (e["h"], e["w"]) and img.dtype == np.uint8, name
        s = e["sizes"]
        assert len(s) == 99 and s[0] is not None
        first_null = s.index(None) + 1 if None in s else 100
        assert first_null == (98 if name in ("lenna", "bench01", "bench17") else 99), name
        assert all(v is None for v in s[first_null - 1:]) and all(isinstance(v, int) and v >= 16 for v in s[: first_null - 1])
    lenna = fx["images"]["lenna"]["sizes"]
    assert (lenna[0], lenna[49], lenna[96]) == (3322, 20765, 120734)
    assert fx["images"]["bench40"]["sizes"][97] == 136813 and fx["images"]["noise256_seed7"]["sizes"][97] == 87909


@pytest.mark.parametrize("name", IMAGES)
def test_entropy_size_equals_the_reference_size(oracle, name):
    """entropy_size of the oracle's coefficients == len(reference compress(img, q)) for every recorded quality; KeyError for null."""
    e = load_fixture()["images"][name]
    img = fixture_image(name)
    for q in range(1, 100):
        zz = oracle.encode_zz16(img, q)
        want = e["sizes"][q - 1]
        if want is None:
            with pytest.raises(KeyError):
                T.entropy_size(zz, e["h"], e["w"])
            with pytest.raises(KeyError):  # ... exactly where the encoder fails
                T.entropy_encode(zz, e["h"], e["w"], q)
        else:
            assert T.entropy_size(zz, e["h"], e["w"]) == want, (name, q)


def test_entropy_size_equals_the_encoder_on_small_and_ragged_shapes(oracle, golden):
    """... and len(entropy_encode(...)) on the 1x1 ... 15x17 and ragged shapes of transform_small.npz (KeyError where it has none)."""
    s = golden("transform_small")
    n = 0
    for key in s["names"]:
        img = s[key + "_img"]
        q = int(str(key).rsplit("_q", 1)[1])
        zz = oracle.encode_zz16(img, q)
        h, w = img.shape
        if s[key + "_bs"].size:
            assert T.entropy_size(zz, h, w) == len(T.entropy_encode(zz, h, w, q)) == s[key + "_bs"].size, key
        else:
            with pytest.raises(KeyError):
                T.entropy_size(zz, h, w)
        n += 1
    assert n >= 10


def test_entropy_size_walk_known_answers():
    """ZRLs, a coefficient in the last position, the first block's raw DC, and the limits of the code tables (DC category 11, AC size 10)."""
    zz = np.zeros((1, 64), np.int16)
    assert T.entropy_size(zz, 8, 8) == 17  # DC category 0 (2 bits) + EOB (4 bits)
    zz[0, 63] = -3  # 3 x ZRL (11 bits each) + (14, 2) (16 bits) + 2 value bits + EOB: 2 + 33 + 18 + 4 = 57 bits
    assert T.entropy_size(zz, 8, 8) == 16 + 8 == len(T.entropy_encode(zz, 8, 8, 50))
    rng = np.random.default_rng(11)
    zz = rng.integers(-1023, 1024, (6, 64)).astype(np.int16)
    zz[:, 0] = [1000, -1000, 1047, -1000, 0, 5]  # differences up to 2047: category 11
    zz[rng.random((6, 64)) < 0.6] = 0
    zz[2, 1:] = 0
    assert T.entropy_size(zz, 16, 24) == len(T.entropy_encode(zz, 16, 24, 50))
    for bad in ((0, 5, 1024), (3, 40, -1024), (1, 0, 2048 + 1000), (5, 63, -32768)):
        z = zz.copy()
        z[bad[0], bad[1]] = bad[2]
        with pytest.raises(KeyError):
            T.entropy_size(z, 16, 24)
        with pytest.raises(KeyError):
            T.entropy_encode(z, 16, 24, 50)
    assert T.entropy_size(np.zeros((0, 64), np.int16), 0, 8) == 16 == len(T.entropy_encode(np.zeros((0, 64), np.int16), 0, 8, 50))


def test_entropy_size_arguments():
    L = N.load()
    n = C.c_size_t(0)
    zz = np.zeros((4, 64), np.int16)
    assert L.tic_entropy_size(zz.ctypes.data, 16, 16, None) == N.TIC_E_ARG
    assert L.tic_entropy_size(None, 16, 16, C.byref(n)) == N.TIC_E_ARG
    assert L.tic_entropy_size(zz.ctypes.data, -1, 16, C.byref(n)) == N.TIC_E_ARG
    assert L.tic_entropy_size(None, 0, 16, C.byref(n)) == N.TIC_OK and n.value == 16
    with pytest.raises(ValueError):
        T.entropy_size(zz, 16, 24)  # 6 blocks expected
    with pytest.raises(ValueError):
        T.entropy_size(zz, -16, 16)


def test_rate_control_arguments_fail_before_any_gpu_work():
    """Quality and image checks of the GPU entry points' Python mirror raise what compress() raises, without touching a device."""
    import struct

    img = np.zeros((16, 16), np.uint8)
    for fn in (lambda q: T.compressed_size(img, q), lambda q: T.compressed_sizes(img, [50, q]), lambda q: T.compress_to_size(img, 1000, q, 99),
               lambda q: T.compress_to_size(img, 1000, 1, q)):
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
    with pytest.raises(ValueError):
        T.compress_to_size(img, 1000, 60, 20)
    with pytest.raises(ValueError):
        T.compressed_size(np.full((8, 8), 300, np.int32))  # 8-bit images only, as compress_batch
    with pytest.raises(ValueError):
        T.compress_to_size(np.full((8, 8), -1, np.int32), 1000)
    assert T.compressed_sizes(img, []).shape == (0,)
