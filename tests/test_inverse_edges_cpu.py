"""tests/golden/inverse_edges.npz on the CPU: the oracle decodes every built frame to what the unmodified reference decoded it to, by both of
its routes, and the fixture still has the properties that make it worth decoding (tests/golden/gen/make_goldens_inverse.py asserted them
when it ran the reference; here they are re-derived from the stored coefficients).  This is what lets tests/test_inverse_transform_gpu.py use
oracle.decompress as its live reference on a machine without the reference."""
import numpy as np
import pytest

import inverse_edges as IE


@pytest.fixture(scope="module")
def fx():
    return IE.Fixture()


@pytest.fixture(scope="module")
def decoded(fx, oracle):
    """name -> oracle.decompress of the frame's stream (every frame that has one), computed once."""
    out = {}
    for name in fx.names(streams_only=True):
        e = fx.frames[name]
        dc, ac = fx.coeffs(name)
        s = IE.stream_of(oracle, dc, ac, e["height"], e["width"], e["quality"], e["flag"])
        assert len(s) == e["stream_bytes"] and IE.sha(s) == e["stream_sha256"], name
        out[name] = oracle.decompress(s)
    return out


def test_the_fixture_holds_every_family(fx):
    fams = {e["family"] for e in fx.frames.values()}
    assert fams == {"sparse", "ragged", "extremes", "clip", "dense", "scaled", "wide"}
    assert {fx.frames[n]["quality"] for n in fx.names("sparse")} == {1, 10, 50, 75, 99, 37.5}
    assert {fx.frames[n]["quality"] for n in fx.names("scaled") if fx.frames[n]["blocks"] == 2048} == {0, 1, 2, 3, 5, 13, 30, 31, 32, 62}
    for name in fx.names(streams_only=True):  # what the device decoder takes on its own: TIC_DECODE_MIN_BLOCKS / _BITS, and a few milliseconds
        e = fx.frames[name]
        assert 1024 <= e["blocks"] <= 4096 and (e["stream_bytes"] - 16) * 8 >= 8192, name
    # both windows of the fused kernel (bits per block <= 240: the small one), with and without the scaled_dct branch
    for scaled in (0, IE.SCALED):
        bpb = [e["stream_bytes"] * 8 // e["blocks"] for e in fx.frames.values() if e["stream_bytes"] and e["flag"] == scaled]
        assert min(bpb) <= 240 and max(bpb) > 256, (scaled, bpb)


def test_oracle_decompress_is_the_reference(fx, decoded):
    for name, px in decoded.items():
        assert fx.matches_reference(name, px), name


def test_oracle_block_idct_route_is_the_reference(fx, oracle):
    """decode() of the dictionary, restated with the oracle's divisors and block_idct - every frame, the non-integral quality included."""
    for name in fx.names():
        e = fx.frames[name]
        dc, ac = fx.coeffs(name)
        px = IE.pixels_block_idct(fx, oracle, IE.zz_absolute(dc, ac), e["height"], e["width"], e["quality"], e["flag"])
        assert fx.matches_reference(name, px), name


def test_sparse_pixels_depend_on_the_operation_order(fx, oracle, decoded):
    """At least 1,000 pixels of the sparse family differ between the reference and a float64 matrix-form IDCT of the same coefficients: a
    kernel with another operation order cannot pass on these frames."""
    total = 0
    for name in fx.names("sparse"):
        e = fx.frames[name]
        dc, ac = fx.coeffs(name)
        zz = IE.zz_absolute(dc, ac)
        ref_px = decoded[name] if name in decoded else IE.pixels_block_idct(fx, oracle, zz, e["height"], e["width"], e["quality"], e["flag"])
        n = int((ref_px != IE.pixels_matrix(fx, oracle, zz, e["height"], e["width"], e["quality"], e["flag"])).sum())
        assert n == e["order_sensitive_pixels"], name
        total += n
    print("order-sensitive pixels:", total)
    assert total == fx.meta["sparse_order_sensitive_pixels"] and total >= 1000


def test_extremes_stand_at_the_worst_case(fx, oracle):
    """The largest |16 r + 2048| of the family is the tables' worst case (about 4.02e8: q = 1, DC 32767, every |AC| = 1023 with the signs of the
    basis function of pixel (3,4)) and inside the int range the fused kernel converts it in without a clamp."""
    worst = 0.0
    for name in fx.names("extremes"):
        e = fx.frames[name]
        dc, ac = fx.coeffs(name)
        zz = IE.zz_absolute(dc, ac)
        assert zz[:, 0].max() == 32767 and zz[:, 0].min() == -32768 and np.abs(zz[:, 1:]).min() == 1023
        worst = max(worst, IE.worst_magnitude(fx, oracle, zz, e["quality"], e["flag"]))
    print("largest |16 r + 2048|: %.6g" % worst)
    assert 4.0e8 <= worst < 2.0 ** 31
    assert abs(worst - fx.meta["extremes_worst_magnitude"]) <= 1e-6 * worst


def test_wide_dc_tells_a_saturating_decoder_apart(fx, oracle, decoded):
    """Per wide-DC frame at least 100 pixels of the reference's output differ from the output with the running DC saturated to int16."""
    for name in fx.names("wide"):
        e = fx.frames[name]
        dc, ac = fx.coeffs(name)
        run = np.cumsum(dc.astype(np.int64))
        assert run.max() > 60000 and run.min() < -60000 and np.abs(dc).max() == 2047
        sat = IE.zz_absolute(IE.clamp_running_dc(dc), ac)
        alt = IE.pixels_block_idct(fx, oracle, sat, e["height"], e["width"], e["quality"], e["flag"])
        n = int((alt != decoded[name]).sum())
        print(name, "pixels a saturating decoder gets wrong:", n)
        assert n == e["pixels_a_saturating_decoder_gets_wrong"] and n >= 100, name
