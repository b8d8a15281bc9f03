"""tests/golden/entropy_blocks.json on the CPU: the frames tests/entropy_blocks.py builds are the ones the unmodified reference entropy coded
(tests/golden/gen/make_goldens_entropy_blocks.py), the oracle and the host coder write the reference's bytes for them - or refuse where
the reference raised KeyError - and every frame still reaches the edge it was built for (the census, re-derived here from the oracle's
code lengths).  This pins the oracle on built coefficients; tests/test_entropy_blocks_gpu.py runs the same frames through the kernels."""
import numpy as np
import pytest

import entropy_blocks as EB

import tinyimgcodec_amd as T


@pytest.fixture(scope="module")
def fx():
    return EB.load_fixture()["frames"]


@pytest.fixture(scope="module")
def lengths(oracle):
    return EB.Lengths(oracle.dump_tables())


@pytest.fixture(scope="module")
def frames(lengths):
    return EB.build_frames(lengths)


def names(fx, family):
    return [n for n, e in fx.items() if e["family"] == family]


def test_the_builder_makes_the_frames_of_the_fixture(fx, frames):
    assert set(frames) == set(fx)
    assert {e["family"] for e in fx.values()} == set(EB.FAMILIES)
    for name, fr in frames.items():
        e = fx[name]
        assert (fr["family"], fr["h"], fr["w"], fr["quality"]) == (e["family"], e["h"], e["w"], e["quality"]), name
        assert fr["zz"].dtype == np.int16 and fr["zz"].shape == (((e["h"] + 7) // 8) * ((e["w"] + 7) // 8), 64), name
        assert EB.coeff_sha(fr["zz"]) == e["coeffs_sha256"], name
    # the shapes the issue of this fixture asks for: the base frame and every strip count, per family where it names them
    for prefix, counts in (("runs_strip_", EB.STRIPS), ("symbols_strip_", EB.STRIPS), ("zeros_strip_", EB.STRIPS), ("dense_max_strip_", EB.DENSE_STRIPS)):
        assert [n for n in counts if prefix + str(n) not in fx] == [], prefix
    for name in ("runs_ordered", "runs_permuted", "symbols", "dense_max", "zeros", "lane_limit_none", "lane_limit_last", "lane_limit_first"):
        assert fx[name]["census"]["blocks"] == EB.BASE_N, name


@pytest.mark.parametrize("family", EB.FAMILIES)
def test_census(fx, frames, lengths, family):
    """Every frame reaches its edge: census() asserts what the family promises and returns the figures the generator recorded."""
    for name in names(fx, family):
        c = EB.census(name, frames[name], lengths)
        print(name, c)
        assert c == fx[name]["census"], name
        if fx[name]["stream"].get("bytes") is not None:
            assert EB.expected_len(c) == fx[name]["stream"]["bytes"], name  # the code lengths add up to the reference's stream
        else:
            assert EB.expected_len(c) is None, name


def test_census_of_the_families_as_a_whole(fx):
    dense = [fx[n] for n in names(fx, "dense_max")]
    assert sorted(e["census"]["blocks"] for e in dense) == sorted((EB.BASE_N,) + EB.DENSE_STRIPS)
    for e in dense:
        assert e["census"]["max_block_bits"] == EB.MAX_BLOCK_BITS and e["stream"]["bytes"] == 16 + (EB.MAX_BLOCK_BITS * e["census"]["blocks"] + 7) // 8
    for n in names(fx, "alignment"):
        if n.startswith("zeros"):
            assert fx[n]["stream"]["bytes"] == 16 + (6 * fx[n]["census"]["blocks"] + 7) // 8, n
    assert {fx[n]["census"]["payload_bits"] % 32 for n in ("alignment_words", "alignment_bytes", "alignment_bits")} == {0, 8, 5}
    assert {tuple(fx[n]["census"]["blocks_over_512"]) for n in names(fx, "lane_limit")} == {(), (0,), (EB.BASE_N - 1,)}
    nocode = names(fx, "nocode")
    offenders = {(fx[n]["census"]["offender"][0], fx[n]["census"]["offender"][2]) for n in nocode}
    assert {v for k, v in offenders if k == "ac"} == set(EB.AC_OFFENDERS)
    assert {v for k, v in offenders if k == "dc"} == set(EB.DC_OFFENDERS) | {32767}  # (32767: the largest raw DC of a first block)
    assert {fx[n]["census"]["offender"][1] for n in nocode} == {0, EB.MIDDLE, EB.BASE_N - 1}
    assert sum(1 for n in nocode if fx[n]["census"]["blocks"] == 1) == 6 + 6
    for n in nocode:
        assert fx[n]["stream"] == {"raises": "KeyError"}, n
        size = int(EB.size_of(fx[n]["census"]["offender"][2]))
        assert ("raises" in fx[n]["adaptive"]) == (size == 16), n  # the reference's own tables carry categories up to 15
    for n, e in fx.items():
        if e["family"] != "nocode":
            assert "bytes" in e["stream"] and "bytes" in e["adaptive"], n


@pytest.mark.parametrize("family", EB.FAMILIES)
def test_oracle_and_host_coder_write_the_references_stream(fx, frames, lengths, oracle, family):
    for name in names(fx, family):
        e, fr = fx[name], frames[name]
        zz, h, w, q = fr["zz"], fr["h"], fr["w"], fr["quality"]
        dc, ac = EB.dc_ac(zz)
        if "raises" in e["stream"]:
            assert e["stream"]["raises"] == "KeyError", name
            with pytest.raises(oracle.OracleError):
                oracle.entropy_encode(dc, ac, h, w, q)
            with pytest.raises(KeyError):
                T.entropy_encode(zz, h, w, q)
            with pytest.raises(KeyError):
                T.entropy_size(zz, h, w)
            continue
        want = oracle.entropy_encode(dc, ac, h, w, q)
        assert len(want) == e["stream"]["bytes"] and EB.sha(want) == e["stream"]["sha256"], name
        got = T.entropy_encode(zz, h, w, q)
        assert got == want, (name, EB.first_difference(got, want, zz, lengths))
        assert T.entropy_size(zz, h, w) == e["stream"]["bytes"], name
