"""tests/golden/decoder_streams.json on the CPU: the frames tests/decoder_streams.py builds reach the decoder states they were built for
(the census, re-derived from the oracle's code lengths), the oracle writes the streams the unmodified reference wrote for them and
decodes them to the reference's pixels (tests/golden/gen/make_goldens_decoder_streams.py), and - the fused kernel gives out pixels only -
a wrong coefficient in a value-bearing frame would change a pixel: visibility, measured with the oracle's own inverse stage.
tests/test_decoder_streams_gpu.py runs the same streams through the device decoder."""
import numpy as np
import pytest

import decoder_streams as DS
import entropy_blocks as EB
import inverse_edges as IE


@pytest.fixture(scope="module")
def fx():
    return DS.load_fixture()


@pytest.fixture(scope="module")
def lengths(oracle):
    return EB.Lengths(oracle.dump_tables())


@pytest.fixture(scope="module")
def frames(lengths):
    return DS.build_frames(lengths)


@pytest.fixture(scope="module")
def ie():
    return IE.Fixture()


FRAME_NAMES = list(DS.load_fixture()["frames"])


def test_the_builder_makes_the_frames_of_the_fixture(fx, frames):
    assert sorted(frames) == sorted(FRAME_NAMES) and fx["generator"] == "tests/golden/gen/make_goldens_decoder_streams.py"
    assert set(DS.REUSED) | {"pairs", "long_codes", "values", "cap"} <= set(frames)
    assert {fr["family"] for fr in frames.values()} >= set(DS.NEW_FAMILIES)
    for name, fr in frames.items():
        e = fx["frames"][name]
        assert (fr["family"], fr["h"], fr["w"], fr["variants"]) == (e["family"], e["h"], e["w"], e["variants"]), name
        assert fr["zz"].shape == (DS.N, 64) and fr["zz"].dtype == (np.int32 if DS.is_twin(name) else np.int16), name
        assert EB.sha(np.ascontiguousarray(fr["zz"], dtype="<i4").tobytes()) == e["coeffs_sha256"], name
        assert set(e["streams"]) == {DS.key(v) for v in fr["variants"]} and len(e["streams"]) == len(fr["variants"]), name
        if name in DS.VALUE_FRAMES:  # the eight plain qualities and one scaled variant
            assert [tuple(v) for v in fr["variants"]] == list(DS.VALUE_VARIANTS), name
        else:                        # two plain variants, quality 5 among them, and one scaled one
            assert [v[0] for v in fr["variants"]] == [0, 0, DS.SCALED] and fr["variants"][0] == [0, 5], name


def test_the_reused_frames_are_those_of_the_entropy_fixture(frames):
    eb = EB.load_fixture()["frames"]
    for name in DS.REUSED:
        assert EB.coeff_sha(frames[name]["zz"]) == eb[name]["coeffs_sha256"], name
        assert [0, eb[name]["quality"]] in frames[name]["variants"], name


@pytest.mark.parametrize("name", FRAME_NAMES)
def test_census(fx, frames, lengths, name):
    """Every frame reaches its edge: census() asserts what the family promises and returns the figures the generator recorded."""
    c = DS.census(name, frames[name], lengths)
    print(name, c)
    assert c == fx["frames"][name]["census"], name
    assert all(s["bytes"] == c["stream_bytes"] for s in fx["frames"][name]["streams"].values()), name  # the lengths add up to the reference's stream
    assert c["stream_bytes"] - 16 >= DS.MIN_PAYLOAD_BYTES and DS.N >= 1024  # what the device decoder takes


def test_census_of_the_fixture_as_a_whole(fx, lengths):
    f = fx["frames"]
    pairs, longs = f["pairs"]["census"], f["long_codes"]["census"]
    assert pairs["fused_pairs_seen"] == pairs["fused_pairs_at_all_extreme_values"] == pairs["fused_pairs_by_the_lengths"] == len(DS.fused_pairs(lengths)) > 0
    # per pair length: every start residue mod 32, a word boundary at every inner bit offset
    by_bits = pairs["residues_and_boundary_offsets_by_pair_bits"]
    assert max(int(t) for t in by_bits) == pairs["longest_pair_bits"] and all(v == [32, int(t) - 1, int(t) - 1] for t, v in by_bits.items()), by_bits
    assert pairs["fused_pairs_with_eob_second"] > 0 and pairs["near_miss_instances"] >= pairs["near_misses_by_the_lengths"] > 0  # (census() checks pair by pair)
    # (with these lengths no pair with a ZRL is fused - its codeword alone fills the window; the frame holds ZRLs as look-ups of their own)
    assert pairs["fused_pairs_with_zrl"] == 0 and pairs["zrl_as_first_lookup"] > 0 and pairs["zrl_behind_a_symbol"] > 0
    assert longs["contexts_seen"] == longs["contexts_needed"] == longs["long_symbols"] * 5 * 3 and longs["long_symbols"] == len(DS.long_symbols(lengths))
    assert f["values"]["census"]["ac_symbols"] == 160
    rules = {n: e["census"]["range_rule"] for n, e in f.items() if e["family"] == "spikes"}
    assert rules == {"spikes_flat_one": 1056, "spikes_flat_two": 1056, "spikes_sparse": 288}
    assert f["spikes_sparse"]["census"]["whole_ranges_one_block_covers"]["288"] == 5
    assert {bits for n in rules for b, bits in f[n]["census"]["spikes"]} == set(DS.SPIKE_BITS)
    for n in ("cap", "zeros"):
        assert f[n]["census"]["block_starts_in_one_range"] == {str(r): [r // 6, DS.cap_of(r)] for r in DS.RANGES}, n
    assert f["zeros"]["census"]["periodic"] and [n for n, e in f.items() if e["census"]["periodic"]] == ["zeros"]
    assert (f["dc_bounds_pos"]["census"]["dc_max"], f["dc_bounds_neg"]["census"]["dc_min"]) == (32767, -32768)
    assert (f["dc_bounds_pos_over"]["census"]["dc_max"], f["dc_bounds_neg_over"]["census"]["dc_min"]) == (32768, -32769)
    # every other frame keeps the running DC inside +-2,047 apart from what symbols does: the new families to the letter (a 1,662-bit
    # spike needs a step of 2,047 from a flat walk inside +-20), and of the reused frames all but the three named here, which are the
    # entropy fixture's as they are (a seeded drift beside their +-2,047 edges; a sum of seeded differences of up to +-200)
    beyond = {"dc_edges_pos": 2050, "dc_edges_pos_ac63": 2050, "dc_edges_neg": 2050, "dc_edges_neg_ac63": 2050, "long_short_alternating": 5390}
    for n, e in f.items():
        if e["family"] != "dc_bounds" and n != "symbols":
            most = max(abs(e["census"]["dc_min"]), abs(e["census"]["dc_max"]))
            assert most <= (2047 + 20 if e["family"] in DS.NEW_FAMILIES else beyond.get(n, 2047)), (n, e["census"])
            assert n not in beyond or most > 2047, n
    # both windows of the fused kernel, with and without the scaled branch (every frame has plain and scaled variants)
    assert {e["census"]["bits_per_block"] <= 240 for e in f.values()} == {True, False}


@pytest.mark.parametrize("name", FRAME_NAMES)
def test_oracle_writes_the_references_stream_and_pixels(fx, frames, oracle, name):
    fr, e = frames[name], fx["frames"][name]
    payload = DS.payload_stream(oracle, fr)
    for variant in fr["variants"]:
        s, rec = DS.with_header(payload, fr, variant), e["streams"][DS.key(variant)]
        dc, ac = DS.dc_ac(fr["zz"])
        if not variant[0]:
            assert s == oracle.entropy_encode(dc, ac, fr["h"], fr["w"], variant[1]), (name, variant)
        assert (len(s), EB.sha(s)) == (rec["bytes"], rec["sha256"]), (name, variant)
        assert IE.px_sha(oracle.decompress(s)) == rec["pixels_sha256"], (name, variant)


@pytest.mark.parametrize("name", FRAME_NAMES)
def test_block_pixels_are_the_oracles(fx, frames, oracle, ie, name):
    """DS.block_pixels - what both visibility measures stand on - gives, block by block, the pixels of oracle.decompress of the frame's
    stream (and so the fixture's digest), under every variant."""
    fr = frames[name]
    payload = DS.payload_stream(oracle, fr)
    for variant in fr["variants"]:
        px = DS.block_pixels(ie, oracle, fr["zz"].astype(np.int64), variant)
        tiled = px.reshape((DS.H + 7) // 8, (DS.W + 7) // 8, 8, 8).swapaxes(1, 2).reshape(DS.H, DS.W)
        assert np.array_equal(tiled, oracle.decompress(DS.with_header(payload, fr, variant))), (name, variant)
        assert IE.px_sha(tiled) == fx["frames"][name]["streams"][DS.key(variant)]["pixels_sha256"], (name, variant)


@pytest.mark.parametrize("name", [n for n in FRAME_NAMES if "visibility" in DS.load_fixture()["frames"][n]])
def test_visibility(fx, frames, oracle, ie, name):
    """Would a wrong coefficient change a pixel?  Sign flipped, magnitude halved, top bit dropped, moved one scan position on (into a
    zero), +-1 towards zero: each counts as seen when the oracle's pixels of the block change under at least one variant of the frame.
    Bars for the value-bearing frames: 100 % of the first four classes, and of +-1 at sizes up to 4.  Shares without a bar - +-1 at larger
    sizes, every class on the other frames - are printed and are the fixture's."""
    v = DS.visibility(ie, oracle, frames[name])
    print(name, {k: "%d / %d" % tuple(x) for k, x in v.items()})
    assert v == fx["frames"][name]["visibility"], name
    if name in DS.VALUE_FRAMES:
        DS.check_bars(name, v)


@pytest.mark.parametrize("name", DS.DC_ONLY)
def test_dc_visibility(fx, frames, oracle, ie, name):
    """The frames without AC: a DC difference changed by +-1 at any block is seen under the quality-5 variant.  A DC step is 20 grey
    levels there, and a block beyond a DC of +-6 is clipped whatever its DC: cap keeps its DC inside +-5, and the dc_edges frames come
    back next to 0 behind every edge and in the last block (EB.dc_edges_blocks), so a wrong difference anywhere moves a block that
    shows it.  4,290 of 4,290 (both signs at 2,145 blocks) for each."""
    seen, of = DS.dc_visibility(ie, oracle, frames[name], (0, 5))
    print(name, "%d / %d" % (seen, of))
    assert [seen, of] == fx["frames"][name]["dc_visibility"], name
    assert seen == of == 2 * DS.N, name


def test_adaptive_digests_cover_the_entropy_fixture(fx):
    """test_entropy_blocks_gpu.py::test_adaptive_kernels takes its pixels from here: a digest for every frame that has an own-table stream."""
    eb = EB.load_fixture()["frames"]
    assert set(fx["adaptive_pixels"]) == {n for n, e in eb.items() if "bytes" in e["adaptive"]}
    for name in DS.REUSED:
        assert fx["adaptive_pixels"][name] == fx["frames"][name]["streams"]["q%d" % eb[name]["quality"]]["pixels_sha256"], name
