"""The host model of the strip kernel's decisions (tests/native/strip_decisions_model.cpp) against its fixture, and the conditions the fixture's
inputs have to meet - on the CPU.  The model is rebuilt from tic_math.h and tic_strip_plan.h as they are now and every case of
tests/golden/strip_decisions.json is recomputed, so the numbers tests/test_strip_decisions_gpu.py holds the device to cannot go stale.

What counts can and cannot tell apart: every planted class block sits within one band of its threshold (tripped) or between one and two bands
(accepted), so a device whose accept test reads another lane's, another group's or the other pass order's threshold counts differently (the
mutants below).  A band narrower by the two float steps thr_below() takes off each threshold (tic_math.h: 2^-25 each, against bands of
1e-6 .. 1e-3) is NOT expected to change any count here: no planted or noise distance is known to fall into so thin a slice, and this test does
not claim otherwise."""
import numpy as np
import pytest

import strip_decisions_common as SD


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("strip_decisions")
    return SD.build_model(d), d


@pytest.fixture(scope="module")
def fixture():
    return SD.load_fixture()


def test_fixture_is_what_the_model_computes_now(model, fixture):
    exe, tmp = model
    assert fixture["base_knobs"] == SD.BASE_KNOBS and tuple(fixture["info_fields"]) == SD.INFO_FIELDS
    names = [c["name"] for c in fixture["cases"]]
    assert len(set(names)) == len(names)
    for c in fixture["cases"]:
        m = SD.model_case(exe, tmp, c)
        assert (m["stats"], m["plan"]) == (c["stats"], c["plan"]), c["name"]
        for mu, want in c.get("mutants", {}).items():
            assert SD.model_case(exe, tmp, c, mutant=mu)["stats"] == want, (c["name"], mu)
        if c["plan"][0]:  # with the team schedule off and the grid capped, the device cannot matter: no team, one grid row, the order asked for
            assert c["plan"][0] == (SD.ORDER_COLS if c["order"] else SD.ORDER_ROWS) and c["plan"][2] == 0 and c["plan"][4] == 1, c["name"]


def test_config2_tie_strips_and_modelled_rates(model, fixture):
    """stats[1] of the 4096 x 4096 config-2 frame (asserted on the device by test_gpu_parity.py::test_config2_4096_coefficient_digest) and the
    trip rates DESIGN.md section 3 quotes as modelled."""
    exe, tmp = model
    raw = tmp / "config2.raw"
    SD.rand_frame(1234, 4096, 4096).tofile(str(raw))
    for q, by_order in fixture["config2_tie_strips"].items():
        for order, want in by_order.items():
            assert SD.run_model(exe, raw, 4096, 4096, 4096, 1, 4096 * 4096, int(q), int(order), SD.BASE_KNOBS)["stats"][1] == want, (q, order)
    SD.rand_frame(2001, 1024, 2048).tofile(str(raw))
    for q, want in fixture["modelled_rates_noise_1024x2048"].items():
        m = SD.run_model(exe, raw, 1024, 2048, 2048, 1, 1024 * 2048, int(q), 1, SD.BASE_KNOBS)
        assert {k: m[k] for k in ("blocks", "trip_blocks", "trip_strips", "fast_strips")} == {k: v for k, v in want.items() if k != "tie_strips"}
        assert m["stats"][1] == want["tie_strips"]


def test_planted_scenarios_are_what_their_names_claim(model, fixture):
    """By the model, in both pass orders: the strips that trip anything are exactly the planted ones, with exactly the planted blocks tripping
    (the background block, flat 128, trips nothing; the true-tie block is an irrational trip without a rational tie; the flat odd block a
    rational tie without a trip) - and on 64 workgroups the model's counts are the ones the rules give by hand."""
    exe, tmp = model
    seen = set()
    for c in fixture["cases"]:
        if c["frame"]["kind"] != "scenario":
            continue
        want = [[0, strip, int(tie), (1 << ntrip) - 1] for strip, ntrip, tie in SD.SCENARIOS[c["frame"]["scenario"]][0]]
        m = SD.model_case(exe, tmp, c, strips=True)
        assert m["strips"] == want, c["name"]
        if "hand" in c:
            assert c["hand"] == SD.SCENARIOS[c["frame"]["scenario"]][1] == c["stats"], c["name"]
            assert c["plan"][1:6] == [SD.KIND_ROWS, 0, 64, 1, 256], c["name"]  # wave 3 walks strips 3, 259 and 515
            seen.add((c["frame"]["scenario"], c["order"]))
    assert seen == {(s, o) for s in SD.SCENARIOS for o in (0, 1)}
    # the same strips under the other walks fall to other waves: the counts of the two-strip scenarios differ from the hand figures
    for walk in ("planted on 128 workgroups: ", "planted, chunked walk of a wide frame: "):
        for c in fixture["cases"]:
            if c["name"].startswith(walk + "5 and 5"):
                assert c["stats"] == [10, 0, 0, 5], c["name"]
    assert any(c["plan"][1] == SD.KIND_CHUNK and c["plan"][5] == 4 for c in fixture["cases"] if c["frame"]["kind"] == "scenario")


def test_class_blocks_sit_where_the_fixture_says(model, fixture):
    """delta = 0.5 - |d| (distance to the tie), beta = 0.5 - thr (the band), class = 3 * lane + group, 24 per pass order.  A "tripped" block has
    delta < beta in its class and is at least two bands from the tie in every other; an "accepted" block trips nothing, has
    beta <= delta < 2 beta in its class and is at least two bands away in every other.  Over the qualities used, every class of either
    order has one of each.  (The rational classes - lanes 0 and 4, group {0,4} - have quotients on a grid of 1 / (8 div): just-accepted ones
    exist only at qualities tuned for them, which the generator bisects; their just-tripped ones are exact ties.)"""
    exe, tmp = model
    covered = {(o, kind): set() for o in (0, 1) for kind in ("tripped", "accepted")}
    for cf in fixture["class_frames"]:
        blocks = SD.planted_blocks(cf["blocks"])
        assert blocks.shape == (len(cf["tripped"]) + len(cf["accepted"]), 8, 8)
        c = SD.classes_of(exe, tmp, blocks, cf["quality"], cf["order"])
        beta = c["beta"]
        assert all(0.0 < b < 0.01 for b in beta)
        for k, (kind, cls) in enumerate([("tripped", x) for x in cf["tripped"]] + [("accepted", x) for x in cf["accepted"]]):
            b = c["blocks"][k]
            for other in range(24):
                if other != cls:
                    assert not b["tripped"][other] and b["delta"][other] >= 2.0 * beta[other], (cf["blocks"], k, cls, other)
            if kind == "tripped":
                assert b["tripped"][cls] and b["delta"][cls] < beta[cls], (cf["blocks"], k, cls)
                assert (b["tie"], b["trip"]) == ((True, False) if cls in (2, 14) else (False, True))
            else:
                assert not b["tripped"][cls] and beta[cls] <= b["delta"][cls] < 2.0 * beta[cls], (cf["blocks"], k, cls)
                assert not b["tie"] and not b["trip"]
            covered[(cf["order"], kind)].add(cls)
    for key, got in covered.items():
        assert got == set(range(24)), (key, sorted(set(range(24)) - got))
    qualities = {cf["quality"] for cf in fixture["class_frames"]}
    assert {50, 90, 1} <= qualities and any(q != int(q) for q in qualities)
    total = sum(len(SD.planted_blocks(cf["blocks"])) for cf in fixture["class_frames"])
    assert 100 <= total <= 600


def test_every_mutant_is_told_apart_in_each_pass_order(fixture):
    """A wrong accept test - groups {1,2,3} and {5,6,7} exchanged, lane u ^ 1's thresholds, the other order's table, the {0,4} threshold
    everywhere - predicts other counts than the true model on at least one case the GPU runs, columns first and rows first."""
    for mu in SD.MUTANTS:
        for order in (0, 1):
            told = [c["name"] for c in fixture["cases"] if c["order"] == order and "mutants" in c and c["mutants"][mu] != c["stats"]]
            assert told, (mu, order)
            # ... and on a class frame, where single planted blocks decide (not only on the statistics of noise)
            assert any(n.startswith("class frame") for n in told), (mu, order, told)


def test_sanitizer_build_reproduces_the_planted_cases(model, fixture, tmp_path):
    """The same program under the address and undefined-behaviour sanitizers, stand-alone, over the planted cases (the 64-wide scenario frames, the
    class frames, the ragged and multi-frame cases) and the block modes."""
    _, tmp = model
    exe = SD.build_model(tmp_path, sanitize=True)
    n = 0
    for c in fixture["cases"]:
        f = c["frame"]
        if f["kind"] in ("classes", "near_ties", "frames") or (f["kind"] == "scenario" and f["w"] == SD.PLANTED_W) or f.get("h") == 200:
            m = SD.model_case(exe, tmp, c, strips=True)
            assert (m["stats"], m["plan"]) == (c["stats"], c["plan"]), c["name"]
            n += 1
    assert n >= 50
    cf = fixture["class_frames"][0]
    assert len(SD.classes_of(exe, tmp, SD.planted_blocks(cf["blocks"]), cf["quality"], cf["order"])["blocks"]) == len(SD.planted_blocks(cf["blocks"]))


def test_merge_rule_is_the_library_s():
    """The case builder's copy of merge_frames (csrc/tic_api.hip): frames without a gap that end on a block row become one tall frame."""
    assert SD.merged_geometry(256, 512, 512, 3, 256 * 512) == (768, 1, 768 * 512)
    assert SD.merged_geometry(256, 512, 512, 3, 256 * 512 + 4096) == (256, 3, 256 * 512 + 4096)
    assert SD.merged_geometry(252, 512, 512, 3, 252 * 512) == (252, 3, 252 * 512)
    assert SD.merged_geometry(256, 512, 512, 1, 256 * 512) == (256, 1, 256 * 512)
    assert np.array_equal(SD.true_tie_block()[0, :2], [192, 64])
