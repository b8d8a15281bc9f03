"""The table of tests/context_state_common.py is whole: every entry point that takes a context is LISTED in a family's record (called by
its callable, or a device-buffer form that the called one is built on: listed, not necessarily run) or exempt with a reason, every buffer name a record uses is one the library registers, and every expected result loads from the oracle or a fixture with
the shape its case says.  Needs no GPU."""
import os
import re

import numpy as np
import pytest

import context_state_common as CS


def test_every_context_call_is_in_a_family_or_exempt():
    calls = CS.header_context_calls()
    assert len(calls) > 100 and "tic_compress" in calls and "tic_test_poison" in calls  # (the header was parsed)
    covered = {c for f in CS.FAMILIES for c in f.calls}
    for c in calls:
        n = (c in covered) + (c in CS.EXEMPT) + c.startswith("tic_last_")
        assert n == 1, "%s: in %d of {a family, the exemptions, tic_last_*}: add it to a record of tests/context_state_common.py" % (c, n)
    assert all(reason.strip() for reason in CS.EXEMPT.values())
    stale = (covered | set(CS.EXEMPT)) - set(calls)
    assert not stale, "not in the header (any more): %s" % sorted(stale)


def test_every_family_of_the_issue_has_a_record():
    want = ["compress", "compress_dev", "compress_dev_async", "compress_batch[uniform]", "compress_batch[mixed]", "compress_adaptive",
            "compress_batch_adaptive", "compress_scaled", "compress_batch_scaled", "rd_points_scaled_batch", "compressed_sizes", "compress_to_size",
            "compressed_sizes_batch", "compress_batch_to_size", "rd_points", "compress_to_psnr", "rd_points_batch", "compress_batch_to_psnr"]
    for d in ("decompress", "decompress_dev", "decompress_dev_async", "decompress_batch", "decompress_adaptive", "decompress_batch_adaptive",
              "decompress_scaled"):
        want += [d + "[device]", d + "[host]"]
    assert sorted(want) == sorted(CS.BY_NAME) and len(CS.BY_NAME) == len(CS.FAMILIES)


def test_buffer_names_are_the_registry_s():
    """Scratch and state are disjoint, every record names known buffers only, every known name is registered in tic_api.hip under its
    class, and DESIGN.md lists every state buffer."""
    assert not set(CS.SCRATCH) & set(CS.STATE)
    for f in CS.FAMILIES:
        assert f.scratch and set(f.scratch) <= set(CS.SCRATCH), (f.name, set(f.scratch) - set(CS.SCRATCH))
        assert set(f.state) <= set(CS.STATE), (f.name, set(f.state) - set(CS.STATE))
    with open(os.path.join(CS.ROOT, "tinyimgcodec_amd", "csrc", "tic_api.hip")) as f:
        src = f.read()
    with open(os.path.join(CS.ROOT, "DESIGN.md")) as f:
        design = f.read()
    for name in list(CS.SCRATCH) + list(CS.STATE):  # exactly once: where its field is declared (the decoder workspaces': in their name sets)
        assert src.count('"%s"' % name) == 1, "%s is written %d times in tic_api.hip" % (name, src.count('"%s"' % name))
    for name in CS.STATE:
        assert "`%s`" % name in design, "DESIGN.md does not list the state buffer %s" % name
    used = {n for f in CS.FAMILIES for n in f.scratch}
    assert used == set(CS.SCRATCH), "scratch buffers no family touches: %s" % sorted(set(CS.SCRATCH) - used)


def _regions(lines, starts):
    """Line numbers inside the top-level definitions that begin on a line starting with one of `starts`: each up to its closing brace in
    column 0."""
    inside, on = set(), False
    for n, line in enumerate(lines):
        on = on or line.startswith(starts)
        if on:
            inside.add(n)
        if on and line.startswith("}"):
            on = False
    return inside


def test_only_the_buffer_type_allocates_and_frees():
    """No leak by construction: in tic_api.hip every hipMalloc, hipHostMalloc, hipFree and hipHostFree stands inside the owning buffer type,
    the four calls that hand memory to the user, or the transpose self-test (buffers of its own), and tic_destroy calls none of them."""
    with open(os.path.join(CS.ROOT, "tinyimgcodec_amd", "csrc", "tic_api.hip")) as f:
        lines = f.read().split("\n")
    calls = ("hipMalloc(", "hipHostMalloc(", "hipFree(", "hipHostFree(")
    allowed = _regions(lines, ("template <class T, BufKind K> struct Buf ", "template <class T, BufKind K> int Buf<T, K>::",
                               "template <class T, BufKind K> void Buf<T, K>::", "int tic_dev_alloc(", "int tic_dev_free(",
                               "int tic_host_alloc_pinned(", "int tic_host_free_pinned(", "int tic_selftest_transpose("))
    destroy = _regions(lines, ("void tic_destroy(",))
    assert 10 < len(destroy) < 60 and len(allowed) > 100 and not allowed & destroy  # (the definitions were found)
    found = [n for n, line in enumerate(lines) if any(c in line.split("//")[0] for c in calls)]
    assert len(found) >= 11, found  # (3 in the type, 4 in the user's calls, 6 in the self-test: several to a line at most)
    for n in found:
        assert n in allowed, "tic_api.hip:%d allocates or frees outside the buffer type, the user's calls and the self-test: %s" % (n + 1, lines[n].strip())
    buf = _regions(lines, ("template <class T, BufKind K> struct Buf ",))
    for kind in calls:  # (one allocating and one freeing function in the type)
        assert sum(kind in lines[n] for n in found if n in buf) == 1, kind


def test_release_names_every_buffer_member():
    """Slot::release and DecWorkspace::release release member by member: every Buf field of the two structs is in its list (one left out
    would be freed with the struct, but keep its registry record)."""
    with open(os.path.join(CS.ROOT, "tinyimgcodec_amd", "csrc", "tic_api.hip")) as f:
        lines = f.read().split("\n")
    for struct, n_fields in (("Slot", 17), ("DecWorkspace", 3)):
        decl = "\n".join(lines[n] for n in sorted(_regions(lines, ("struct %s {" % struct,))))
        body = "\n".join(lines[n] for n in sorted(_regions(lines, ("void %s::release(" % struct,))))
        fields = re.findall(r"^    (?:Dev|Pin|Mapped)Buf<[^>]+> (\w+)\{", decl, flags=re.M)
        assert len(fields) == n_fields, (struct, fields)
        for name in fields:
            assert "%s.release(ctx)" % name in body, "%s::release does not release %s" % (struct, name)


def _frames(f, which):
    """The (h, w) of a case's frames."""
    case = f.cases[which]
    if f.expect in (CS.exp_adaptive_pixels, CS.exp_adaptive_streams):
        return [(CS.adaptive_entry(i)["height"], CS.adaptive_entry(i)["width"]) for i in case]
    if isinstance(case[0][0], str):
        return [CS.scaled_image(k).shape for k, _ in case]
    return [img.shape for img, _ in case]


@pytest.mark.parametrize("f", CS.FAMILIES, ids=repr)
def test_expected_results_load(f):
    for which in ("small", "ragged", "dense"):
        shapes, exp = _frames(f, which), f.expected(which)
        n, nq = len(shapes), len(CS.QS_DENSE if which == "dense" else CS.QS_SMALL)
        if f.expect in (CS.exp_streams, CS.exp_scaled_streams, CS.exp_adaptive_streams):
            assert len(exp) == n and all(isinstance(s, bytes) and len(s) >= 16 for s in exp)
            for s, (h, w) in zip(exp, shapes):
                assert (int.from_bytes(s[0:4], "little"), int.from_bytes(s[4:8], "little")) == (h, w)
        elif f.expect in (CS.exp_pixels, CS.exp_scaled_pixels):
            assert [e[1] for e in exp] == [tuple(s) for s in shapes] and all(e[0] == "|u1" for e in exp)
        elif f.expect is CS.exp_adaptive_pixels:
            assert len(exp) == n and all(len(e) == 64 for e in exp)
        elif f.expect is CS.exp_sizes:
            assert [e[1] for e in exp] == [(nq,)] * n
        elif f.expect is CS.exp_sizes_batch:
            assert exp[1] == (n, nq)
        elif f.expect is CS.exp_rd:
            assert [[a[1] for a in e] for e in exp] == [[(nq,)] * 3] * n
        elif f.expect in (CS.exp_rd_batch, CS.exp_scaled_rd):
            assert [a[1] for a in exp] == [(n, n if f.expect is CS.exp_scaled_rd else nq)] * 3
        elif f.expect is CS.exp_to_size:
            assert len(exp) == n and all(isinstance(s, bytes) and 1 <= q <= 99 for s, q in exp)
        elif f.expect is CS.exp_to_psnr:
            assert len(exp) == n and all(isinstance(s, bytes) and 1 <= q <= CS.PSNR_MAX_QUALITY and p > 0 for s, q, p in exp)
        else:
            raise AssertionError("no shape rule for %s" % f.expect.__name__)


def test_dense_cases_are_dense_and_valid():
    """The dense frames have a Huffman code for every coefficient at their quality (a dense case must run, not raise), and their streams are
    long; the sharing criterion gives every family at least itself as a partner."""
    for img, q in CS.DENSE + CS.UNIFORM_DENSE:
        assert CS._size(img, q) > img.size // 2
    assert all((f, f) in CS.sharing_pairs() for f in CS.FAMILIES)
    assert np.array_equal(CS.SMALL[0][0], np.full((8, 8), 77, np.uint8))
