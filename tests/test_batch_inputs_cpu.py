"""tests/batch_inputs_common.py alone (no GPU): for every layout the views a call would build from pointer, stride, h and w are the frames,
every other byte of the arena is poison, the arena holds whatever a copy at the staged pitch would read, and each layout has the property
its name promises - odd addresses, shared rows, plan order, gaps, where a registration ends."""
import numpy as np
import pytest

import batch_inputs_common as B

SHAPES = [(8, 8), (8, 72), (24, 8), (16, 40), (13, 21), (0, 16), (32, 40), (16, 120), (5, 3), (7, 9), (64, 96)]
QUALS = [50, 20, 85, 35, 60, 45, 35, 10, 90, 70, 30]
RAGGED = [4, 5, 8, 9]


def frames_of(idx=None):
    idx = range(len(SHAPES)) if idx is None else idx
    return [np.random.default_rng(900 + i).integers(1, 255, SHAPES[i], dtype=np.uint8) for i in idx], [QUALS[i] for i in idx]  # (no pixel is a poison)


def build_all(layout, poison):
    """Every variant of a layout -> [(Arena, frames, quals)]."""
    if layout == "ragged_at_256":
        frames, quals = frames_of(RAGGED)
        return [(B.build(frames, layout, poison, quals), frames, quals)]
    frames, quals = frames_of()
    variants = (0, 1) if layout in ("mosaic", "half_registered") else (0,)
    return [(B.build(frames, layout, poison, quals, variant=v), frames, quals) for v in variants]


@pytest.mark.parametrize("poison", [0x00, 0xFF])
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_views_poison_and_bounds(layout, poison):
    for a, frames, quals in build_all(layout, poison):
        ptrs, strides = a.inputs()
        base, size = a.arena.ctypes.data, a.arena.size
        assert a.arena.dtype == np.uint8 and base % B.PAGE == 0 and size % B.PAGE == 0 and a.arena.base is a.raw
        mask = np.zeros(size, bool)
        for i, f in enumerate(frames):
            h, w = f.shape
            assert strides[i] >= max(w, 1)
            if f.size == 0:
                assert ptrs[i] == 0
                continue
            off = ptrs[i] - base
            view = np.lib.stride_tricks.as_strided(a.arena[off:], (h, w), (strides[i], 1))
            assert np.array_equal(view, f), (layout, i)
            for y in range(h):
                assert not mask[off + y * strides[i]: off + y * strides[i] + w].any(), (layout, i, "two frames share a byte")
                mask[off + y * strides[i]: off + y * strides[i] + w] = True
            # whatever a copy may take for this frame's extent lies inside the arena: its rows at its stride, its rows at the staged pitch, and
            # every frame's staged bytes behind it
            staged = sum(B.batch_pitch(g.shape[1]) * g.shape[0] for g in frames)
            assert off >= 0 and off + h * max(strides[i], B.batch_pitch(w)) + staged <= size, (layout, i)
        assert (a.arena[~mask] == poison).all() and (a.raw == poison).sum() >= a.raw.size - int(mask.sum())
        reg = a.register_range()
        assert (reg is not None) == (layout in B.REGISTERED)
        if reg:
            assert reg[0] == base and reg[1] % B.PAGE == 0 and 0 < reg[1] <= size


def test_what_each_layout_promises():
    frames, quals = frames_of()
    shapes = [f.shape for f in frames]
    with_pixels = [i for i, f in enumerate(frames) if f.size]
    order = sorted(with_pixels, key=lambda i: (quals[i], shapes[i][1], shapes[i][0]))  # the documented rule: (quality, width, height), stable
    assert order != with_pixels and order.index(3) + 1 == order.index(6)  # (the caller's order differs; the two 40-wide frames of q = 35 are neighbours)
    pitch = [w if w % 8 == 0 else (w + 255) // 256 * 256 for _, w in shapes]

    a = B.build(frames, "dense", 0, quals)
    assert [a.strides[i] for i in with_pixels] == [shapes[i][1] for i in with_pixels]
    a = B.build(frames, "wide_odd", 0, quals)
    assert all(a.strides[i] == shapes[i][1] + 13 and a.pointers()[i] % 2 == 1 for i in with_pixels)
    for layout in ("wide_8", "registered_wide"):
        a = B.build(frames, layout, 0, quals)
        assert all(a.strides[i] == shapes[i][1] + 24 and a.pointers()[i] % 8 == 0 for i in with_pixels)
        assert (a.register is None) == (layout == "wide_8") and (a.register is None or a.register == (0, a.arena.size))

    # mosaic: one stride, the width of the picture; the bytes right of a window's row are its neighbour's pixels, another one per variant
    right = []
    for v in (0, 1):
        a = B.build(frames, "mosaic", 0, quals, variant=v)
        assert len({a.strides[i] for i in with_pixels}) == 1 and a.strides[0] == sum(shapes[i][1] for i in with_pixels)
        i = with_pixels[3]
        h, w = shapes[i]
        nb = a.arena[a.offsets[i] + w: a.offsets[i] + w + 8]
        j = with_pixels[4] if v == 0 else with_pixels[2]
        assert np.array_equal(nb[: min(8, shapes[j][1])], frames[j][0, : min(8, shapes[j][1])]), v
        right.append(nb.copy())
    assert not np.array_equal(right[0], right[1])

    a = B.build(frames, "packed_in_plan_order", 0xFF, quals)
    cursor = 0
    for i in order:
        assert a.offsets[i] == cursor and a.strides[i] == pitch[i]
        cursor += pitch[i] * shapes[i][0]
    assert a.register == (0, a.arena.size)

    a = B.build(frames, "packed_reversed_with_gaps", 0xFF, quals)
    cursor = 0
    for i in order[::-1]:
        assert a.offsets[i] == cursor and a.strides[i] == pitch[i]
        cursor += pitch[i] * shapes[i][0]
        assert (a.arena[cursor: cursor + 64] == 0xFF).all()
        cursor += 64

    # half_registered: a leading, page-aligned part; (a) it ends between the frames at plan positions 3 and 4, (b) inside the one at position 4
    for v in (0, 1):
        a = B.build(frames, "half_registered", 0, quals, variant=v, split=4)
        first, nbytes = a.register
        assert first == 0 and nbytes % B.PAGE == 0 and 0 < nbytes < a.arena.size
        for pos, i in enumerate(order):
            lo, hi = a.extent(i)
            assert a.strides[i] == pitch[i] and hi - lo == pitch[i] * shapes[i][0]
            if pos < 4:
                assert hi <= nbytes
            elif pos == 4:
                assert (lo == nbytes) if v == 0 else (lo < nbytes < hi - 1)
            else:
                assert lo > nbytes
        assert [a.offsets[i] for i in order] == sorted(a.offsets[i] for i in order)

    rf, rq = frames_of(RAGGED)
    a = B.build(rf, "ragged_at_256", 0, rq)
    first, nbytes = a.register
    ends = {i: a.extent(i)[1] for i, f in enumerate(rf) if f.size}
    assert all(a.strides[i] == 256 for i in ends)
    assert ends[2] == nbytes and ends[0] == nbytes + 16 and ends[3] <= a.extent(2)[0]  # 5 x 3 ends with the registration, 13 x 21 crosses it
    assert a.extent(0)[0] < nbytes and a.extent(2)[0] >= 0


def test_crops_of_a_strip():
    pic = np.random.default_rng(5).integers(1, 255, (64, 40), dtype=np.uint8)
    windows = [(0, 16), (16, 32), (32, 16)]
    a = B.crops_of_a_strip(pic, windows, 0xFF)
    ptrs, strides = a.inputs()
    assert strides == [40] * 3 and a.register == (0, a.arena.size)
    assert ptrs[1] == ptrs[0] + 16 * 40 and ptrs[2] == ptrs[0] + 32 * 40  # the second follows the first; the third lies inside the second
    for i, (r, m) in enumerate(windows):
        assert np.array_equal(a.view(i), pic[r: r + m])
    assert (a.arena[48 * 40:] == 0xFF).all() and np.array_equal(a.arena[: 48 * 40].reshape(48, 40), pic[:48])
