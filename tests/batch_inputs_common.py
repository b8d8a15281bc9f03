"""Host memory for the batch entry points that take a pointer and a row stride per frame (tic_compress_batch_v and its seven relatives): given
frames and a layout name, ONE uint8 arena that owns every byte a call may be handed - the frames at the layout's addresses and strides, every
other byte a poison value of the caller's choice - with the pointers, the strides and the range to register, if the layout has one.  The arena
is allocated memory from its first byte to its last, with a tail behind the last frame as long as all frames staged together: a copy that
takes the wrong stride, the wrong length or the wrong neighbour reads poison or another frame's pixels, never an unmapped address.
tests/test_batch_inputs_cpu.py checks this module alone; tests/test_batch_input_routes_gpu.py runs the calls on it.  No test lives here."""
import numpy as np

PAGE = 4096
GAP = 64
LAYOUTS = ("dense", "wide_odd", "wide_8", "mosaic", "packed_in_plan_order", "packed_reversed_with_gaps", "registered_wide", "half_registered",
           "ragged_at_256")
REGISTERED = ("packed_in_plan_order", "packed_reversed_with_gaps", "registered_wide", "half_registered", "ragged_at_256")


def align_up(v, a):
    return (v + a - 1) // a * a


def batch_pitch(w):
    """The row pitch at which the library stages a frame (tic_host_pipeline.h): rows of a multiple of 8 bytes back to back, others at the
    next multiple of 256."""
    return w if w % 8 == 0 else align_up(w, 256)


def plan_order(shapes, quals):
    """The frames with blocks in the order of the library's plan: by (quality, width, height), stable."""
    return sorted((i for i, (h, w) in enumerate(shapes) if h > 0 and w > 0), key=lambda i: (quals[i], shapes[i][1], shapes[i][0]))


class Arena:
    """arena: the uint8 array (page-aligned, a whole number of pages; `raw` is the allocation it is cut from, poison too); offsets[i]: where
    frame i's first pixel lies in it (None: a frame without pixels, passed as a null pointer); strides[i]; register: (offset, bytes) of the
    range to register or None; boundary: where a registration that covers part of the arena ends."""

    def __init__(self, frames, layout, poison, offsets, strides, end, register_to=None):
        self.frames, self.layout, self.poison = frames, layout, poison
        self.offsets, self.strides = list(offsets), list(strides)
        tail = align_up(sum(batch_pitch(f.shape[1]) * f.shape[0] for f in frames if f.size), PAGE) + PAGE
        size = align_up(end + tail, PAGE)
        self.raw = np.full(size + PAGE, poison, np.uint8)
        skip = -self.raw.ctypes.data % PAGE
        self.arena = self.raw[skip: skip + size]
        assert self.arena.ctypes.data % PAGE == 0 and self.arena.base is self.raw
        for i, f in enumerate(frames):
            if f.size:
                self.view(i)[...] = f
        assert int(self.pixel_mask().sum()) == sum(f.size for f in frames) or layout == "crops_of_a_strip", "two frames share a byte"
        self.register = None if register_to is None else (0, size if register_to == "all" else register_to)
        self.boundary = None if self.register is None else self.register[1]

    def view(self, i):
        """Frame i as the call sees it: h rows of w bytes, strides[i] apart, from its pointer on."""
        h, w = self.frames[i].shape
        return np.lib.stride_tricks.as_strided(self.arena[self.offsets[i]:], (h, w), (self.strides[i], 1))

    def pixel_mask(self):
        mask = np.zeros(self.arena.size, bool)
        for i, f in enumerate(self.frames):
            if f.size:
                h, w = f.shape
                np.lib.stride_tricks.as_strided(mask[self.offsets[i]:], (h, w), (self.strides[i], 1))[...] = True
        return mask

    def pointers(self):
        return [0 if o is None else self.arena.ctypes.data + o for o in self.offsets]

    def inputs(self):
        """(pointers, strides): what VCall, SCall, ACall and frame_arrays take as `inputs`."""
        return self.pointers(), list(self.strides)

    def register_range(self):
        """(address, bytes) for tic_host_register, or None."""
        return None if self.register is None else (self.arena.ctypes.data + self.register[0], self.register[1])

    def extent(self, i):
        """(first, end) offsets of frame i's staged image if it is read where it lies: pitch * h bytes from its pointer."""
        h, w = self.frames[i].shape
        return self.offsets[i], self.offsets[i] + batch_pitch(w) * h


def build(frames, layout, poison, quals=None, variant=0, split=4, last=None, cross=None):
    """-> Arena.  quals: the qualities the plan-order layouts sort by.  variant: mosaic - 0 windows side by side in the caller's order, 1 in
    reverse (other neighbours); half_registered - 0 the registration ends between the frames at plan positions split - 1 and split, 1 eight
    bytes into the frame at position split.  last, cross (ragged_at_256): the frame whose staged image ends with the registration and the
    one whose ends 16 bytes behind it; by default the one with the fewest rows and the one with the most."""
    assert layout in LAYOUTS, layout
    frames = [np.asarray(f, np.uint8) for f in frames]
    shapes = [f.shape for f in frames]
    n = len(frames)
    with_pixels = [i for i in range(n) if frames[i].size]
    offsets, strides = [None] * n, [max(w, 1) for _, w in shapes]
    end, register_to = 0, None
    if layout in ("dense", "wide_odd", "wide_8", "registered_wide"):
        extra = {"dense": 0, "wide_odd": 13}.get(layout, 24)
        cursor = GAP
        for i in range(n):
            h, w = shapes[i]
            strides[i] = max(w, 1) + extra
            if frames[i].size:
                offsets[i] = (cursor | 1) if layout == "wide_odd" else align_up(cursor, 64) + (0 if layout == "dense" else 8)
                cursor = offsets[i] + h * strides[i] + GAP
        end = cursor
        register_to = "all" if layout == "registered_wide" else None
    elif layout == "mosaic":
        width = sum(shapes[i][1] for i in with_pixels)
        x = GAP
        for i in (with_pixels if variant == 0 else with_pixels[::-1]):
            offsets[i] = x
            x += shapes[i][1]
        for i in range(n):
            strides[i] = width
        end = GAP + width * max(shapes[i][0] for i in with_pixels)
    elif layout in ("packed_in_plan_order", "packed_reversed_with_gaps", "half_registered"):
        order = plan_order(shapes, quals)
        cursor = 0
        for pos, i in enumerate(order if layout != "packed_reversed_with_gaps" else order[::-1]):
            h, w = shapes[i]
            strides[i] = batch_pitch(w)
            if layout == "half_registered" and pos == split:
                if variant == 0:
                    register_to = cursor = align_up(max(cursor, 1), PAGE)
                else:
                    register_to = align_up(cursor + 8, PAGE)
                    cursor = register_to - 8
            offsets[i] = cursor
            cursor += strides[i] * h + (GAP if layout == "packed_reversed_with_gaps" else 0)
        end = cursor
        if layout != "half_registered":
            register_to = "all"
        assert register_to is not None, "half_registered needs more than `split` frames"
    else:  # ragged_at_256
        assert all(shapes[i][1] % 8 != 0 for i in with_pixels), "ragged_at_256 takes frames whose width is no multiple of 8"
        by_rows = sorted(with_pixels, key=lambda i: shapes[i][0])
        last = by_rows[0] if last is None else last
        cross = by_rows[-1] if cross is None else cross
        cursor = 0
        for i in with_pixels:
            strides[i] = batch_pitch(shapes[i][1])
            if i not in (last, cross):
                offsets[i] = cursor
                cursor += strides[i] * shapes[i][0]
        size_last, size_cross = strides[last] * shapes[last][0], strides[cross] * shapes[cross][0]
        register_to = align_up(cursor + size_last + size_cross + 256, PAGE)
        offsets[last] = register_to - size_last
        offsets[cross] = register_to + 16 - size_cross
        end = register_to + 16
    return Arena(frames, layout, poison, offsets, strides, end, register_to)


def crops_of_a_strip(picture, windows, poison):
    """Frames that are row windows [(first row, rows), ...] of ONE dense picture whose width is a multiple of 8 - dense at the staged pitch,
    free to overlap - in an arena that is to be registered as a whole -> Arena (frames: the windows' pixels; rows of the picture that no window
    holds are poison like everything else)."""
    picture = np.ascontiguousarray(picture, np.uint8)
    h, w = picture.shape
    assert w % 8 == 0 and all(0 <= a and a + b <= h for a, b in windows)
    return Arena([picture[r: r + m] for r, m in windows], "crops_of_a_strip", poison, [r * w for r, _ in windows], [w] * len(windows), h * w, "all")
