"""One long-lived context as state: every family of calls (tests/context_state_common.py) out of poisoned allocations, after every family it
shares a scratch buffer with, across grow and shrink, after every error the suite can produce, with tickets open and across the wrap of
the decoder's epoch.  Every comparison is exact - bytes and integers - against the oracle's result or a fixture of the unmodified
reference; nothing here waits for a hang, every check is of values after calls that returned.  DESIGN.md section 9 says which buffers
tic_test_poison and TIC_POISON fill and which they must never touch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import context_state_common as CS
import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

pytestmark = pytest.mark.gpu
BYTES = CS.POISON_BYTES


@pytest.fixture()
def ctx():
    c = T.Context(0)
    yield c
    c.close()


def poison(ctx, byte):
    """tic_test_poison -> (scratch buffers filled, bytes filled, state buffers kept), as the call reports them."""
    import re

    ctx.check(N.load().tic_test_poison(ctx.handle, byte))
    m = re.match(r"tic_test_poison: (\d+) scratch buffers and (\d+) bytes filled with 0x%02x, (\d+) state buffers kept" % byte,
                 N.load().tic_last_error(ctx.handle).decode())
    assert m, N.load().tic_last_error(ctx.handle)
    return tuple(int(g) for g in m.groups())


def test_hook_is_this_build_s(ctx):
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    assert L.tic_test_poison(ctx.handle, 256) == N.TIC_E_ARG and L.tic_test_poison(ctx.handle, -1) == N.TIC_E_ARG
    assert L.tic_test_poison(None, 0) == N.TIC_E_ARG
    filled, nbytes, kept = poison(ctx, 0xA5)  # (a context that has allocated next to nothing yet)
    assert filled == 0 and nbytes == 0 and kept == 5  # d_consts, d_huff, d_total_bits, h_stat, d_fallback


def test_poison_reaches_every_buffer_the_families_use(ctx, monkeypatch):
    """After every family's dense case the registry holds every scratch name of the records (several of some: slots, lanes) and every
    state name; the fill covers at least the pixels, coefficients and streams of the dense frames."""
    for f in CS.FAMILIES:
        f.check(ctx, "dense", monkeypatch)
    filled, nbytes, kept = poison(ctx, 0x5A)
    assert filled >= len(CS.SCRATCH) - 1 and kept >= len(CS.STATE), (filled, kept)  # (d_dc32 only exists once a DC has left int16)
    assert nbytes > 40 * CS.DENSE[0][0].size, nbytes
    for f in CS.FAMILIES:
        f.check(ctx, "small", monkeypatch, "(everything the context holds filled with 0x5A)")


# ---- poisoned allocation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", BYTES, ids=lambda b: "0x%02X" % b)
def test_poisoned_allocation(byte, monkeypatch):
    """A fresh context under TIC_POISON: every family's small case first - each buffer is first used at its smallest size, straight out of
    a poisoned allocation - then the dense cases (every buffer grows: poisoned again), then the small ones once more."""
    monkeypatch.setenv("TIC_POISON", "0x%02X" % byte)
    ctx, bad = T.Context(0), []
    try:
        for k, which in enumerate(("small", "dense", "small")):
            for f in CS.FAMILIES:
                f.check(ctx, which, monkeypatch, "(TIC_POISON=0x%02X, pass %d, over the %s cases)" % (byte, k, which), bad)
    finally:
        ctx.close()
    assert not bad, "\n".join(bad)


# ---- dirty, then small ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", CS.FAMILIES, ids=repr)
def test_dirty_then_small(a, ctx, monkeypatch):
    """For every family B that shares a scratch buffer with A (by the records' names; A itself included): A's dense case, then B's small
    case - once on A's real leftovers, once more with every scratch buffer filled with each of the three bytes in between."""
    partners, bad = [b for x, b in CS.sharing_pairs() if x is a], []
    assert a in partners
    for b in partners:
        for byte in (None,) + BYTES:
            a.check(ctx, "dense", monkeypatch, "(as the dirtying call in front of %s)" % b.name, bad)
            if byte is not None:
                poison(ctx, byte)
            b.check(ctx, "small", monkeypatch, "(after %s's dense case%s)" % (a.name, "" if byte is None else ", scratch filled with 0x%02X" % byte), bad)
    assert not bad, "\n".join(bad)


# ---- grow and shrink inside a family ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", CS.FAMILIES, ids=repr)
def test_grow_and_shrink(f, ctx, monkeypatch):
    bad = []
    for k, which in enumerate(("small", "dense", "ragged", "small")):
        poison(ctx, BYTES[k % 3])
        f.check(ctx, which, monkeypatch, "(step %d of small, dense, ragged, small; scratch filled with 0x%02X)" % (k, BYTES[k % 3]), bad)
    assert not bad, "\n".join(bad)


# ---- after an error -----------------------------------------------------------------------------------------------------------------------
def _raises(exc, fn):
    with pytest.raises(exc):
        fn()
    return "raised"


def _err_range_single(ctx, mp):
    """A coefficient without a Huffman code: the int16 frame of wide_pixels.npz (host entropy coder) and 8-bit noise at quality 99 (the
    device entropy stage raises its flag)."""
    d = np.load(os.path.join(CS.GOLDEN, "wide_pixels.npz"))
    return (_raises(KeyError, lambda: T.compress(d["int16_full_img"], 50, ctx=ctx)), _raises(KeyError, lambda: T.compress(CS.DENSE[0][0], 99, ctx=ctx)))


def _err_range_later_chunk(ctx, mp):
    """... in the last chunk of a mixed batch of one frame per chunk."""
    mp.setenv("TIC_BATCH_CHUNK", "1")
    frames = [img for img, _ in CS.SMALL] + [CS.DENSE[0][0]]
    try:
        return _raises(KeyError, lambda: T.compress_batch(frames, [q for _, q in CS.SMALL] + [99], ctx=ctx))
    finally:
        mp.delenv("TIC_BATCH_CHUNK")


def _err_truncated(ctx, mp):
    """Truncated streams: tic_decompress gives what the reference gives (truncated_streams.npz), on the device decoder's route and the
    host's; the strict adaptive decoder refuses one (TIC_E_STREAM)."""
    d = np.load(os.path.join(CS.GOLDEN, "truncated_streams.npz"))
    for env in (CS.DEVICE_ROUTE, CS.HOST_ROUTE):
        for k in CS.DEVICE_ROUTE:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        for name in d["names"]:
            assert np.array_equal(T.decompress(d[str(name) + "_bs"].tobytes(), ctx=ctx), d[str(name) + "_out"]), name
    s = bytes.fromhex(CS.adaptive_frame(CS.ADAPT_DENSE[0])[0]["stream"])
    return (_raises(ValueError, lambda: T.decompress_adaptive(s[: len(s) // 2], ctx=ctx)),
            _raises(ValueError, lambda: T.decompress_batch_adaptive([s, s[: len(s) // 2]], ctx=ctx)))


def _c_compress(ctx, img, q, cap):
    out, n = np.full(cap + 64, 0xAB, np.uint8), C.c_size_t(0)
    rc = N.load().tic_compress(ctx.handle, img.ctypes.data, img.shape[0], img.shape[1], img.shape[1], q, out.ctypes.data, cap, C.byref(n))
    assert np.all(out[cap:] == 0xAB), "tic_compress wrote behind the capacity it was given"
    return rc


def _err_space(ctx, mp):
    """An output buffer one byte short: the small frame (host-mapped route) and the dense one (device stream buffer)."""
    out = []
    for img, q in (CS.SMALL[1], CS.DENSE[0]):
        rc = _c_compress(ctx, img, q, len(CS.oracle().compress(img, q)) - 1)
        assert rc == N.TIC_E_SPACE, rc
        out.append(rc)
    return out


def _err_argument(ctx, mp):
    img = CS.SMALL[1][0]
    rcs = [_c_compress(ctx, img, 0, 4096), _c_compress(ctx, img, 100, 4096)]
    out, n = np.zeros(4096, np.uint8), C.c_size_t(0)
    rcs.append(N.load().tic_compress(ctx.handle, img.ctypes.data, -1, 24, 24, 50, out.ctypes.data, 4096, C.byref(n)))
    rcs.append(N.load().tic_compress(ctx.handle, img.ctypes.data, 16, 24, 8, 50, out.ctypes.data, 4096, C.byref(n)))  # (rows overlap)
    assert all(rc in (N.TIC_E_ARG, N.TIC_E_QUALITY) for rc in rcs), rcs
    return rcs


def _err_lane_overflow(ctx, mp):
    """The lane-per-block packer turned on for every quality, then dense noise at quality 98, whose blocks need more than the packer's 512
    bits (the dense stream averages 688 bits per block): the stage is to run again with the 8-lane kernel and the stream is exact.  That the
    first kernel overflowed is not asserted - the library has no getter for it; what is asserted is that a context with the lane kernel on
    gives exact streams here, in every family behind it, and in the same call again."""
    img, q = CS.DENSE[0]
    assert (len(CS.oracle().compress(img, q)) - 16) * 8 > 512 * (img.size // 64)  # (more than 512 bits per block on average)
    ctx.check(N.load().tic_set_entropy_lane_kernel(ctx.handle, 99))
    got = T.compress(img, q, ctx=ctx)
    assert got == CS.oracle().compress(img, q)
    return got


def _err_header_guess(ctx, mp):
    """tic_decompress_dev launches on a guess of the header after two equal ones; a stream of another quality makes the guess wrong: it is
    decoded again and exact."""
    for k, v in CS.DEVICE_ROUTE.items():
        mp.setenv(k, v)
    f = CS.BY_NAME["decompress_dev[device]"]
    img = CS.DENSE[0][0]
    for _ in range(3):
        assert CS.norm(f.run(ctx, CS.DENSE)) == f.expected("dense")
    other = ((img, 60),)
    got = CS.norm(f.run(ctx, other))
    guess = N.load().tic_last_decode_guess(ctx.handle)
    assert got == CS.norm(CS.exp_pixels(other))
    assert guess == -1, "the header guess was not wrong (%d): the case does not reach the path it is about" % guess
    return got


ERRORS = {
    "range_single": (_err_range_single, "compress"),
    "range_later_chunk": (_err_range_later_chunk, "compress_batch[mixed]"),
    "truncated_stream": (_err_truncated, "decompress[device]"),
    "space_one_byte_short": (_err_space, "compress"),
    "bad_argument": (_err_argument, "compress"),
    "lane_kernel_overflow": (_err_lane_overflow, "compress"),
    "wrong_header_guess": (_err_header_guess, "decompress_dev[device]"),
}


@pytest.mark.parametrize("name", ERRORS, ids=str)
def test_after_an_error(name, ctx, monkeypatch):
    """The failing call; every family's small case, exact; the failing call again, failing the same way; a good call of the same family
    twice - the two flags used in turn are both clean."""
    fail, family = ERRORS[name]
    first, bad = CS.norm(fail(ctx, monkeypatch)), []
    for f in CS.FAMILIES:
        f.check(ctx, "small", monkeypatch, "(after the error %s)" % name, bad)
    assert not bad, "\n".join(bad)
    assert CS.norm(fail(ctx, monkeypatch)) == first, "%s: the second failure differs from the first" % name
    for k in range(2):
        CS.BY_NAME[family].check(ctx, "dense", monkeypatch, "(good call %d after the error %s)" % (k, name))
        CS.BY_NAME[family].check(ctx, "small", monkeypatch, "(good call %d after the error %s)" % (k, name))


# ---- tickets ------------------------------------------------------------------------------------------------------------------------------
def _burst():
    """small, dense, small ... : 3 + 1 + 3 + 1 frames, so that both lanes take both kinds and four decode slots are used twice."""
    frames = list(CS.SMALL) + list(CS.DENSE) + list(CS.SMALL) + list(CS.DENSE)
    order = [5, 0, 7, 2, 3, 6, 1, 4]  # collected out of order
    return frames, order


def test_compress_tickets(ctx, monkeypatch):
    L = N.load()
    CS.BY_NAME["compress_dev_async"].check(ctx, "dense", monkeypatch, "(warm-up: the lanes exist)")
    poison(ctx, 0xA5)
    frames, order = _burst()
    want = [CS.oracle().compress(img, q) for img, q in frames]
    tickets = CS.open_compress_tickets(ctx, frames)
    assert L.tic_test_poison(ctx.handle, 0xFF) == N.TIC_E_BUSY
    got = {}
    for n, i in enumerate(order):
        got[i] = CS.collect_compress_ticket(ctx, tickets[i])
        assert L.tic_test_poison(ctx.handle, 0xFF) == (N.TIC_E_BUSY if n + 1 < len(order) else N.TIC_OK)
    assert [got[i] for i in range(len(frames))] == want
    CS.BY_NAME["compress_dev_async"].check(ctx, "small", monkeypatch, "(after the burst and a poison)")


def test_decompress_tickets(ctx, monkeypatch):
    """A ticket is launched on a slot (its own stream, workspace, look-back and status words) behind two equal headers, on a guess of the
    next one; so the bursts are of one frame each.  After a warm-up that gives every slot a workspace of the dense size, and a fill of
    everything: four dense tickets (all launched, on the filled workspaces, the guess holds), twice four small ones (behind the header's
    change tickets run synchronously or are decoded again; then all four are launched and hold), twice four dense ones (the same).
    Every burst is collected out of order; the fill is refused while a ticket is open; what became of each ticket is the hooks build's
    own report (tic_last_error)."""
    L = N.load()
    f = CS.BY_NAME["decompress_dev_async[device]"]
    f.check(ctx, "dense", monkeypatch, "(warm-up: six tickets, every slot has launched one)")
    filled = poison(ctx, 0xA5)
    small, dense = CS.DEV_SMALL[0], CS.DENSE[0]
    held, slots = [], set()
    for frame, all_hold in ((dense, True), (small, False), (small, True), (dense, False), (dense, True)):
        want = CS.norm(CS.exp_pixels((frame,)))[0]
        tickets = CS.open_decompress_tickets(ctx, (frame,) * 4)
        assert L.tic_test_poison(ctx.handle, 0xFF) == N.TIC_E_BUSY
        count = 0
        for n, i in enumerate((2, 0, 3, 1)):
            assert CS.norm(CS.collect_decompress_ticket(ctx, tickets[i])) == want
            t = CS.last_ticket(ctx)
            assert t and t["ticket"] == tickets[i][0], t
            count += t["launched"] and t["held"]
            if all_hold:
                slots.add(t["slot"])
            assert L.tic_test_poison(ctx.handle, 0xFF) == (N.TIC_E_BUSY if n < 3 else N.TIC_OK)
        held.append(count)
        assert count == 4 or not all_hold, "tickets launched on a slot with a guess that held, per burst so far: %s" % held
    assert slots == {0, 1, 2, 3}
    assert poison(ctx, 0x00)[0] == filled[0]  # (the same buffers: nothing was regrown, the first burst ran on filled workspaces)
    f.check(ctx, "small", monkeypatch, "(after the bursts and a poison)")


# ---- ownership and teardown -------------------------------------------------------------------------------------------------------------------
def _exact_8x8(ctx):
    img, q = CS.SMALL[0]
    s = T.compress(img, q, ctx=ctx)
    assert s == CS.oracle().compress(img, q) and np.array_equal(T.decompress(s, ctx=ctx), CS.oracle().decompress(s))


def test_registry_is_ownership(monkeypatch):
    """What the registry records is what the context owns: after every family's dense case on a fresh context, the buffers
    tic_test_poison walks are the buffers allocated since the context was made (other contexts of the process may be alive: base)."""
    live = N.load().tic_test_live_buffers
    base = live()
    assert base >= 0
    ctx = T.Context(0)
    try:
        assert live() - base == 5  # d_consts, d_huff, d_total_bits, h_stat, d_fallback
        for f in CS.FAMILIES:
            f.check(ctx, "dense", monkeypatch)
        filled, _, kept = poison(ctx, 0x5A)
        assert filled >= len(CS.SCRATCH) - 1 and kept >= len(CS.STATE), (filled, kept)
        assert filled + kept == live() - base, (filled, kept, live(), base)
    finally:
        ctx.close()
    assert live() == base


def test_destroy_frees_everything(monkeypatch):
    """Three contexts in turn: every family's small case, the batch families' dense cases (the slots grow, some one by one), close - and
    the process owns what it owned before.  Then a new context is exact."""
    live = N.load().tic_test_live_buffers
    base = live()
    for k in range(3):
        ctx = T.Context(0)
        try:
            for f in CS.FAMILIES:
                f.check(ctx, "small", monkeypatch, "(context %d)" % k)
            for f in CS.FAMILIES:
                if "batch" in f.name:
                    f.check(ctx, "dense", monkeypatch, "(context %d)" % k)
            assert live() - base > len(CS.SCRATCH)
        finally:
            ctx.close()
        assert live() == base, "context %d left %d buffers behind" % (k, live() - base)
    ctx = T.Context(0)
    try:
        _exact_8x8(ctx)
    finally:
        ctx.close()
    assert live() == base


def test_destroy_with_tickets_open(monkeypatch):
    """Closing a context with a compress and a decode ticket issued and never collected is a supported call: tic_destroy waits for every
    stream first.  Everything the context owned is freed, the frames' own device buffers outlive it, and a new context is exact."""
    live = N.load().tic_test_live_buffers
    base = live()
    for k, v in CS.DEVICE_ROUTE.items():
        monkeypatch.setenv(k, v)
    ctx = T.Context(0)
    try:
        f = CS.BY_NAME["decompress_dev_async[device]"]
        f.check(ctx, "dense", monkeypatch, "(warm-up: the next ticket is launched on a slot)")
        (ct,) = CS.open_compress_tickets(ctx, CS.DENSE)
        (dt,) = CS.open_decompress_tickets(ctx, CS.DENSE)
        assert N.load().tic_test_poison(ctx.handle, 0xFF) == N.TIC_E_BUSY  # (both are open)
    finally:
        ctx.close()
    assert live() == base
    ctx = T.Context(0)
    try:
        # the closed context waited for both frames: their outputs, in the caller's buffers, are whole
        ct[2].ctx = dt[2].ctx = ctx
        want = CS.oracle().compress(*CS.DENSE[0])
        assert ct[2].down(len(want)).tobytes() == want
        h, w = CS.DENSE[0][0].shape
        assert np.array_equal(dt[2].down(h * w).reshape(h, w), CS.oracle().decompress(want))  # (w is a multiple of 8: rows without a gap)
        for d in (ct[1], ct[2], dt[1], dt[2]):
            d.ctx = ctx
            d.free()
        _exact_8x8(ctx)
    finally:
        ctx.close()
    assert live() == base


# ---- epoch wrap ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["decompress[device]", "decompress_dev_async[device]", "decompress_batch[device]"])
def test_epoch_wrap(name, ctx, monkeypatch):
    """Three workspaces: tic_decompress's, a decode ticket's slot and the batch's.  Under TIC_DEC_EPOCH three short of 2^22 the dense
    stream stamps many look-back words with an epoch just below 2^22; the 24 x 32 stream then crosses the wrap (the words are cleared on
    the workspace's stream, the epoch starts over at 1) and runs behind it, and so does the dense stream.  The hooks build reports the
    epoch of every run (tic_last_error), so the test reads that the wrap was reached: 2^22 - 2, 2^22 - 1, 1, 2 for tic_decompress and
    for the batch (four frames per call, one run of its kernels).  Tickets go to their slots in turn, eight frames per step, so that every
    slot takes two runs per step and the last ticket of a step is launched on a guess that holds: 2^22 - 2 and 2^22 - 1 on every slot
    under the variable, the wrap on every slot in the first step behind it."""
    f = CS.BY_NAME[name]
    tickets = "async" in name
    k = 1 if name.startswith("decompress[") else (8 if tickets else 4)
    dense, mid = CS.DENSE * k, (CS.DEV_SMALL[0],) * k
    epoch = (lambda: CS.last_ticket(ctx)["epoch"]) if tickets else (lambda: CS.last_epoch(ctx)[1])
    assert f.route is not None and f.route_all
    f.check(ctx, dense, monkeypatch, "(the workspaces exist)")
    monkeypatch.setenv("TIC_DEC_EPOCH", str((1 << 22) - 3))
    f.check(ctx, dense, monkeypatch, "(just below 2^22)")
    monkeypatch.delenv("TIC_DEC_EPOCH")
    seen = [epoch()]
    for step in range(3):
        f.check(ctx, mid, monkeypatch, "(run %d across the epoch's wrap)" % step)
        seen.append(epoch())
    assert seen == ([(1 << 22) - 1, 2, 4, 6] if tickets else [(1 << 22) - 2, (1 << 22) - 1, 1, 2]), seen
    f.check(ctx, "small", monkeypatch, "(behind the wrap)")
    f.check(ctx, dense, monkeypatch, "(behind the wrap)")


# ---- the shipped library --------------------------------------------------------------------------------------------------------------------
def test_shipped_library_dirty_then_small():
    """The pairs of test_dirty_then_small with nothing in between, on libtinyimgcodec_hip.so in a fresh child process; tic_test_poison is
    TIC_E_ARG there and tic_test_live_buffers -1.  The shipped library reads no hook variable, so the seven [device] decoder families - which exist by those variables
    - cannot run on it and are left out, with their pairs (541 of the 912 remain): there the decoder families take the host route, which
    is asserted."""
    code = r'''
import os, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N
import context_state_common as CS
L = N.load()
assert L.tic_build_has_test_hooks() == 0 and N._lib_path() == N.LIB_PATH
class NoEnv:
    def setenv(self, k, v): pass
    def delenv(self, k, raising=True): pass
ctx = T.Context(0)
assert L.tic_test_poison(ctx.handle, 0xA5) == N.TIC_E_ARG
assert L.tic_test_live_buffers() == -1  # (no counter in the shipped library)
fams = [f for f in CS.FAMILIES if not f.env]
n = 0
for a, b in CS.sharing_pairs():
    if a in fams and b in fams:
        a.check(ctx, "dense", NoEnv(), "(shipped library, in front of %s)" % b.name)
        b.check(ctx, "small", NoEnv(), "(shipped library, after %s's dense case)" % a.name)
        n += 1
assert L.tic_test_poison(ctx.handle, 0xA5) == N.TIC_E_ARG
ctx.close()
print("shipped library ok:", n, "pairs")
'''
    env = {k: v for k, v in os.environ.items() if not k.startswith("TIC_")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and "shipped library ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
