"""The device entropy encoder on BUILT coefficients (tests/entropy_blocks.py; tests/golden/entropy_blocks.json holds what the unmodified
reference's compress() wrote for them): both default-table packers with the placing kernel, the size kernel and the adaptive kernels,
through the C-ABI, on the states pixels cannot reach - 1,662-bit blocks, every zero run at every lane boundary, blocks of exactly 512 and
513 bits, symbols without a code, DC differences of category 11 where the previous DC comes from another wave, partition ends at every
residue mod 32, long and 48-bit staging slots under one placing workgroup.  tests/test_entropy_blocks_cpu.py shows on the CPU that every
frame reaches its edge (the census) and that the oracle writes the fixture's streams; here the fixture is the expectation and the oracle
only names the first differing byte when a stream is wrong."""
import ctypes as C

import numpy as np
import pytest

import decoder_streams as DS
import entropy_blocks as EB
import inverse_edges as IE

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

pytestmark = pytest.mark.gpu

SENTINEL = 256
LANE_OWN_CONTEXT = ("lane_limit", "dense_max")  # a fresh context each: the first attempt is then known to be the lane-per-block kernel


@pytest.fixture(scope="module")
def fx():
    return EB.load_fixture()["frames"]


@pytest.fixture(scope="module")
def lengths(oracle):
    return EB.Lengths(oracle.dump_tables())


@pytest.fixture(scope="module")
def frames(fx, lengths):
    out = EB.build_frames(lengths)
    assert set(out) == set(fx)
    for name, fr in out.items():
        assert EB.coeff_sha(fr["zz"]) == fx[name]["coeffs_sha256"], name
    return out


@pytest.fixture(scope="module")
def decoded():
    """tests/golden/decoder_streams.json: what the reference decodes the frames to."""
    return DS.load_fixture()


@pytest.fixture(scope="module")
def decoder_frames(lengths):
    return DS.build_frames(lengths)


def names(fx, family):
    return [n for n, e in fx.items() if e["family"] == family]


class Device:
    """A context with a coefficient buffer and a stream buffer for the largest frame of the fixture, reused by every call."""

    def __init__(self, lane_kernel=False):
        self.L = N.load()
        self.ctx = T.Context(0)
        assert self.ctx.arch.startswith("gfx950"), self.ctx.arch
        self.lane_kernel = lane_kernel
        self.max_cap = self.L.tic_compress_bound(EB.BASE_H, EB.BASE_W)
        self.d_zz, self.d_out = C.c_void_p(), C.c_void_p()
        self.ctx.check(self.L.tic_dev_alloc(self.ctx.handle, EB.BASE_N * 128, C.byref(self.d_zz)))
        self.ctx.check(self.L.tic_dev_alloc(self.ctx.handle, self.max_cap + SENTINEL, C.byref(self.d_out)))

    def arm(self):
        """The lane-per-block kernel for every quality again (a fallback lowers the limit for the rest of the context's life)."""
        self.ctx.check(self.L.tic_set_entropy_lane_kernel(self.ctx.handle, 99))

    def upload(self, fr):
        zz = fr["zz"]
        assert zz.dtype == np.int16 and zz.flags.c_contiguous and zz.nbytes <= EB.BASE_N * 128
        self.ctx.check(self.L.tic_memcpy_h2d(self.ctx.handle, self.d_zz, zz.ctypes.data, zz.nbytes))

    def encode(self, fr):
        """tic_entropy_encode_dev into a buffer of 0xFF bytes with a sentinel behind its tic_compress_bound() bytes -> (rc, stream)."""
        L, ctx = self.L, self.ctx
        cap = L.tic_compress_bound(fr["h"], fr["w"])
        assert cap <= self.max_cap
        self.upload(fr)
        ctx.check(L.tic_memset_dev(ctx.handle, self.d_out, 0xFF, cap))
        ctx.check(L.tic_memset_dev(ctx.handle, C.c_void_p(self.d_out.value + cap), 0xA5, SENTINEL))
        n = C.c_size_t(0)
        rc = L.tic_entropy_encode_dev(ctx.handle, self.d_zz, fr["h"], fr["w"], fr["quality"], self.d_out, cap, C.byref(n))
        got = np.empty(cap + SENTINEL, np.uint8)
        ctx.check(L.tic_memcpy_d2h(ctx.handle, got.ctypes.data, self.d_out, got.size))
        assert (got[cap:] == 0xA5).all(), "bytes behind the caller's buffer were written"
        assert n.value <= cap
        return rc, got[: n.value].tobytes()

    def size(self, fr):
        self.upload(fr)
        n = C.c_size_t(0)
        rc = self.L.tic_entropy_size_dev(self.ctx.handle, self.d_zz, fr["h"], fr["w"], C.byref(n))
        return rc, n.value

    def close(self):
        self.L.tic_dev_free(self.ctx.handle, self.d_zz)
        self.L.tic_dev_free(self.ctx.handle, self.d_out)
        self.ctx.close()


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


@pytest.fixture(scope="module")
def lane_dev():
    d = Device(lane_kernel=True)
    yield d
    d.close()


def check_stream(d, name, fx, frames, oracle, lengths, what):
    """One frame through tic_entropy_encode_dev: the fixture's bytes, or TIC_E_RANGE where the reference raised KeyError."""
    e, fr = fx[name], frames[name]
    rc, got = d.encode(fr)
    if "raises" in e["stream"]:
        assert e["stream"]["raises"] == "KeyError" and rc == N.TIC_E_RANGE, (what, name, rc)
        return
    assert rc == N.TIC_OK, (what, name, rc, N.load().tic_last_error(d.ctx.handle))
    if len(got) != e["stream"]["bytes"] or EB.sha(got) != e["stream"]["sha256"]:
        dc, ac = EB.dc_ac(fr["zz"])
        want = oracle.entropy_encode(dc, ac, fr["h"], fr["w"], fr["quality"])  # (diagnosis only)
        pytest.fail("%s, %s: %s" % (what, name, EB.first_difference(got, want, fr["zz"], lengths)))


@pytest.mark.parametrize("family", EB.FAMILIES)
def test_eight_lane_packer_and_placing(dev, fx, frames, oracle, lengths, family):
    """tic_entropy_encode_dev in a default context: entropy_pack_kernel and entropy_place_kernel.  In front of the families of short
    partitions the context packs dense_max, so that every staging slot holds 13,296 stale bits when 48-bit partitions are placed."""
    order = names(fx, family)
    if family in ("runs", "alignment", "long_short"):
        order = ["dense_max", "zeros"] + order
    for name in order:
        check_stream(dev, name, fx, frames, oracle, lengths, "8-lane packer")


@pytest.mark.parametrize("family", [f for f in EB.FAMILIES if f not in LANE_OWN_CONTEXT])
def test_lane_per_block_packer_and_placing(lane_dev, fx, frames, oracle, lengths, family):
    """The same with tic_set_entropy_lane_kernel(ctx, 99): entropy_pack_lane_kernel<16> first for every frame (armed again in front of
    each: a frame with a block beyond 512 bits is packed again by the 8-lane kernel and lowers the context's limit)."""
    order = names(fx, family)
    if family in ("runs", "alignment", "long_short"):
        order = ["dense_max", "zeros"] + order
    for name in order:
        lane_dev.arm()
        check_stream(lane_dev, name, fx, frames, oracle, lengths, "lane-per-block packer")


@pytest.mark.parametrize("first", ["lane_limit_none", "lane_limit_last", "lane_limit_first", "dense_max"])
def test_lane_per_block_limit_and_fallback(fx, frames, oracle, lengths, first):
    """A fresh context: its first frame has no block beyond 512 bits (511 and 512 are there), one of 513 - in the last, partial partition
    or in block 0 - or 1,662 bits in every block.  The fixture's bytes either way, and again for the runs frames encoded behind it in the
    same context (quality 37: still the lane-per-block kernel; 50: the 8-lane kernel once the limit dropped to 49 or 98 ... whichever
    kernel, the same bytes), then for the first frame once more."""
    d = Device(lane_kernel=True)
    try:
        d.arm()
        group = names(fx, "dense_max") if first == "dense_max" else [first]
        for name in group:
            if first == "dense_max":
                d.arm()  # every dense frame meets the lane-per-block kernel first
            check_stream(d, name, fx, frames, oracle, lengths, "fresh lane-kernel context")
        for name in ("runs_permuted", "runs_ordered", "zeros", group[0]):
            check_stream(d, name, fx, frames, oracle, lengths, "behind " + first)
    finally:
        d.close()


@pytest.mark.parametrize("family", EB.FAMILIES)
def test_size_kernel(dev, fx, frames, family):
    """tic_entropy_size_dev: the length of the reference's stream, or TIC_E_RANGE where it raised."""
    for name in names(fx, family):
        e, fr = fx[name], frames[name]
        rc, n = dev.size(fr)
        if "raises" in e["stream"]:
            assert rc == N.TIC_E_RANGE, (name, rc, n)
        else:
            assert (rc, n) == (N.TIC_OK, e["stream"]["bytes"]), name
            if family == "dense_max":
                assert T.entropy_size(fr["zz"], fr["h"], fr["w"]) == e["stream"]["bytes"], name


@pytest.mark.parametrize("family", EB.FAMILIES)
def test_adaptive_kernels(dev, fx, frames, decoded, family):
    """T.entropy_encode_adaptive: the stream the reference wrote with the frame's own tables (the three adaptive kernels; the table itself
    is built on the host), or its exception - OverflowError for a category 16, which the table's 4-bit field cannot hold.  The library's
    decoder reads every stream back to the pixels of the reference's decode() of the frame's dictionary (its own decompress() misreads
    the adaptive flag): as recorded with the default-table stream of the same frame and quality where tests/golden/decoder_streams.json
    has one, else the digest recorded there for this purpose."""
    for name in names(fx, family):
        e, fr = fx[name], frames[name]
        if "raises" in e["adaptive"]:
            assert e["adaptive"]["raises"] == "OverflowError", name
            with pytest.raises(OverflowError):
                T.entropy_encode_adaptive(fr["zz"], fr["h"], fr["w"], fr["quality"], ctx=dev.ctx)
            continue
        got = T.entropy_encode_adaptive(fr["zz"], fr["h"], fr["w"], fr["quality"], ctx=dev.ctx)
        assert (len(got), EB.sha(got)) == (e["adaptive"]["bytes"], e["adaptive"]["sha256"]), (name, len(got), e["adaptive"]["bytes"])
        px = T.decompress_adaptive(got, ctx=dev.ctx)
        assert px.shape == (fr["h"], fr["w"]) and px.dtype == np.uint8, name
        if name in decoded["frames"]:
            want = decoded["frames"][name]["streams"]["q%d" % fr["quality"]]["pixels_sha256"]
        else:
            want = decoded["adaptive_pixels"][name]
        assert IE.px_sha(px) == want, (name, "the adaptive decode kernels' pixels are not the reference's")


@pytest.mark.parametrize("name", [n for n, e in DS.load_fixture()["frames"].items() if e["family"] in DS.NEW_FAMILIES and not DS.is_twin(n)])
def test_adaptive_kernels_on_the_decoder_frames(dev, decoded, decoder_frames, oracle, name):
    """The frames built for the device decoder (tests/decoder_streams.py: every fused pair, every long codeword, spikes, full ranges, the
    int16 boundary of the DC) with their own tables: entropy_encode_adaptive -> decompress_adaptive gives the pixels the reference
    decoded the default-table stream of the same coefficients and quality to."""
    fr = decoder_frames[name]
    q = max(v[1] for v in fr["variants"] if not v[0])
    got = T.entropy_encode_adaptive(fr["zz"], fr["h"], fr["w"], q, ctx=dev.ctx)
    px = T.decompress_adaptive(got, ctx=dev.ctx)
    if px.shape != (fr["h"], fr["w"]) or IE.px_sha(px) != decoded["frames"][name]["streams"]["q%d" % q]["pixels_sha256"]:
        want = oracle.decompress(DS.with_header(DS.payload_stream(oracle, fr), fr, (0, q)))  # (diagnosis only: the same coefficients)
        pytest.fail("%s q%d: %s" % (name, q, DS.first_difference(px, want)))
