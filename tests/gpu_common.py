"""Constants and small helpers of the GPU tests (test infrastructure only): pointers and split-fp16 planes, the project's tolerances, the
product's tile ids, the per-layer bound, the fenced output buffer, the sentinel-filled input staging with its bit-for-bit check and the `dev` fixture.  A test file imports what it uses by name, the
fixture included (`from gpu_common import dev  # noqa: F401`)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import rise_ref

SCORE_TOL = 1e-4            # the project's tolerance on a score: the ceiling of the end-to-end bound
SCORE_BOUND = 2e-5          # ... and its end-to-end bound
LAYER_TOL = 4e-6            # relative to max(|want|, 1), times sqrt(max(K, 4608) / 4608): layer_bound
# Every product tile id: the rows of kTiles in csrc/mpx_api.hip (tests/test_host_logic.py holds this tuple to that table).  16 and 18 are the
# grouped 3x3 kernels, which every layer that is not grouped refuses.
ALL_TILES = (0, 1, 2, 4, 6, 7, 9, 10, 12, 13, 14, 16, 18)
GENERIC = {0, 1, 2, 4, 7}
FALLBACK = {9: 2, 10: 7, 12: 6, 13: 2, 14: 7}        # the small-tile kernel a persistent / 256x256 launch may hand work to
FENCE_ROWS = 256                    # pixel rows in front of and behind every fenced output plane
SENTINEL_BITS = 0x7e00              # an fp16 NaN no kernel produces
F32_SENTINEL_BITS = 0x7fc01234      # an fp32 NaN with a payload no arithmetic produces


def ptr(t, offset=0):
    """The device (or host) pointer of tensor t, `offset` fp16 elements in; None stays None."""
    return C.c_void_p(t.data_ptr() + 2 * offset) if t is not None else None


def split(x):
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    return hi.contiguous(), lo.contiguous()


def merge(hi, lo):
    return hi.float() + lo.float()


def pitch_of(c):
    return -(-c // 32) * 32


def bits(t):
    return t.view(torch.int16).to(torch.int32) & 0xFFFF


def dev_view(p, n, dev):
    """n floats at a raw device pointer (a c_void_p the library handed out), copied to the host."""
    class _V:
        __cuda_array_interface__ = {"data": (p.value, False), "shape": (n,), "typestr": "<f4", "version": 2}
    return torch.as_tensor(_V(), device=dev).clone().cpu()


def round_up_one_digit(v):
    e = math.floor(math.log10(v))
    return math.ceil(v / 10 ** e - 1e-9) * 10 ** e


def layer_index(eng, name):
    return [d.name.decode() for d in eng.layers].index(name)


def accepted_tiles(eng, i):
    """The ids of ALL_TILES that mpx_set_conv_tile accepts for layer i, which is left on its default tile."""
    accepted = [t for t in ALL_TILES if eng._lib.mpx_set_conv_tile(eng._h, i, t) == 0]
    eng._lib.mpx_set_conv_tile(eng._h, i, -1)
    return accepted


def layer_bound(d, scale, k=None):
    """The project's per-layer bound on max |got - fp64| for conv layer d whose fp64 output reaches `scale`: the one place it is written.
    k: the length of the sums where it is not the layer's packed K (a grouped layer, two layers fused in one launch)."""
    return LAYER_TOL * math.sqrt(max(d.k_packed if k is None else k, 4608) / 4608) * max(scale, 1.0)


class Fenced:
    """rows x cout output elements between two fences of FENCE_ROWS pixel rows, everything prefilled with a NaN no kernel produces and
    compared by its bits: a store of any value into a fence shows, and so does a payload element that no store reached."""

    def __init__(self, rows, cout, dev, f32=False):
        self.fence, self.rows, self.cout = FENCE_ROWS * cout, rows, cout
        self.sentinel = F32_SENTINEL_BITS if f32 else SENTINEL_BITS
        self.bits = torch.full((2 * self.fence + rows * cout,), self.sentinel, dtype=torch.int32 if f32 else torch.int16, device=dev)
        self.values = self.bits.view(torch.float32 if f32 else torch.float16)

    @property
    def payload(self):
        return self.values[self.fence:self.fence + self.rows * self.cout].view(self.rows, self.cout)

    @property
    def payload_bits(self):
        return self.bits[self.fence:self.fence + self.rows * self.cout].view(self.rows, self.cout)

    def problems(self):
        """What a launch left wrong around and in the payload: [] when the fences are intact and every payload element was written."""
        out = []
        front, back = self.bits[:self.fence] != self.sentinel, self.bits[self.fence + self.rows * self.cout:] != self.sentinel
        if front.any():
            out.append("front fence: %d elements overwritten, the last at %d before the payload" % (int(front.sum()), self.fence - int(front.nonzero().max())))
        if back.any():
            out.append("back fence: %d elements overwritten, the first at %d behind the payload" % (int(back.sum()), int(back.nonzero().min())))
        left = self.payload_bits == self.sentinel
        if left.any():
            out.append("payload: %d elements never written, the first in pixel row %d" % (int(left.sum()), int(left.nonzero()[0, 0])))
        return out


class FencedPair:
    """The hi and lo plane of one split-fp16 output, each Fenced."""

    def __init__(self, rows, c, dev):
        self.hi, self.lo = Fenced(rows, c, dev), Fenced(rows, c, dev)

    def ptrs(self):
        return ptr(self.hi.payload), ptr(self.lo.payload)

    def result(self):
        """(hi, lo) [rows * c] once the launch is done: fences intact, every element written, no NaN."""
        torch.cuda.synchronize()
        for plane, which in ((self.hi, "hi"), (self.lo, "lo")):
            assert plane.problems() == [], "%s plane: %s" % (which, "; ".join(plane.problems()))
            assert not torch.isnan(plane.payload).any(), which
        return self.hi.payload.reshape(-1).clone(), self.lo.payload.reshape(-1).clone()


PLANE_IMG = 224
PLANE_SENTINEL = 0x5A3C     # fp16 bits of 199.5: neither 0 nor anything a normalised pixel times a weight splits into at every element


class Planes:
    """The engine's input staging filled with a sentinel for the length of a `with` block, and put back afterwards (the 3-pixel border is
    zero for the life of an engine and the stem conv reads it)."""

    def __init__(self, e):
        self.e = e
        self.hi, self.lo = (t.view(torch.int16) for t in e.input_planes())

    def __enter__(self):
        self.saved = self.hi.clone(), self.lo.clone()
        self.hi.fill_(PLANE_SENTINEL)
        self.lo.fill_(PLANE_SENTINEL)
        return self

    def __exit__(self, *exc):
        self.hi.copy_(self.saved[0])
        self.lo.copy_(self.saved[1])
        torch.cuda.synchronize()

    def read(self):
        torch.cuda.synchronize()
        return self.hi.cpu().numpy(), self.lo.cpu().numpy()

    def intact(self):
        hi, lo = self.read()
        return bool((hi == PLANE_SENTINEL).all() and (lo == PLANE_SENTINEL).all())


def check_planes(planes, x, w, slot0, out=None):
    """Slots [slot0, slot0 + M) hold split(fl(x * w[m])) bit for bit in channels 0..2 and +0.0 in channel 3; their 3-pixel border and every
    other slot still hold the sentinel; out (f32[M,3,224,224]) holds fl(x * w[m]) bit for bit."""
    hi, lo = planes.read()
    m = len(w)
    want = x.numpy()[None] * w[:, None]                             # [M,3,224,224] fp32: one rounded multiply
    assert want.dtype == np.float32
    whi, wlo = rise_ref.split16(want.transpose(0, 2, 3, 1))         # NHWC
    for name, got, exp in (("hi", hi, whi), ("lo", lo, wlo)):
        inner = got[slot0:slot0 + m, 3:3 + PLANE_IMG, 3:3 + PLANE_IMG]
        assert (inner[..., :3] == exp).all(), "%s plane differs from split(v * w) at %d elements" % (name, int((inner[..., :3] != exp).sum()))
        assert (inner[..., 3] == 0).all(), "%s: channel 3 is not +0.0" % name
        border = got[slot0:slot0 + m].copy()
        border[:, 3:3 + PLANE_IMG, 3:3 + PLANE_IMG] = PLANE_SENTINEL
        assert (border == PLANE_SENTINEL).all(), "%s: the 3-pixel border was written" % name
        assert (got[:slot0] == PLANE_SENTINEL).all() and (got[slot0 + m:] == PLANE_SENTINEL).all(), "%s: a slot outside [slot0, slot0 + M) was written" % name
    if out is not None:
        assert (out.cpu().numpy().view(np.int32) == want.view(np.int32)).all(), "out_f32_nchw differs from v * w"


@pytest.fixture(scope="module")
def dev(mpx_lib):
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda", 0)
