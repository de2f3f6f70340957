"""RegNetY-800MF .. -8GF on the GPU (run on the MI355X box: pytest -m gpu), everything through the C-ABI: the SE gate with ReLU
(mpx_se_gate_relu) against fp64 inside a propagated bound, against the SiLU gate, batch-independent bit for bit, its refusals and the device
vectors mpx_load_se made; the group-width-56 instantiation of the any-width grouped 3x3 kernel (csrc/mpx_gconvw.h, tile 18) on the cases of
tests/regnety_draws.py behind fences and inside their per-element bound (through the stand-alone entry mpx_gconvw3x3_bn_act: one group, a
ragged last workgroup, pad channels, regnet_y_8gf's group counts on its smallest maps, 5 x 5 maps); the descriptors, tiles, SE lists and
refusals of the four engines; every distinct conv shape of the four networks on every tile that accepts it; and the four networks end to end
on the rows tests/test_regnety_cpu.py holds the weights to.

The gate's bound is tests/test_gpu_efficientnet.py's, propagated through the same three phases, with SiLU's terms replaced: ReLU has slope
<= 1 and adds no rounding, so d_s1 = d_z1.
    d_pool = hw u mean|x|                                           (hw - 1 adds and one division, hi + lo exact)
    d_z1   = |W1| d_pool + (ceil(pitch / 64) + 7) u (|W1| |pooled| + |b1|)
    d_s1   = d_z1
    d_z2   = |W2| d_s1 + (q + 1) u (|W2| |s1| + |b2|)
    bound  = d_z2 / 4 + 4 u gate,  u = 2^-24
The case (8, 8, 1, 1, 1) has ONE fc1 pre-activation, which cannot be a quarter negative and a quarter positive: it runs twice, once with a
negative and once with a positive pre-activation; every other case asserts the two quarters on its own draws.

End to end, measured on one MI355X (d = fp32 batch-1 CPU loop against fp64 over the rows; 4 d < 2e-5 on all four, so the bound is 2e-5):
  regnet_y_800mf  6 rows: d 8.7e-07, engine - fp64 7.5e-07, engine - fp32 loop 4.9e-07; logits d_L 9.3e-06, engine 1.3e-05 (1.42 d_L)
  regnet_y_1_6gf  6 rows: d 2.2e-06, engine - fp64 2.1e-06, engine - fp32 loop 3.3e-06; logits d_L 1.3e-05, engine 2.0e-05 (1.57 d_L)
  regnet_y_3_2gf  6 rows: d 9.4e-07, engine - fp64 2.3e-06, engine - fp32 loop 3.3e-06; logits d_L 1.6e-05, engine 2.4e-05 (1.47 d_L)
  regnet_y_8gf    3 rows: d 1.4e-06, engine - fp64 4.6e-06, engine - fp32 loop 4.3e-06; logits d_L 2.5e-05, engine 4.1e-05 (1.67 d_L)
(8GF scores 3 rows, as regnet_x_8gf does: its fp64 CPU forward is the slowest of the four.)  Gate: worst err / bound 0.109; group width 56:
worst err / tol 0.340 (DESIGN.md 27 has the table).  The 169 tests take 9.4 s.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import regnety_draws as yd
import regnety_ref as ref
from gpu_common import dev, dev_view, Fenced, GENERIC, layer_bound, layer_index, merge, ptr, split  # noqa: F401  (dev is a fixture)
from net_harness import check_api, check_end_to_end, check_position_independence, Reference, stage_stem_input
from network_interpretation_imagenet_amd import _lib, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine

pytestmark = pytest.mark.gpu

ARCHS = ref.ARCHS
DENSE_TILES = (0, 1, 2, 4, 6, 7, 9, 10, 12, 13, 14)
EPS = 1e-5
U = 2.0 ** -24


@pytest.fixture(scope="module")
def sds():
    return {a: synth.make_state_dict(a) for a in ARCHS}


@pytest.fixture(scope="module")
def engines(dev, sds):
    """One small engine per network, with its synthetic weights."""
    out = {a: MaskedForwardEngine(a, max_batch=8, device=0).load_state_dict(sds[a]) for a in ARCHS}
    yield out
    for e in out.values():
        e.close()


@pytest.fixture(scope="module")
def eng(engines):
    """The engine the stand-alone entries are called on."""
    return engines["regnet_y_800mf"]


def _pitches(eng, i):
    pin, pout, off = C.c_int(), C.c_int(), C.c_int()
    assert eng._lib.mpx_conv_in_slice(eng._h, i, C.byref(pin), C.byref(off), None, None) == 0 and off.value == 0
    assert eng._lib.mpx_conv_out_slice(eng._h, i, C.byref(pout), C.byref(off)) == 0 and off.value == 0
    return pin.value, pout.value


def _sentinel(shape, dev):
    return torch.full(shape, yd.SENTINEL_BITS, dtype=torch.int16, device=dev).view(torch.float16)


def _at_pitch(x, pitch, pad_sentinel=False):
    """[..., width] -> contiguous [..., pitch] with the pad channels zero (or the NaN sentinel)."""
    out = _sentinel(x.shape[:-1] + (pitch,), x.device) if pad_sentinel else torch.zeros(x.shape[:-1] + (pitch,), dtype=x.dtype, device=x.device)
    out[..., :x.shape[-1]] = x
    return out.contiguous()


# ------------------------------------------------------------------------------------------------
# 1. the SE gate with ReLU
# ------------------------------------------------------------------------------------------------
def _se_inputs(c, pitch, hw, q, batch, seed, dev, sign=-1.0):
    """Planes (pads exact zeros; values >= 0 mostly, as behind f.b's ReLU, a tenth exact zeros, a dim band), fc1 [q][pitch] and fc2 j-major
    [q][pitch] with zero pad columns, b2 with -inf on the pads: the layout mpx_load_se uploads.  b1 is chosen so that image 0's fp64 fc1
    pre-activations are sign * (-2 .. 2) in even steps (in a shuffled order; q = 1: the one value is 2 sign), b2 so that image 0's fp64
    pre-sigmoid values are -4 .. 4 in even steps: ReLU cuts half of fc1's outputs and the gates cover (0, 1) whatever the draws."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(batch, hw, pitch, generator=g) * 2.0 + torch.randn(1, 1, pitch, generator=g)).clamp_min(-0.25)
    x[torch.rand(x.shape, generator=g) < 0.1] = 0.0
    x[..., : max(1, c // 4)] *= 1e-3
    x[..., c:] = 0.0
    w1 = torch.zeros(q, pitch)
    w1[:, :c] = torch.randn(q, c, generator=g) * (2.0 / c) ** 0.5
    w2 = torch.zeros(q, pitch)
    w2[:, :c] = torch.randn(q, c, generator=g) * (4.0 / q) ** 0.5
    xh, xl = split(x[:1])
    pooled = merge(xh, xl).double()[0, :, :c].mean(0)
    steps = torch.linspace(-2.0, 2.0, q) if q > 1 else torch.tensor([-2.0])
    b1 = ((-sign) * steps[torch.randperm(q, generator=g)].double() - pooled @ w1[:, :c].double().t()).float()
    s1 = torch.relu(pooled @ w1[:, :c].double().t() + b1.double())
    b2 = torch.full((pitch,), float("-inf"))
    b2[:c] = (torch.linspace(-4.0, 4.0, c)[torch.randperm(c, generator=g)].double() - s1 @ w2[:, :c].double()).float()
    return x.to(dev), w1.to(dev), b1.to(dev), w2.to(dev), b2.to(dev)


def _se_gate_run(eng, xh, xl, w1, b1, w2, b2, hw, pitch, q, entry="mpx_se_gate_relu"):
    batch = xh.shape[0]
    out = torch.full((batch * pitch + 64,), float("nan"), dtype=torch.float32, device=xh.device)
    rc = getattr(eng._lib, entry)(eng._h, ptr(xh), ptr(xl), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(out), batch, hw, pitch, q, eng._stream())
    _lib.check(eng._h, rc, entry)
    torch.cuda.synchronize()
    assert torch.isnan(out[batch * pitch:]).all(), "%s wrote behind its output" % entry
    return out[: batch * pitch].view(batch, pitch).clone()


def _se_gate_want(xh, xl, w1, b1, w2, b2, c, hw, pitch, q):
    """fp64 gates of the real channels, their propagated bound (module docstring) and fc1's fp64 pre-activations."""
    x = merge(xh, xl).double()[..., :c]                            # [B][hw][c]
    W1, B1, W2, B2 = w1[:, :c].double(), b1.double(), w2[:, :c].double(), b2[:c].double()
    pooled = x.mean(1)
    d_pool = hw * U * x.abs().mean(1)
    z1 = pooled @ W1.t() + B1
    d_z1 = d_pool @ W1.abs().t() + (math.ceil(pitch / 64) + 7) * U * (pooled.abs() @ W1.abs().t() + B1.abs())
    s1 = torch.relu(z1)
    d_s1 = d_z1
    z2 = s1 @ W2 + B2
    d_z2 = d_s1 @ W2.abs() + (q + 1) * U * (s1.abs() @ W2.abs() + B2.abs())
    gate = 1.0 / (1.0 + torch.exp(-z2))
    return gate, 0.25 * d_z2 + 4 * U * gate, z1


# channels, pitch, pixels, q, batch, sign of image 0's first pre-activation step.  (2016, 2016, 49, 224, 2): one slice, the channels strided
# over the 256 threads eight times, q far above the 4 waves
SE_CASES = [(8, 8, 1, 1, 1, -1.0), (8, 8, 1, 1, 1, 1.0), (16, 32, 49, 6, 3, -1.0), (144, 160, 196, 36, 2, -1.0), (64, 64, 3136, 8, 1, -1.0),
            (2016, 2016, 49, 224, 2, -1.0)]


@pytest.mark.parametrize("c,pitch,hw,q,batch,sign", SE_CASES)
def test_se_gate_relu_against_fp64(eng, dev, c, pitch, hw, q, batch, sign):
    x, w1, b1, w2, b2 = _se_inputs(c, pitch, hw, q, batch, seed=100 * c + hw, dev=dev, sign=sign)
    xh, xl = split(x)
    got = _se_gate_run(eng, xh, xl, w1, b1, w2, b2, hw, pitch, q)
    assert (got[:, c:].view(torch.int32) == 0).all()                                    # pad channels: exactly +0
    want, tol, z1 = _se_gate_want(xh, xl, w1, b1, w2, b2, c, hw, pitch, q)
    neg, pos = (z1 < 0).double().mean().item(), (z1 > 0).double().mean().item()
    if z1.numel() >= 4:
        assert neg >= 0.25 and pos >= 0.25, (neg, pos)                                  # ReLU is exercised on both sides
    else:
        assert z1.numel() == 1 and (z1 < 0).all().item() == (sign < 0) and (z1 != 0).all(), z1              # the one pre-activation: negative in one run, positive in the other
    assert (want < 0.1).any() and (want > 0.9).any() and ((want > 0.3) & (want < 0.7)).any()       # the yardstick's gates cover (0, 1)
    err = (got[:, :c].double() - want).abs()
    print("SE gate (ReLU) C %d pitch %d hw %d q %d batch %d: pre-activations %.0f %% < 0, %.0f %% > 0, gates %.4f .. %.4f, max err %.3e, worst err / bound %.3f"
          % (c, pitch, hw, q, batch, 100 * neg, 100 * pos, want.min().item(), want.max().item(), err.max().item(), (err / tol).max().item()))
    assert not torch.isnan(got).any() and (err <= tol).all()
    again = _se_gate_run(eng, xh, xl, w1, b1, w2, b2, hw, pitch, q)                     # the same bits on a second run
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))


def test_se_gate_relu_is_not_the_silu_gate(eng, dev):
    """Case 2 through both entries: they differ by more than 1e3 x the bound on some channel (and the SiLU gate is not inside the ReLU bound)."""
    c, pitch, hw, q, batch = 16, 32, 49, 6, 3
    x, w1, b1, w2, b2 = _se_inputs(c, pitch, hw, q, batch, seed=100 * c + hw, dev=dev)
    xh, xl = split(x)
    relu = _se_gate_run(eng, xh, xl, w1, b1, w2, b2, hw, pitch, q)
    silu = _se_gate_run(eng, xh, xl, w1, b1, w2, b2, hw, pitch, q, entry="mpx_se_gate")
    want, tol, _z1 = _se_gate_want(xh, xl, w1, b1, w2, b2, c, hw, pitch, q)
    ratio = ((relu[:, :c].double() - silu[:, :c].double()).abs() / tol).max().item()
    print("ReLU gate against SiLU gate: largest difference / bound %.3g" % ratio)
    assert ratio > 1e3
    assert ((relu[:, :c].double() - want).abs() <= tol).all() and not ((silu[:, :c].double() - want).abs() <= tol).all()
    assert (silu[:, c:].view(torch.int32) == 0).all()


@pytest.mark.parametrize("c,pitch,hw,q", [(16, 32, 49, 6), (144, 160, 196, 36)])
def test_se_gate_relu_of_an_image_has_the_same_bits_alone_and_inside_a_batch(eng, dev, c, pitch, hw, q):
    x, w1, b1, w2, b2 = _se_inputs(c, pitch, hw, q, 3, seed=31 + c, dev=dev)
    xh, xl = split(x)
    in_batch = _se_gate_run(eng, xh, xl, w1, b1, w2, b2, hw, pitch, q)
    for n in range(3):
        alone = _se_gate_run(eng, xh[n:n + 1].contiguous(), xl[n:n + 1].contiguous(), w1, b1, w2, b2, hw, pitch, q)
        assert torch.equal(alone[0].view(torch.int32), in_batch[n].view(torch.int32)), n
    assert not torch.equal(in_batch[0], in_batch[2])                                    # ... and the images are different images


def test_se_gate_relu_refuses_bad_arguments(eng, dev):
    z = torch.zeros(4096, dtype=torch.float16, device=dev)
    f = torch.zeros(4096, dtype=torch.float32, device=dev)
    a, b = ptr(z), ptr(f)
    gate = eng._lib.mpx_se_gate_relu
    assert gate(eng._h, a, a, b, b, b, b, ptr(torch.zeros(64, device=dev)), 1, 4, 8, 3, None) == 0
    torch.cuda.synchronize()
    off = C.c_void_p(f.data_ptr() + 4)
    assert gate(None, a, a, b, b, b, b, b, 1, 4, 8, 3, None) == -1
    for k in range(7):                                                                  # every pointer: null, then misaligned
        args = [a, a, b, b, b, b, b]
        args[k] = None
        assert gate(eng._h, *args, 1, 4, 8, 3, None) == -1 and b"se_gate_relu: null pointer" in eng._lib.mpx_last_error(eng._h), k
        args[k] = C.c_void_p(z.data_ptr() + 2) if k < 2 else off
        assert gate(eng._h, *args, 1, 4, 8, 3, None) == -1 and b"16-byte aligned" in eng._lib.mpx_last_error(eng._h), k
    assert gate(eng._h, a, a, b, b, b, b, b, 0, 4, 8, 3, None) == -1                     # empty batch
    assert gate(eng._h, a, a, b, b, b, b, b, 1, 0, 8, 3, None) == -1                     # empty map
    assert gate(eng._h, a, a, b, b, b, b, b, 1, 4, 12, 3, None) == -1                    # pitch % 8
    assert gate(eng._h, a, a, b, b, b, b, b, 1, 4, 0, 3, None) == -1
    assert gate(eng._h, a, a, b, b, b, b, b, 1, 4, 8, 0, None) == -1                     # q 0
    assert gate(eng._h, a, a, b, b, b, b, b, 1, 4, 8192, 3, None) == -1 and b"64 KB" in eng._lib.mpx_last_error(eng._h)     # two copies of the pitch pass 64 KB of LDS


def test_se_gate_relu_with_engine_layer_parameters(eng, dev, sds):
    """The device vectors mpx_load_se made for a padded layer of regnet_y_800mf (block2-1.f.se: 144 channels at pitch 160, q 36), and the
    gate on them."""
    sd = sds["regnet_y_800mf"]
    name = "trunk_output.block2.block2-1.f.se"
    k = [d.name.decode() for d in eng.ses].index(name)
    d = eng.ses[k]
    assert (d.channels, d.pitch, d.q, d.hw) == (144, 160, 36, 28) and eng.se_acts[k] == 1
    ptrs = [C.c_void_p() for _ in range(4)]
    assert eng._lib.mpx_se_params(eng._h, k, *[C.byref(p) for p in ptrs]) == 0
    w1, b1, w2, b2 = dev_view(ptrs[0], 36 * 160, dev).view(36, 160), dev_view(ptrs[1], 36, dev), dev_view(ptrs[2], 36 * 160, dev).view(36, 160), dev_view(ptrs[3], 160, dev)
    assert torch.equal(w1[:, :144], sd[name + ".fc1.weight"].reshape(36, 144)) and (w1[:, 144:] == 0).all()
    assert torch.equal(w2[:, :144], sd[name + ".fc2.weight"].reshape(144, 36).t()) and (w2[:, 144:] == 0).all()
    assert torch.equal(b1, sd[name + ".fc1.bias"]) and torch.equal(b2[:144], sd[name + ".fc2.bias"]) and torch.isneginf(b2[144:]).all()
    x = _se_inputs(144, 160, 784, 36, 2, seed=3, dev=dev)[0]
    xh, xl = split(x)
    args = [t.to(dev) for t in (w1, b1, w2, b2)]
    got = _se_gate_run(eng, xh, xl, *args, 784, 160, 36)
    want, tol, z1 = _se_gate_want(xh, xl, *args, 144, 784, 160, 36)
    assert (z1 < 0).any() and (z1 > 0).any()
    assert ((got[:, :144].double() - want).abs() <= tol).all() and (got[:, 144:].view(torch.int32) == 0).all()


# ------------------------------------------------------------------------------------------------
# 2. group width 56 on tile 18, behind fences, inside the per-element bound
# ------------------------------------------------------------------------------------------------
_packed = {}


def _pack(eng, d):
    """mpx_pack_gconvw_weights of case d on the host, uploaded: (w_hi, w_lo, scale, shift) device tensors, and the case's state_dict."""
    if d.name not in _packed:
        sd = yd.weights(d)
        rows, kp = d.groups * 4 * 16, 512
        w_hi, w_lo = torch.zeros(rows * kp, dtype=torch.int16), torch.zeros(rows * kp, dtype=torch.int16)
        scale, shift = torch.zeros(rows), torch.zeros(rows)
        t = [sd[d.name + ".weight"].contiguous()] + [sd[d.bn_name + "." + k].contiguous() for k in ("weight", "bias", "running_mean", "running_var")]
        rc = eng._lib.mpx_pack_gconvw_weights(d.width, d.groups, *[ptr(v) for v in t], EPS, ptr(w_hi), ptr(w_lo), ptr(scale), ptr(shift))
        assert rc == 0
        _packed[d.name] = (tuple(v.to(eng.device) for v in (w_hi, w_lo, scale, shift)), sd)
    return _packed[d.name]


def _launch_cg56(eng, d, x_hi, x_lo, batch, pad_sentinel=False):
    """mpx_gconvw3x3_bn_act of case d over `batch` images (x_*: [batch][hin][hin][width], placed into planes at the case's pitch) -> fenced
    (hi, lo) at that pitch; tile 18 and nothing else must have run.  Every pad channel of the output is +0."""
    (w_hi, w_lo, scale, shift), _sd = _pack(eng, d)
    pitch = yd.pitch(d.width)
    rows = batch * d.hout * d.hout
    xh, xl = _at_pitch(x_hi, pitch, pad_sentinel), _at_pitch(x_lo, pitch, pad_sentinel)
    hi, lo = Fenced(rows, pitch, eng.device), Fenced(rows, pitch, eng.device)
    rc = eng._lib.mpx_gconvw3x3_bn_act(eng._h, ptr(xh), ptr(xl), ptr(w_hi), ptr(w_lo), ptr(scale), ptr(shift), ptr(hi.payload), ptr(lo.payload),
                                        batch, d.hin, d.width, d.groups, pitch, pitch, d.stride, 1, eng._stream())
    _lib.check(eng._h, rc, "mpx_gconvw3x3_bn_act(%s, batch %d)" % (d.name, batch))
    mask = eng._lib.mpx_last_conv_kernels(eng._h)
    torch.cuda.synchronize()
    assert mask == 1 << yd.TILE, "%s ran kernels %#x" % (d.name, mask)
    for plane, which in ((hi, "hi"), (lo, "lo")):
        assert plane.problems() == [], "%s batch %d, %s plane: %s" % (d.name, batch, which, "; ".join(plane.problems()))
        assert (plane.payload_bits[:, d.width:] == 0).all(), "%s: a pad channel of the %s plane is not +0" % (d.name, which)
    return hi, lo


CG56 = [(d, b) for d in yd.CASES for b in yd.BATCHES]


@pytest.mark.parametrize("d,batch", CG56, ids=["%s-b%d" % (d.name, b) for d, b in CG56])
def test_cg56_behind_fences_inside_the_per_element_bound(eng, d, batch):
    x = yd.draws(d, batch, device=eng.device)
    _packed_, sd = _pack(eng, d)
    pre, want, b = (t.reshape(-1, d.width) for t in yd.reference(sd, d, x[2]))
    yd.preconditions(want)
    hi, lo = _launch_cg56(eng, d, x[0], x[1], batch)
    got = hi.payload[:, :d.width].double() + lo.payload[:, :d.width].double()
    assert not torch.isnan(got).any()
    err, tol = (got - want).abs(), yd.tol(d, b)
    ratio = (err / tol).max().item()
    worst = torch.argmax(err / tol).item()
    print("cg 56 %s groups %d width %d at pitch %d stride %d map %d batch %d (M = %d): worst err / tol %.3f (pixel row %d, channel %d), C %g"
          % (d.name, d.groups, d.width, yd.pitch(d.width), d.stride, d.hin, batch, got.shape[0], ratio, worst // d.width, worst % d.width, yd.C_TOL[d.name]))
    assert ratio <= 1.0, "%d elements over their bound, worst err / tol %.3f at pixel row %d, channel %d" % (
        int((err > tol).sum()), ratio, worst // d.width, worst % d.width)
    neg = pre < -tol
    assert neg.any() and (hi.payload_bits[:, :d.width][neg] == 0).all() and (lo.payload_bits[:, :d.width][neg] == 0).all(), \
        "a clearly negative pre-activation is not +0 in both planes"


@pytest.mark.parametrize("name", [d.name for d in yd.CASES])
def test_cg56_image_has_the_same_bits_alone_and_at_index_2_of_a_batch_of_3(eng, name):
    d = yd.case(name)
    x_hi, x_lo, _x = yd.draws(d, 3, device=eng.device)
    a_hi, a_lo = _launch_cg56(eng, d, x_hi[:1].contiguous(), x_lo[:1].contiguous(), 1)
    order = [1, 2, 0]
    b_hi, b_lo = _launch_cg56(eng, d, x_hi[order].contiguous(), x_lo[order].contiguous(), 3)
    n = d.hout * d.hout
    assert torch.equal(a_hi.payload_bits, b_hi.payload_bits[2 * n:]) and torch.equal(a_lo.payload_bits, b_lo.payload_bits[2 * n:])


@pytest.mark.parametrize("name", ["g1", "g3"])
def test_cg56_input_pad_channels_are_never_read(eng, name):
    """Width 56 at pitch 64, 168 at 192: input pad channels filled with the NaN sentinel change no output bit."""
    d = yd.case(name)
    assert yd.pitch(d.width) - d.width in (8, 24)
    x_hi, x_lo, _x = yd.draws(d, 2, device=eng.device)
    a_hi, a_lo = _launch_cg56(eng, d, x_hi, x_lo, 2)
    b_hi, b_lo = _launch_cg56(eng, d, x_hi, x_lo, 2, pad_sentinel=True)
    assert torch.equal(a_hi.payload_bits, b_hi.payload_bits) and torch.equal(a_lo.payload_bits, b_lo.payload_bits)


def test_the_stand_alone_grouped_entry_gives_an_engine_layers_bits(engines, sds):
    """regnet_y_8gf's block4-0.f.b (36 groups of 56, 14 -> 7) through mpx_conv_bn_act and, with weights packed by mpx_pack_gconvw_weights from the
    same state_dict, through mpx_gconvw3x3_bn_act: the same planes bit for bit."""
    eng, sd = engines["regnet_y_8gf"], sds["regnet_y_8gf"]
    name, bn = "trunk_output.block4.block4-0.f.b.0", "trunk_output.block4.block4-0.f.b.1"
    i = layer_index(eng, name)
    e = eng.layers[i]
    assert (e.cin, e.stride, e.hin, eng.groups[i]) == (2016, 2, 14, 36) and _pitches(eng, i) == (2016, 2016)
    d = yd.GDesc("regnet_y_8gf", name, bn, 2016, 56, 36, 2, 14, 7)
    x_hi, x_lo, _x = yd.xgd.draws(d, 3, seed=77, device=eng.device)
    a_hi, a_lo = _sentinel((3 * 49, 2016), eng.device), _sentinel((3 * 49, 2016), eng.device)
    _lib.check(eng._h, eng._lib.mpx_conv_bn_act(eng._h, i, ptr(x_hi), ptr(x_lo), None, None, ptr(a_hi), ptr(a_lo), None, 3, eng._stream()), "mpx_conv_bn_act")
    assert eng._lib.mpx_last_conv_kernels(eng._h) == 1 << 18
    rows = 36 * 64
    w_hi, w_lo = torch.zeros(rows * 512, dtype=torch.int16), torch.zeros(rows * 512, dtype=torch.int16)
    scale, shift = torch.zeros(rows), torch.zeros(rows)
    t = [sd[name + ".weight"].contiguous()] + [sd[bn + "." + k].contiguous() for k in ("weight", "bias", "running_mean", "running_var")]
    assert eng._lib.mpx_pack_gconvw_weights(2016, 36, *[ptr(v) for v in t], EPS, ptr(w_hi), ptr(w_lo), ptr(scale), ptr(shift)) == 0
    dv = [v.to(eng.device) for v in (w_hi, w_lo, scale, shift)]
    b_hi, b_lo = _sentinel((3 * 49, 2016), eng.device), _sentinel((3 * 49, 2016), eng.device)
    rc = eng._lib.mpx_gconvw3x3_bn_act(eng._h, ptr(x_hi), ptr(x_lo), *[ptr(v) for v in dv], ptr(b_hi), ptr(b_lo), 3, 14, 2016, 36, 2016, 2016, 2, 1, eng._stream())
    _lib.check(eng._h, rc, "mpx_gconvw3x3_bn_act")
    torch.cuda.synchronize()
    assert not torch.isnan(a_hi).any() and (a_hi != 0).any()
    assert torch.equal(a_hi.view(torch.int16), b_hi.view(torch.int16)) and torch.equal(a_lo.view(torch.int16), b_lo.view(torch.int16))


def test_the_stand_alone_grouped_entry_refuses_bad_arguments(eng, dev):
    z = torch.zeros(1 << 16, dtype=torch.float16, device=dev)
    f = torch.zeros(4096, dtype=torch.float32, device=dev)
    a, b = ptr(z), ptr(f)
    run = eng._lib.mpx_gconvw3x3_bn_act
    ok = dict(B=1, hin=3, width=56, groups=1, pin=64, pout=64, stride=1)

    def call(ptrs=None, **kw):
        v = dict(ok, **kw)
        ptrs = ptrs or [a, a, a, a, b, b, a, a]
        return run(eng._h, *ptrs, v["B"], v["hin"], v["width"], v["groups"], v["pin"], v["pout"], v["stride"], 1, None)

    assert call() == 0
    torch.cuda.synchronize()
    for k in range(8):
        ptrs = [a, a, a, a, b, b, a, a]
        ptrs[k] = None
        assert call(ptrs) == -1 and b"null pointer" in eng._lib.mpx_last_error(eng._h), k
        ptrs[k] = C.c_void_p(z.data_ptr() + 8)
        assert call(ptrs) == -1 and b"16-byte aligned" in eng._lib.mpx_last_error(eng._h), k
    for bad in (dict(B=0), dict(hin=0), dict(stride=3), dict(stride=0), dict(groups=0), dict(width=60), dict(width=64, groups=2), dict(width=56, groups=7),
                dict(pin=48), dict(pin=60), dict(pout=48), dict(pout=60)):
        assert call(**bad) == -1, bad
    pack = eng._lib.mpx_pack_gconvw_weights
    w = torch.zeros(56 * 56 * 9)
    h16, f32 = torch.zeros(64 * 512, dtype=torch.int16), torch.zeros(64)
    v = torch.ones(56)
    assert pack(56, 1, ptr(w), ptr(v), ptr(v), ptr(v), ptr(v), EPS, ptr(h16), ptr(h16.clone()), ptr(f32), ptr(f32.clone())) == 0
    assert pack(56, 7, ptr(w), ptr(v), ptr(v), ptr(v), ptr(v), EPS, ptr(h16), ptr(h16), ptr(f32), ptr(f32)) == -1        # 8 channels per group
    assert pack(56, 1, None, ptr(v), ptr(v), ptr(v), ptr(v), EPS, ptr(h16), ptr(h16), ptr(f32), ptr(f32)) == -1
    assert pack(56, 1, ptr(w), None, ptr(v), ptr(v), ptr(v), EPS, ptr(h16), ptr(h16), ptr(f32), ptr(f32)) == -1


# ------------------------------------------------------------------------------------------------
# 3. descriptors, groups, tiles, SE lists, refusals, workspace
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ARCHS)
def test_descriptors_groups_tiles_se_layers_and_refusals(engines, arch):
    eng = engines[arch]
    lib, h = eng._lib, eng._h
    topo = ref.topology(arch)
    assert len(eng.layers) == len(topo) == lib.mpx_num_convs(h) == ref.TABLE[arch][6]
    n_grouped, on_16 = 0, []
    for i, (d, t) in enumerate(zip(eng.layers, topo)):
        name, bn, cin, cout, k, stride, pad, hin, hout, relu, res, groups = t
        assert (d.name.decode(), d.bn_name.decode(), d.cin, d.cout, d.ksize, d.stride, d.pad, d.hin, d.hout, d.relu, d.residual) == t[:11], name
        g = C.c_int()
        assert lib.mpx_conv_groups(h, i, C.byref(g)) == 0 and g.value == groups == eng.groups[i], name
        pin, pout = _pitches(eng, i)
        assert pin == (4 if cin == 3 else ref.pitch(cin)) and pout == (cout if name == "fc" else ref.pitch(cout)), name
        tile = lib.mpx_get_conv_tile(h, i)
        if groups > 1:
            n_grouped += 1
            cg = cin // groups
            assert d.k_packed == (9 * cg + 31) // 32 * 32 and d.cout_pad == groups * ((cg + 15) // 16) * 16 and tile == 18, name
            for other in DENSE_TILES:            # a grouped layer accepts no dense tile ...
                assert lib.mpx_set_conv_tile(h, i, other) == -1 and b"grouped" in lib.mpx_last_error(h), (name, other)
            ok16 = cg == 16 and cin % 64 == 0      # ... and tile 16 where the shape is one of that kernel's: refused where it was refused before
            assert lib.mpx_set_conv_tile(h, i, 16) == (0 if ok16 else -1), name
            if ok16:
                on_16.append(cin)
            else:
                assert b"grouped" in lib.mpx_last_error(h)
            assert lib.mpx_set_conv_tile(h, i, 18) == 0 and lib.mpx_set_conv_tile(h, i, -1) == 0 and lib.mpx_get_conv_tile(h, i) == 18
        else:
            assert d.k_packed == (96 if cin == 3 else k * k * ref.pitch(cin)) and d.cout_pad == -(-cout // 128) * 128, name
            for t_ in (16, 18):                  # ... and neither grouped kernel a dense layer
                assert lib.mpx_set_conv_tile(h, i, t_) == -1 and b"grouped" in lib.mpx_last_error(h), (name, t_)
            assert lib.mpx_get_conv_tile(h, i) == tile and tile in GENERIC, (name, tile)
        for unknown in (15, 17):
            assert lib.mpx_set_conv_tile(h, i, unknown) == -1 and b"product ids" in lib.mpx_last_error(h)
    assert n_grouped == sum(ref.TABLE[arch][2])          # every f.b of these networks is grouped
    assert sorted(set(on_16)) == {"regnet_y_800mf": [64, 320]}.get(arch, [])
    # the SE list
    ses = ref.se_layers(arch)
    assert lib.mpx_num_se(h) == len(eng.ses) == len(ses) == ref.TABLE[arch][7]
    for k, (e, want) in enumerate(zip(eng.ses, ses)):
        assert (e.name.decode(), e.channels, e.pitch, e.q, e.hw) == want, want[0]
        a = C.c_int(-1)
        assert lib.mpx_se_act(h, k, C.byref(a)) == 0 and a.value == 1 == eng.se_acts[k]
    assert lib.mpx_se_act(h, len(ses), C.byref(C.c_int())) == -1 and lib.mpx_se_act(h, -1, C.byref(C.c_int())) == -1 and lib.mpx_se_act(h, 0, None) == -1
    assert lib.mpx_num_bottleneck_tails(h) == 0 and lib.mpx_num_pointwise_tails(h) == 0 and lib.mpx_num_dwconvs(h) == 0
    assert abs(eng.flops_per_forward - 2.0 * ref.macs(arch)) <= 1e-9 * eng.flops_per_forward
    assert not eng.has_stem_table and eng.stem == "conv"
    lab = torch.zeros(224, 224, dtype=torch.int32, device=eng.device)
    assert lib.mpx_stem_table_build(h, None, None, ptr(lab), 1, None, None, None) == -2 and b"RegNetY" in lib.mpx_last_error(h)
    out = torch.zeros(8, dtype=torch.float16, device=eng.device)
    assert lib.mpx_stem_conv_maxpool(h, ptr(out), ptr(out), 1, None) == -2 and b"7x7 stem" in lib.mpx_last_error(h)


def test_set_conv_tile_18_on_an_8gf_layer_and_where_it_was_refused_before(engines, dev):
    eng = engines["regnet_y_8gf"]
    i = layer_index(eng, "trunk_output.block3.block3-1.f.b.0")
    assert eng.groups[i] == 16 and eng.layers[i].cin // 16 == 56
    assert eng._lib.mpx_set_conv_tile(eng._h, i, 18) == 0 and eng._lib.mpx_get_conv_tile(eng._h, i) == 18
    assert eng._lib.mpx_set_conv_tile(eng._h, i, 16) == -1 and eng._lib.mpx_set_conv_tile(eng._h, i, 2) == -1
    assert eng._lib.mpx_set_conv_tile(eng._h, layer_index(eng, "trunk_output.block3.block3-1.f.a.0"), 18) == -1
    for arch, grouped in (("resnet18", None), ("resnext50_32x4d", "layer1.0.conv2"), ("efficientnet_b0", None)):
        other = MaskedForwardEngine(arch, max_batch=2, device=0)
        try:
            assert other._lib.mpx_set_conv_tile(other._h, 1, 18) == -1 and b"grouped" in other._lib.mpx_last_error(other._h)
            if grouped:
                j = layer_index(other, grouped)
                assert other._lib.mpx_set_conv_tile(other._h, j, 18) == -1 and other._lib.mpx_get_conv_tile(other._h, j) == 16
            if arch == "efficientnet_b0":       # every SE layer of an EfficientNet engine keeps SiLU
                assert len(other.ses) == 16 and other.se_acts == [0] * 16
        finally:
            other.close()


def test_unknown_ids_in_the_regnet_y_range_are_refused(dev):
    lib = _lib.load()
    known = {ref.TABLE[a][0] for a in ARCHS}
    for arch_id in (15000, 15004, 15009, 15160, 15320, 15999):
        assert arch_id not in known
        h = C.c_void_p()
        assert lib.mpx_create(arch_id, 2, 0, C.byref(h)) == -1 and not h.value
    for arch_id in sorted(known):
        h = C.c_void_p()
        assert lib.mpx_create(arch_id, 2, 0, C.byref(h)) == 0 and h.value
        assert lib.mpx_destroy(h) == 0


@pytest.mark.parametrize("arch", ARCHS)
def test_default_max_batch_and_bytes_per_slot(dev, arch):
    """Default max_batch 512 (RegNetX's rule).  Bytes per slot from the plan: the padded NHWC4 staging, four activation buffers of the largest
    map at its pitch, the pooled planes, the logits -- two split-fp16 planes each -- and ONE gate row of the widest stage's pitch in fp32."""
    act = max(c[8] * c[8] * ref.pitch(c[3]) for c in ref.topology(arch)[:-1])
    feat = ref.TABLE[arch][1][3]
    want = 2 * 2 * 230 * 230 * 4 + 4 * 2 * 2 * act + 2 * 2 * ref.pitch(feat) + 4 * 1000 + 4 * ref.pitch(feat)
    small = MaskedForwardEngine(arch, max_batch=8, device=0)
    big = MaskedForwardEngine(arch, max_batch=72, device=0)
    try:
        per_slot = (big.workspace_bytes - small.workspace_bytes) / 64
        print("%s: %.3f MB per slot (plan: %.3f MB)" % (arch, per_slot / 1e6, want / 1e6))
        assert abs(per_slot - want) <= 64
    finally:
        small.close()
        big.close()
    if arch == ARCHS[0]:
        e = MaskedForwardEngine(arch, device=0)
        try:
            assert e.max_batch == 512
        finally:
            e.close()


# ------------------------------------------------------------------------------------------------
# 4. every distinct conv shape of the four networks on every tile that accepts it
# ------------------------------------------------------------------------------------------------
def _bn(sd, bn, dev):
    s = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + EPS)
    return s.to(dev), (sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * s).to(dev)


def _layer_want(sd, d, groups, x64, res64):
    """fp64 conv (dense or grouped) + BatchNorm or bias (+ residual) (+ ReLU), one matrix product per tap and group:
    [B][hout][hout][cout] on the device."""
    name, bn = d.name.decode(), d.bn_name.decode()
    dev = x64.device
    cg = d.cin // groups
    w = sd[name + ".weight"].double().reshape(groups, d.cout // groups, cg, d.ksize, d.ksize).to(dev)
    xc = F.pad(x64, (0, 0, d.pad, d.pad, d.pad, d.pad)) if d.pad else x64
    s, ho = d.stride, d.hout
    acc = None
    for ky in range(d.ksize):
        for kx in range(d.ksize):
            tap = xc[:, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (ho - 1) + 1:s, :].reshape(-1, groups, cg).transpose(0, 1)
            y = torch.bmm(tap, w[:, :, :, ky, kx].transpose(1, 2))
            acc = y if acc is None else acc + y
    acc = acc.transpose(0, 1).reshape(-1, d.cout)
    if bn:
        sc, sh = _bn(sd, bn, dev)
        acc = acc * sc + sh
    else:
        acc = acc + sd[name + ".bias"].double().to(dev)
    acc = acc.view(x64.shape[0], ho, ho, d.cout)
    if res64 is not None:
        acc = acc + res64
    return torch.relu(acc) if d.relu else acc


def _run_layer(eng, sd, i, batch):
    """Layer i on its current tile, on planes at its pitches (pad channels of the input and the residual +0) -> (got, want, kernels)."""
    d, dev = eng.layers[i], eng.device
    pin, pout = _pitches(eng, i)
    fc = d.name.decode() == "fc"
    g = torch.Generator(device=dev).manual_seed(1000 * i + batch)
    xh, xl = split(torch.randn(batch, d.hin, d.hin, d.cin, generator=g, device=dev).clamp_min(-0.5) * 1.5)
    rh = rl = None
    if d.residual:
        rh, rl = split(torch.randn(batch, d.hout, d.hout, d.cout, generator=g, device=dev))
    if i == 0:      # the stem reads the engine's padded NHWC4 staging: write the interior, zero border and 4th channel
        stage_stem_input(eng, xh, xl, batch)
        in_h = in_l = None
    else:
        in_h, in_l = _at_pitch(xh, pin), _at_pitch(xl, pin)
    res_h, res_l = (_at_pitch(rh, pout), _at_pitch(rl, pout)) if d.residual else (None, None)
    want = _layer_want(sd, d, eng.groups[i], merge(xh, xl).double(), merge(rh, rl).double() if d.residual else None)
    if fc:          # the fc writes fp32 logits
        out = torch.full((batch + 1, 1000), float("nan"), dtype=torch.float32, device=dev)
        rc = eng._lib.mpx_conv_bn_act(eng._h, i, ptr(in_h), ptr(in_l), None, None, None, None, ptr(out), batch, eng._stream())
        _lib.check(eng._h, rc, "mpx_conv_bn_act(fc)")
        ran = eng._lib.mpx_last_conv_kernels(eng._h)
        torch.cuda.synchronize()
        assert torch.isnan(out[batch]).all()
        return out[:batch].double().view(batch, 1, 1, 1000), want, ran
    oh, ol = _sentinel((batch + 1, d.hout, d.hout, pout), dev), _sentinel((batch + 1, d.hout, d.hout, pout), dev)
    rc = eng._lib.mpx_conv_bn_act(eng._h, i, ptr(in_h), ptr(in_l), ptr(res_h), ptr(res_l), ptr(oh), ptr(ol), None, batch, eng._stream())
    _lib.check(eng._h, rc, "mpx_conv_bn_act")
    ran = eng._lib.mpx_last_conv_kernels(eng._h)
    torch.cuda.synchronize()
    assert torch.isnan(oh[batch]).all() and torch.isnan(ol[batch]).all(), "%s wrote past its last pixel" % d.name.decode()
    assert (oh[:batch, ..., d.cout:].view(torch.int16) == 0).all() and (ol[:batch, ..., d.cout:].view(torch.int16) == 0).all(), "pad channels are not +0"
    return merge(oh[:batch, ..., :d.cout], ol[:batch, ..., :d.cout]).double(), want, ran


def _distinct_shapes():
    """(arch, name) of the first layer of every distinct (cin, cout, ksize, stride, input map, residual, groups) of the four networks.  A shape
    two of the networks share is kept in both: their descriptors differ in the name, and the weights differ."""
    out = []
    for arch in ARCHS:
        seen = set()
        for c in ref.topology(arch):
            key = (c[2], c[3], c[4], c[5], c[7], c[10], c[11])
            if key not in seen:
                seen.add(key)
                out.append((arch, c[0]))
    return out


SHAPES = _distinct_shapes()


@pytest.mark.parametrize("arch,name", SHAPES, ids=["%s-%s" % s for s in SHAPES])
def test_conv_shape_on_its_default_tile_and_on_every_tile_that_accepts_it(engines, sds, arch, name):
    eng, sd = engines[arch], sds[arch]
    i = layer_index(eng, name)
    d = eng.layers[i]
    default = eng._lib.mpx_get_conv_tile(eng._h, i)
    accepted = [t for t in DENSE_TILES + (16, 18) if eng._lib.mpx_set_conv_tile(eng._h, i, t) == 0]
    if eng.groups[i] > 1:
        assert default == 18 and set(accepted) <= {16, 18}
    else:
        assert default in accepted and GENERIC <= set(accepted)
    batch = 1 if d.hin >= 112 else 3
    kdim = d.cin // eng.groups[i] * d.ksize * d.ksize
    try:
        for tile in accepted:
            assert eng._lib.mpx_set_conv_tile(eng._h, i, tile) == 0
            got, want, ran = _run_layer(eng, sd, i, batch)
            assert not torch.isnan(got).any(), (name, tile)
            err, scale = (got - want).abs().max().item(), want.abs().max().item()
            bound = layer_bound(d, scale, k=kdim)
            print("%s %s %d->%d k%d s%d h%d res %d groups %d tile %d%s batch %d: max err %.3e (scale %.2f, bound %.3e), kernels 0x%x"
                  % (arch, name, d.cin, d.cout, d.ksize, d.stride, d.hin, d.residual, eng.groups[i], tile, " (default)" if tile == default else "", batch, err, scale, bound, ran))
            assert err <= bound, "%s tile %d: max err %.3e (scale %.2f, bound %.3e)" % (name, tile, err, scale, bound)
            if eng.groups[i] > 1:
                assert ran == 1 << tile
    finally:
        assert eng._lib.mpx_set_conv_tile(eng._h, i, -1) == 0 and eng._lib.mpx_get_conv_tile(eng._h, i) == default


# ------------------------------------------------------------------------------------------------
# 5. end to end
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ARCHS)
def test_regnet_y_end_to_end(engines, sds, golden_dir, arch):
    """800MF / 1.6GF / 3.2GF: 4 felzenszwalb + 2 grid rows; 8GF: 3 felzenszwalb rows.  Scores by the MobileNetV2 rule (d = max |fp32 CPU loop -
    fp64|: bound 2e-5 when 4 d < 2e-5, else 4 d rounded up to one digit, never above 1e-4), all logits through the logits lens (4 d_L), every
    argmax equal."""
    rows = [(kind,) + row for kind, row in ref.e2e_rows(golden_dir, arch).items()]
    check_end_to_end(engines[arch], arch, Reference(ref, sds[arch], arch), rows,
                     "%(arch)s: yardstick distance %(d).3e over %(n)d rows -> end-to-end bound %(bound).1e", segments=False, peaks=True)


@pytest.mark.parametrize("arch", ("regnet_y_800mf", "regnet_y_8gf"))
def test_a_mask_row_scores_the_same_bits_wherever_it_sits(engines, golden_dir, arch):
    check_position_independence(engines[arch], *ref.e2e_inputs(golden_dir, "felz"), (3, ((1, 0, (0,)), (8, 41, (0, 5, 7)), (13, 44, (3, 8, 12)))))


def test_api_on_a_regnet_y_engine(engines, sds, golden_dir):
    arch = "regnet_y_800mf"
    check_api(engines[arch], Reference(ref, sds[arch], arch), *ref.e2e_inputs(golden_dir, "grid"),
              rows=4, same_pred=True, heatmaps=0, predict=False, table_step=49)


@pytest.mark.parametrize("arch", ("regnet_y_800mf", "regnet_y_8gf"))
def test_profile_lists_one_gate_and_one_scale_row_per_block(engines, dev, arch):
    eng = engines[arch]
    img = torch.from_numpy(synth.make_images(1, kind="noise")[0]).to(dev)
    seg = torch.from_numpy(synth.grid_segments()).to(dev)
    onoff = torch.from_numpy(synth.random_onoff(4, 196)).to(dev)
    labels = torch.zeros(4, dtype=torch.int32, device=dev)
    eng.profile(True)
    eng.stage_masks(img, seg, onoff, 0)
    eng.forward(4, labels)
    eng.profile(False)
    prof = eng.collect_profile()
    n_blocks = sum(ref.TABLE[arch][2])
    assert len(prof["per_conv_ms"]) == len(eng.layers) and all(ms > 0 for ms in prof["per_conv_ms"])      # no conv rides in another's launch
    assert len(prof["per_se_gate_ms"]) == len(prof["per_se_scale_ms"]) == n_blocks == len(eng.ses)
    assert all(ms > 0 for ms in prof["per_se_gate_ms"]) and all(ms > 0 for ms in prof["per_se_scale_ms"])
    assert prof["launches"]["conv"] == len(eng.layers) and prof["launches"]["head"] == 1
    assert prof["launches"]["pool"] == 2 * n_blocks + 1                     # gate and scale of every block, the global average pool


def test_regnet_y_error_paths(dev, sds):
    arch = "regnet_y_800mf"
    with pytest.raises(ValueError, match="no 7x7 stem"):
        MaskedForwardEngine(arch, max_batch=2, device=0, stem="table")
    sd = sds[arch]
    eng = MaskedForwardEngine(arch, max_batch=2, device=0)
    try:
        lib, h = eng._lib, eng._h
        assert lib.mpx_weights_complete(h) == 0
        se_names = [d.name.decode() for d in eng.ses]
        eng.load_state_dict(sd, only=[d.name.decode() for d in eng.layers])           # every conv, no SE layer
        assert lib.mpx_weights_complete(h) == 0
        img = torch.from_numpy(synth.make_images(1, kind="noise")[0]).to(dev)
        seg = torch.from_numpy(synth.grid_segments()).to(dev)
        onoff = torch.from_numpy(synth.random_onoff(2, 196)).to(dev)
        eng.stage_masks(img, seg, onoff, 0)
        labels = torch.zeros(2, dtype=torch.int32, device=dev)
        score = torch.zeros(2, dtype=torch.float32, device=dev)
        pred = torch.zeros(2, dtype=torch.int32, device=dev)
        assert lib.mpx_forward(h, ptr(labels), ptr(score), ptr(pred), None, 2, eng._stream()) == -2 and b"weights not loaded" in lib.mpx_last_error(h)
        eng.load_state_dict(sd, only=se_names[:-1])
        assert lib.mpx_weights_complete(h) == 0 and lib.mpx_forward(h, ptr(labels), ptr(score), ptr(pred), None, 2, eng._stream()) == -2
        eng.load_state_dict(sd, only=se_names[-1:])
        assert lib.mpx_weights_complete(h) == 1
        assert lib.mpx_forward(h, ptr(labels), ptr(score), ptr(pred), None, 2, eng._stream()) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(score).all() and (score > 0).all()
        bad = dict(sd)
        bad[se_names[0] + ".fc1.weight"] = torch.zeros(9, 64, 1, 1)
        with pytest.raises(ValueError, match="expected"):
            eng.load_state_dict(bad, only=se_names[:1])
        assert lib.mpx_load_se(h, 0, None, None, None, None) == -1 and lib.mpx_load_se(h, len(se_names), None, None, None, None) == -1
    finally:
        eng.close()
