"""EfficientNet-B0 on the MI355X (pytest -m gpu), through the C-ABI as tests/test_gpu_mobilenet.py does: the topology, the depthwise k x k +
BN kernel with SiLU on either side, the SE gate and scale kernels and the SiLU global pool against fp64 with bounds derived from their
roundings, every distinct conv shape on every tile it accepts against an fp64 conv + BatchNorm of the same split inputs, the whole network
against the batch-1 fp32 CPU loop and the fp64 restatement (tests/efficientnet_ref.py), position independence of a mask row, the
reference-named API, the profile and the error paths.

Bounds.  u = 2^-24 is one fp32 rounding relative to the rounded value; the re-split into (hi, lo) is 2^-22 = 4 u relative, with half of
lo's fp16 subnormal step, 2^-25 <= 2^-24, as the absolute floor.  silu(x) = x / (1 + expf(-x)) with expf within 1 ulp is within 4 u of the exact
value (expf 2 u, the add 1 u, the division 1 u), and so is sigmoid; |silu'| <= 1.1, |sigmoid'| <= 0.25, |silu(v)| <= |v|.
  Depthwise, per element, with M = |s| sum|w_i a_i| + |t| over the taps inside the map (a_i = the exact silu(x_i) or x_i): the loaded a_i
  carry 4 u each (4 u sum|w a|), the fma chain one rounding per tap (at most 25 u sum|w a|), the BatchNorm two more (2 u M): the
  pre-activation v is within 31 u M.  The output SiLU turns that into at most 1.1 x 31 u M + 4 u |silu(v)| <= 38.1 u M, the re-split adds 4 u:
  42.1 u M < 64 u M.  Bound: 2^-18 M + 2^-24, for all four (act_in, act_out) combinations.
  SE gate, per channel, propagated in fp64 from the test's own inputs:
      d_pool[c] = hw u mean|x_c|                        any summation tree over hw values makes at most hw - 1 adds on a path, then the division
      d_z1[j]   = sum_c |w1[j][c]| d_pool[c] + (ceil(pitch / 64) + 7) u (sum_c |w1[j][c] pooled[c]| + |b1[j]|)       lane chain, 6 folds, bias
      d_s1[j]   = 1.1 d_z1[j] + 4 u |s1[j]|
      d_z2[c]   = sum_j |w2[j][c]| d_s1[j] + (q + 1) u (sum_j |w2[j][c] s1[j]| + |b2[c]|)
      d_gate[c] = 0.25 d_z2[c] + 4 u gate[c]
  SE scale, per element, against the exact product p of hi + lo and the fp32 gate: (2^-24 + 2^-22) |p| + 2^-24.
  SiLU pool, per element: ((hw + 4) 2^-24 + 2^-22) mean|silu(x_i)| + 2^-24 -- 4 u per SiLU, at most hw roundings of the sum and the division,
  the re-split.
  Per conv layer: 4e-6 sqrt(max(K, 4608) / 4608) of max(|want|, 1), the project's per-layer bound (every K here is <= 1280: 4e-6).
  End to end: the MobileNetV2 rule.  With d = max |fp32 batch-1 CPU loop - fp64| over the 28 rows, the bound on |engine - fp64| and |engine -
  fp32 loop| is the project's 2e-5 when 4 d < 2e-5, else 4 d rounded up to one digit and never above 1e-4.  The same argmax on EVERY row
  (tests/test_efficientnet_cpu.py asserts a top-two fp64 margin >= 1e-3 on exactly these rows).

d, the fp32 batch-1 CPU loop against fp64 (rows of efficientnet_ref.E2E_CASES: 20 felzenszwalb + 8 grid masks), felzenszwalb / grid:
1.4e-06 / 2.2e-07; 4 x 1.4e-06 < 2e-05: the bound is 2e-05.  Measured on one MI355X, max |d| of a score: engine vs fp64 1.5e-06 / 1.2e-07,
engine vs fp32 CPU loop 1.5e-06 / 2.1e-07.  The test prints every figure on every run."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import efficientnet_ref as ref
from gpu_common import accepted_tiles, dev, dev_view, FALLBACK, GENERIC, merge, pitch_of, ptr, split  # noqa: F401  (dev is a fixture)
from net_harness import check_api, check_conv_layer, check_end_to_end, check_position_independence, e2e_rows, Reference
from network_interpretation_imagenet_amd import _lib, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine
from oracle import scorer

pytestmark = pytest.mark.gpu

ARCH = "efficientnet_b0"
EPS = 1e-5
U = 2.0 ** -24


def silu64(x):
    return x / (1.0 + torch.exp(-x))


@pytest.fixture(scope="module")
def sd():
    return synth.make_state_dict(ARCH)


@pytest.fixture(scope="module")
def small_engine(mpx_lib, dev, sd):
    """A small workspace, for everything that hands the kernels device pointers of its own."""
    e = MaskedForwardEngine(ARCH, max_batch=8, device=0).load_state_dict(sd)
    yield e
    e.close()


@pytest.fixture(scope="module")
def engine(mpx_lib, dev, sd):
    e = MaskedForwardEngine(ARCH, device=0).load_state_dict(sd)            # the default max_batch
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------
# topology
# ------------------------------------------------------------------------------------------------
def _expected_default_tile(d):
    """The unchanged default_tile rules, spelled out for the EfficientNet-B0 shapes."""
    if d.cout <= 64:
        return 1 if d.ksize >= 3 else 4             # the stem; the project convs onto 16 .. 40 channels
    if d.cout % 256 == 0 and d.cin % 64 == 0 and d.cin >= 128 and d.cout > d.cin:
        return 10                                   # features.8: 320 -> 1280
    if d.cout > d.cin:
        return 7                                    # every expand conv, and the widening project convs
    return 2                                        # the narrowing project convs with cout > 64, the classifier


def test_efficientnet_topology_and_default_tiles(small_engine):
    eng = small_engine
    convs, dws, ses = ref.topology()
    assert len(convs) == 34 and len(dws) == 16 and len(ses) == 16
    acts = []
    for i in range(len(eng.layers)):
        a = C.c_int(-1)
        assert eng._lib.mpx_conv_consumer_act(eng._h, i, C.byref(a)) == 0
        acts.append(a.value)
    got = [(d.name.decode(), d.bn_name.decode(), d.cin, d.cout, d.ksize, d.stride, d.pad, d.hin, d.hout, d.relu, d.residual, a) for d, a in zip(eng.layers, acts)]
    assert got == convs
    assert sum(acts) == 1 + 15 + 1                              # the stem, the 15 expand convs, features.8
    for d in eng.layers:
        assert d.cout_pad == -(-d.cout // 128) * 128
        assert d.k_packed == (96 if d.cin == 3 else pitch_of(d.cin))
    shapes = []
    for k, d in enumerate(eng.dwconvs):
        v = C.c_int(), C.c_int(), C.c_int()
        assert eng._lib.mpx_dwconv_shape(eng._h, k, *[C.byref(x) for x in v]) == 0
        assert (v[1].value, v[2].value) == (1, 1) and d.clamp_in == 0 and d.pitch == pitch_of(d.channels)
        shapes.append((d.name.decode(), d.bn_name.decode(), d.channels, v[0].value, d.stride, d.hin))
    assert shapes == dws and eng.dw_ksizes == [s[3] for s in dws]
    assert [(d.name.decode(), d.channels, d.q, d.hw) for d in eng.ses] == ses and all(d.pitch == pitch_of(d.channels) for d in eng.ses)
    assert sorted({(d.channels, d.pitch) for d in eng.dwconvs if d.channels != d.pitch}) == [(144, 160), (240, 256)]
    assert eng.flops_per_forward == 2.0 * ref.MACS
    geo = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert eng._lib.mpx_geometry(eng._h, *[C.byref(v) for v in geo]) == 0 and [v.value for v in geo] == [224, 3, 1000, 1000]
    for i, d in enumerate(eng.layers):
        t = eng._lib.mpx_get_conv_tile(eng._h, i)
        assert t == _expected_default_tile(d), (d.name, t)
    assert eng.stem == "conv" and not eng.has_stem_table and eng._lib.mpx_weights_complete(eng._h) == 1
    assert eng._lib.mpx_num_bottleneck_tails(eng._h) == 0 and eng._lib.mpx_num_norms(eng._h) == 0 and eng._lib.mpx_num_shuffles(eng._h) == 0


def test_efficientnet_default_max_batch_and_workspace(engine):
    eng = engine
    assert eng.max_batch == 512
    # per slot: three 112x112x96 split-fp16 buffers, the NHWC4 staging and 1152 fp32 gates: 15.3 MB
    per_slot = 3 * 2 * 112 * 112 * 96 * 2 + 2 * 230 * 230 * 4 * 2 + 1152 * 4
    w = sum(2 * d.cout_pad * d.k_packed * 2 for d in eng.layers)
    assert per_slot * 512 + w < eng.workspace_bytes < per_slot * 512 + w + (16 << 20)
    print("efficientnet_b0: %.2f MB per slot, workspace %.2f GB at max_batch 512" % (per_slot / 1e6, eng.workspace_bytes / 1e9))


# ------------------------------------------------------------------------------------------------
# depthwise k x k + BN with SiLU on either side
# ------------------------------------------------------------------------------------------------
def _dw_inputs(c, pitch, hin, k, batch, seed, dev):
    """Planes with exact zeros, values beyond +-10 and a channel band scaled by 1e-3 (lo in fp16's subnormals); weights [c][k][k]; BatchNorm
    with both signs of gamma.  The pitch's padding channels are exact zeros on the input side, as the engine produces them."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, hin, hin, pitch, generator=g) * 3.0
    x[torch.rand(x.shape, generator=g) < 0.15] = 0.0
    x[torch.rand(x.shape, generator=g) < 0.10] *= 4.0                     # beyond +-10
    x[..., : max(1, c // 4)] *= 1e-3                                       # lo in fp16's subnormals
    x[..., c:] = 0.0
    w = torch.randn(c, k, k, generator=g) * (2.0 / (k * k)) ** 0.5
    gamma = torch.empty(c).uniform_(0.5, 2.5, generator=g) * torch.where(torch.rand(c, generator=g) < 0.3, -1.0, 1.0)
    gamma[0] = -abs(gamma[0])                                              # at least one negative BatchNorm scale
    beta = torch.randn(c, generator=g) * 0.5
    mean = torch.randn(c, generator=g) * 0.3
    var = torch.empty(c).uniform_(0.3, 2.0, generator=g)
    s64 = gamma.double() / torch.sqrt(var.double() + EPS)
    t64 = beta.double() - mean.double() * s64
    wt = torch.zeros(k * k, pitch)
    wt[:, :c] = w.reshape(c, k * k).t()
    sc = torch.zeros(pitch)
    sh = torch.zeros(pitch)
    sc[:c] = s64.float()
    sh[:c] = t64.float()
    return x.to(dev), wt.contiguous().to(dev), sc.to(dev), sh.to(dev)


def _dw_run(eng, xh, xl, wt, sc, sh, pitch, hin, k, stride, act_in, act_out):
    dev = xh.device
    batch = xh.shape[0]
    ho = (hin - 1) // stride + 1
    n_out = batch * ho * ho * pitch
    oh = torch.full((n_out + 64,), float("nan"), dtype=torch.float16, device=dev)
    ol = torch.full_like(oh, float("nan"))
    rc = eng._lib.mpx_dwconv_bn_act(eng._h, ptr(xh), ptr(xl), ptr(wt), ptr(sc), ptr(sh), ptr(oh), ptr(ol), batch, hin, pitch, k, stride, act_in, act_out, eng._stream())
    _lib.check(eng._h, rc, "mpx_dwconv_bn_act")
    torch.cuda.synchronize()
    assert torch.isnan(oh[n_out:]).all() and torch.isnan(ol[n_out:]).all()              # the neighbours behind the planes are untouched
    return oh[:n_out].view(batch, ho, ho, pitch), ol[:n_out].view(batch, ho, ho, pitch)


def _dw_check(eng, xh, xl, wt, sc, sh, c, pitch, hin, k, stride, act_in, act_out, what):
    """Runs the kernel and checks every image against fp64.  -> (worst err / bound, merged output)."""
    yh, yl = _dw_run(eng, xh, xl, wt, sc, sh, pitch, hin, k, stride, act_in, act_out)
    got = merge(yh, yl).double()
    assert not torch.isnan(got).any(), what
    if pitch > c:                                                                       # padded outputs: exact zeros, both planes
        assert (yh[..., c:].view(torch.int16) == 0).all() and (yl[..., c:].view(torch.int16) == 0).all(), what
    x64 = merge(xh[..., :c], xl[..., :c]).double().permute(0, 3, 1, 2)
    a64 = silu64(x64) if act_in else x64
    w64 = wt[:, :c].double().t().reshape(c, 1, k, k)
    s64, t64 = sc[:c].double()[None, :, None, None], sh[:c].double()[None, :, None, None]
    pad = (k - 1) // 2
    acc = F.conv2d(a64, w64, None, stride, pad, 1, c)
    mag = F.conv2d(a64.abs(), w64.abs(), None, stride, pad, 1, c)
    pre = s64 * acc + t64
    want = (silu64(pre) if act_out else pre).permute(0, 2, 3, 1)
    tol = (2.0 ** -18 * (s64.abs() * mag + t64.abs()) + 2.0 ** -24).permute(0, 2, 3, 1)
    worst = ((got[..., :c] - want).abs() / tol).max().item()
    print("%s: worst err / bound %.3f" % (what, worst))
    assert worst <= 1.0, (what, worst)
    return worst, got


DW_CASES = [
    # channels, pitch, hin, kernel, stride, batch
    (8, 8, 1, 5, 1, 1),             # a single pixel: every tap but the centre is clipped
    (8, 8, 2, 5, 2, 2),             # a map smaller than the kernel
    (16, 32, 7, 5, 1, 3),           # a short last run, pad channels, a batch index > 0
    (24, 32, 14, 5, 2, 2),          # even side at stride 2
    (8, 8, 13, 5, 2, 1),            # odd side at stride 2
    (40, 40, 9, 3, 2, 1),           # a pitch that is not a multiple of 32
    (32, 32, 6, 3, 1, 2),           # a 3x3 stride-1 layer
]


@pytest.mark.parametrize("act_out", [0, 1])
@pytest.mark.parametrize("act_in", [0, 1])
@pytest.mark.parametrize("c,pitch,hin,k,stride,batch", DW_CASES)
def test_depthwise_against_fp64(small_engine, dev, c, pitch, hin, k, stride, batch, act_in, act_out):
    x, wt, sc, sh = _dw_inputs(c, pitch, hin, k, batch, seed=1000 * c + 10 * hin + stride, dev=dev)
    xh, xl = split(x)
    x64 = merge(xh, xl)
    if hin >= 6:
        assert (x64 == 0).any() and (x64 > 10).any() and (x64 < -10).any() and (sc[:c] < 0).any()
    _dw_check(small_engine, xh, xl, wt, sc, sh, c, pitch, hin, k, stride, act_in, act_out,
              "depthwise C %d pitch %d %dx%d k %d stride %d batch %d act %d/%d" % (c, pitch, hin, hin, k, stride, batch, act_in, act_out))


def test_depthwise_silu_is_not_the_linear_kernel(small_engine, dev):
    """The SiLU variants differ from the linear one by far more than the bound: what the comparisons above accept is the activation."""
    c, pitch, hin, k, stride, batch = 16, 32, 7, 5, 1, 3
    x, wt, sc, sh = _dw_inputs(c, pitch, hin, k, batch, seed=77, dev=dev)
    xh, xl = split(x)
    outs = {}
    for act_in, act_out in ((0, 0), (1, 0), (0, 1), (1, 1)):
        _w, outs[act_in, act_out] = _dw_check(small_engine, xh, xl, wt, sc, sh, c, pitch, hin, k, stride, act_in, act_out, "depthwise act %d/%d" % (act_in, act_out))
    scale = outs[0, 0].abs().max().item()
    for key in ((1, 0), (0, 1), (1, 1)):
        diff = (outs[key] - outs[0, 0]).abs().max().item()
        print("act %s vs linear: max |d| %.3f of scale %.3f" % (key, diff, scale))
        assert diff > 1e4 * 2.0 ** -18 * scale
    assert (outs[1, 1] - outs[1, 0]).abs().max().item() > 1e4 * 2.0 ** -18 * scale


def test_depthwise_with_engine_layer_parameters(small_engine, dev, sd):
    """The device vectors mpx_load_dwconv made for a padded 5x5 layer (features.3.1.block.1.0: 240 channels at pitch 256, 25 taps), and
    the kernel run with them at the layer's own shape."""
    eng = small_engine
    k_idx = [d.name.decode() for d in eng.dwconvs].index("features.3.1.block.1.0")
    d = eng.dwconvs[k_idx]
    assert (d.channels, d.pitch, d.stride, d.hin, eng.dw_ksizes[k_idx]) == (240, 256, 1, 28, 5)
    pw, ps, pt = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert eng._lib.mpx_dwconv_params(eng._h, k_idx, C.byref(pw), C.byref(ps), C.byref(pt)) == 0
    got_w, got_s, got_t = dev_view(pw, 25 * 256, dev).view(25, 256), dev_view(ps, 256, dev), dev_view(pt, 256, dev)
    name, bn = d.name.decode(), d.bn_name.decode()
    assert torch.equal(got_w[:, :240], sd[name + ".weight"].reshape(240, 25).t()) and (got_w[:, 240:] == 0).all()
    s64 = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + EPS)
    assert torch.equal(got_s[:240], s64.float()) and torch.equal(got_t[:240], (sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * s64).float())
    assert (got_s[240:] == 0).all() and (got_t[240:] == 0).all()
    batch = 3
    x, _wt, _sc, _sh = _dw_inputs(240, 256, 28, 5, batch, seed=5, dev=dev)
    xh, xl = split(x)
    _dw_check(eng, xh, xl, got_w.contiguous().to(dev), got_s.to(dev), got_t.to(dev), 240, 256, 28, 5, 1, 1, 1, "engine layer %s batch %d" % (name, batch))


def test_depthwise_strides_over_the_rest_of_a_capped_grid(small_engine, dev):
    """8 channels of a 224x224 map at batch 48: 48 * 224 * 56 = 602,112 runs of one 8-channel group each, more than the 2048 x 256 threads
    of the capped grid on 256 CUs: the first threads take a second unit."""
    eng = small_engine
    c = pitch = 8
    hin, batch = 224, 48
    assert batch * hin * (hin // 4) > eng.num_cus * 8 * 256
    x, wt, sc, sh = _dw_inputs(c, pitch, hin, 3, batch, seed=9, dev=dev)
    xh, xl = split(x)
    _dw_check(eng, xh, xl, wt, sc, sh, c, pitch, hin, 3, 1, 1, 1, "depthwise 8 channels 224x224 batch 48")


def test_depthwise_refuses_bad_arguments(small_engine, dev):
    eng = small_engine
    z = torch.zeros(4096, dtype=torch.float16, device=dev)
    f = torch.zeros(1024, dtype=torch.float32, device=dev)
    a, b = ptr(z), ptr(f)
    call = eng._lib.mpx_dwconv_bn_act
    assert call(eng._h, a, a, b, b, b, a, a, 1, 4, 8, 5, 1, 1, 1, None) == 0
    torch.cuda.synchronize()
    assert call(eng._h, None, a, b, b, b, a, a, 1, 4, 8, 5, 1, 1, 1, None) == -1          # null planes
    assert call(eng._h, a, a, None, b, b, a, a, 1, 4, 8, 5, 1, 1, 1, None) == -1          # null weights
    assert call(eng._h, a, a, b, b, b, a, a, 0, 4, 8, 5, 1, 1, 1, None) == -1             # empty batch
    assert call(eng._h, a, a, b, b, b, a, a, 1, 0, 8, 5, 1, 1, 1, None) == -1             # empty map
    assert call(eng._h, a, a, b, b, b, a, a, 1, 4, 12, 5, 1, 1, 1, None) == -1            # pitch % 8
    assert call(eng._h, a, a, b, b, b, a, a, 1, 4, 0, 5, 1, 1, 1, None) == -1             # pitch 0
    for ksize in (1, 4, 7):
        assert call(eng._h, a, a, b, b, b, a, a, 1, 4, 8, ksize, 1, 1, 1, None) == -1     # kernel size
    for stride in (0, 3):
        assert call(eng._h, a, a, b, b, b, a, a, 1, 4, 8, 5, stride, 1, 1, None) == -1    # stride
    assert call(eng._h, a, a, b, b, b, a, a, 1, 4, 8, 5, 1, 2, 1, None) == -1             # act codes
    assert call(eng._h, a, a, b, b, b, a, a, 1, 4, 8, 5, 1, 1, -1, None) == -1
    assert call(eng._h, C.c_void_p(z.data_ptr() + 2), a, b, b, b, a, a, 1, 4, 8, 5, 1, 1, 1, None) == -1      # misaligned
    assert call(eng._h, a, a, C.c_void_p(f.data_ptr() + 4), b, b, a, a, 1, 4, 8, 5, 1, 1, 1, None) == -1


# ------------------------------------------------------------------------------------------------
# Squeeze-and-Excitation: gate and scale
# ------------------------------------------------------------------------------------------------
def _se_inputs(c, pitch, hw, q, batch, seed, dev):
    """Planes (pads exact zeros), fc1 [q][pitch] and fc2 j-major [q][pitch] with zero pad columns, b2 with -inf on the pads: the layout
    mpx_load_se uploads.  b2 is chosen so that image 0's fp64 pre-sigmoid values are -4 .. 4 in even steps (in a shuffled channel order): its
    gates cover (0, 1) -- 0.018 and 0.982 at the ends, 0.36 and 0.64 next to the middle -- whatever the draws."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, hw, pitch, generator=g) * 2.0 + torch.randn(1, 1, pitch, generator=g)
    x[torch.rand(x.shape, generator=g) < 0.1] = 0.0
    x[..., : max(1, c // 4)] *= 1e-3
    x[..., c:] = 0.0
    w1 = torch.zeros(q, pitch)
    w1[:, :c] = torch.randn(q, c, generator=g) * (2.0 / c) ** 0.5
    b1 = torch.randn(q, generator=g) * 0.3
    w2 = torch.zeros(q, pitch)
    w2[:, :c] = torch.randn(q, c, generator=g) * (4.0 / q) ** 0.5
    xh, xl = split(x[:1])
    s1 = silu64(merge(xh, xl).double()[0, :, :c].mean(0) @ w1[:, :c].double().t() + b1.double())
    b2 = torch.full((pitch,), float("-inf"))
    b2[:c] = (torch.linspace(-4.0, 4.0, c)[torch.randperm(c, generator=g)].double() - s1 @ w2[:, :c].double()).float()
    return x.to(dev), w1.to(dev), b1.to(dev), w2.to(dev), b2.to(dev)


def _se_gate_run(eng, xh, xl, w1, b1, w2, b2, hw, pitch, q):
    batch = xh.shape[0]
    out = torch.full((batch * pitch + 64,), float("nan"), dtype=torch.float32, device=xh.device)
    rc = eng._lib.mpx_se_gate(eng._h, ptr(xh), ptr(xl), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(out), batch, hw, pitch, q, eng._stream())
    _lib.check(eng._h, rc, "mpx_se_gate")
    torch.cuda.synchronize()
    assert torch.isnan(out[batch * pitch:]).all()
    return out[: batch * pitch].view(batch, pitch).clone()


def _se_gate_want(xh, xl, w1, b1, w2, b2, c, hw, pitch, q):
    """fp64 gates of the real channels and their propagated bound (module docstring)."""
    x = merge(xh, xl).double()[..., :c]                            # [B][hw][c]
    W1, B1, W2, B2 = w1[:, :c].double(), b1.double(), w2[:, :c].double(), b2[:c].double()
    pooled = x.mean(1)
    d_pool = hw * U * x.abs().mean(1)
    z1 = pooled @ W1.t() + B1
    d_z1 = d_pool @ W1.abs().t() + (math.ceil(pitch / 64) + 7) * U * (pooled.abs() @ W1.abs().t() + B1.abs())
    s1 = silu64(z1)
    d_s1 = 1.1 * d_z1 + 4 * U * s1.abs()
    z2 = s1 @ W2 + B2
    d_z2 = d_s1 @ W2.abs() + (q + 1) * U * (s1.abs() @ W2.abs() + B2.abs())
    gate = 1.0 / (1.0 + torch.exp(-z2))
    return gate, 0.25 * d_z2 + 4 * U * gate


SE_CASES = [(8, 8, 1, 1, 1), (16, 32, 49, 6, 3), (48, 64, 257, 12, 2), (8, 8, 12544, 4, 1)]        # channels, pitch, pixels, q, batch


@pytest.mark.parametrize("c,pitch,hw,q,batch", SE_CASES)
def test_se_gate_against_fp64(small_engine, dev, c, pitch, hw, q, batch):
    eng = small_engine
    x, w1, b1, w2, b2 = _se_inputs(c, pitch, hw, q, batch, seed=100 * c + hw, dev=dev)
    xh, xl = split(x)
    got = _se_gate_run(eng, xh, xl, w1, b1, w2, b2, hw, pitch, q)
    assert (got[:, c:].view(torch.int32) == 0).all()                                    # pad channels: exactly +0
    want, tol = _se_gate_want(xh, xl, w1, b1, w2, b2, c, hw, pitch, q)
    assert (want < 0.1).any() and (want > 0.9).any() and ((want > 0.3) & (want < 0.7)).any()       # the yardstick's gates cover (0, 1)
    err = (got[:, :c].double() - want).abs()
    print("SE gate C %d pitch %d hw %d q %d batch %d: gates %.4f .. %.4f, max err %.3e, worst err / bound %.3f"
          % (c, pitch, hw, q, batch, want.min().item(), want.max().item(), err.max().item(), (err / tol).max().item()))
    assert not torch.isnan(got).any() and (err <= tol).all()
    # the same bits on a second run
    again = _se_gate_run(eng, xh, xl, w1, b1, w2, b2, hw, pitch, q)
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize("c,pitch,hw,q", [(16, 32, 49, 6), (48, 64, 257, 12), (144, 160, 196, 6)])
def test_se_gate_of_an_image_has_the_same_bits_alone_and_inside_a_batch(small_engine, dev, c, pitch, hw, q):
    eng = small_engine
    x, w1, b1, w2, b2 = _se_inputs(c, pitch, hw, q, 3, seed=31 + c, dev=dev)
    xh, xl = split(x)
    in_batch = _se_gate_run(eng, xh, xl, w1, b1, w2, b2, hw, pitch, q)
    alone = _se_gate_run(eng, xh[2:3].contiguous(), xl[2:3].contiguous(), w1, b1, w2, b2, hw, pitch, q)
    assert torch.equal(alone[0].view(torch.int32), in_batch[2].view(torch.int32))
    assert not torch.equal(in_batch[0], in_batch[2])                                    # ... and the images are different images


def test_se_gate_with_engine_layer_parameters(small_engine, dev, sd):
    """The device vectors mpx_load_se made for a padded layer (features.3.0.block.2: 144 channels at pitch 160, q 6)."""
    eng = small_engine
    k = [d.name.decode() for d in eng.ses].index("features.3.0.block.2")
    d = eng.ses[k]
    assert (d.channels, d.pitch, d.q, d.hw) == (144, 160, 6, 28)
    ptrs = [C.c_void_p() for _ in range(4)]
    assert eng._lib.mpx_se_params(eng._h, k, *[C.byref(p) for p in ptrs]) == 0
    w1, b1, w2, b2 = dev_view(ptrs[0], 6 * 160, dev).view(6, 160), dev_view(ptrs[1], 6, dev), dev_view(ptrs[2], 6 * 160, dev).view(6, 160), dev_view(ptrs[3], 160, dev)
    name = d.name.decode()
    assert torch.equal(w1[:, :144], sd[name + ".fc1.weight"].reshape(6, 144)) and (w1[:, 144:] == 0).all()
    assert torch.equal(w2[:, :144], sd[name + ".fc2.weight"].reshape(144, 6).t()) and (w2[:, 144:] == 0).all()
    assert torch.equal(b1, sd[name + ".fc1.bias"]) and torch.equal(b2[:144], sd[name + ".fc2.bias"]) and torch.isneginf(b2[144:]).all()
    x = _se_inputs(144, 160, 784, 6, 2, seed=3, dev=dev)[0]
    xh, xl = split(x)
    args = [t.to(dev) for t in (w1, b1, w2, b2)]
    got = _se_gate_run(eng, xh, xl, *args, 784, 160, 6)
    want, tol = _se_gate_want(xh, xl, *args, 144, 784, 160, 6)
    assert ((got[:, :144].double() - want).abs() <= tol).all() and (got[:, 144:].view(torch.int32) == 0).all()


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("c,pitch,hw,batch", [(16, 32, 49, 3), (8, 8, 1, 1), (40, 40, 12544, 7)])
def test_se_scale_against_the_exact_product(small_engine, dev, c, pitch, hw, batch, in_place):
    eng = small_engine
    g = torch.Generator().manual_seed(c + hw)
    x = torch.randn(batch, hw, pitch, generator=g) * 3.0
    x[torch.rand(x.shape, generator=g) < 0.1] = 0.0
    x[..., : max(1, c // 4)] *= 1e-3
    x[..., c:] = 0.0
    gate = torch.rand(batch, pitch, generator=g)
    gate[:, c:] = 0.0
    gate[:, 0] = 1.0
    xh, xl = split(x.to(dev))
    gate = gate.to(dev)
    want = merge(xh, xl).double() * gate.double()[:, None, :]
    n = batch * hw * pitch
    if in_place:
        oh = torch.cat([xh.reshape(-1), torch.full((64,), float("nan"), dtype=torch.float16, device=dev)])
        ol = torch.cat([xl.reshape(-1), torch.full((64,), float("nan"), dtype=torch.float16, device=dev)])
        ih, il = oh, ol
    else:
        oh = torch.full((n + 64,), float("nan"), dtype=torch.float16, device=dev)
        ol = torch.full_like(oh, float("nan"))
        ih, il = xh, xl
    _lib.check(eng._h, eng._lib.mpx_se_scale(eng._h, ptr(ih), ptr(il), ptr(gate), ptr(oh), ptr(ol), batch, hw, pitch, eng._stream()), "mpx_se_scale")
    torch.cuda.synchronize()
    assert torch.isnan(oh[n:]).all() and torch.isnan(ol[n:]).all()
    got = merge(oh[:n], ol[:n]).double().view(batch, hw, pitch)
    tol = (2.0 ** -24 + 2.0 ** -22) * want.abs() + 2.0 ** -24
    err = (got - want).abs()
    print("SE scale C %d pitch %d hw %d batch %d in place %d: worst err / bound %.3f" % (c, pitch, hw, batch, in_place, (err / tol).max().item()))
    assert (err <= tol).all()
    assert (oh[:n].view(batch, hw, pitch)[..., c:].view(torch.int16) == 0).all() and (ol[:n].view(batch, hw, pitch)[..., c:].view(torch.int16) == 0).all()


def test_se_entries_refuse_bad_arguments(small_engine, dev):
    eng = small_engine
    z = torch.zeros(4096, dtype=torch.float16, device=dev)
    f = torch.zeros(4096, dtype=torch.float32, device=dev)
    a, b = ptr(z), ptr(f)
    gate, scale = eng._lib.mpx_se_gate, eng._lib.mpx_se_scale
    assert gate(eng._h, a, a, b, b, b, b, ptr(torch.zeros(64, device=dev)), 1, 4, 8, 3, None) == 0
    assert scale(eng._h, a, a, b, a, a, 1, 4, 8, None) == 0
    torch.cuda.synchronize()
    off = C.c_void_p(f.data_ptr() + 4)
    assert gate(eng._h, None, a, b, b, b, b, b, 1, 4, 8, 3, None) == -1
    assert gate(eng._h, a, a, b, None, b, b, b, 1, 4, 8, 3, None) == -1
    assert gate(eng._h, a, a, b, b, b, b, None, 1, 4, 8, 3, None) == -1
    assert gate(eng._h, a, a, b, b, b, b, b, 0, 4, 8, 3, None) == -1
    assert gate(eng._h, a, a, b, b, b, b, b, 1, 0, 8, 3, None) == -1
    assert gate(eng._h, a, a, b, b, b, b, b, 1, 4, 12, 3, None) == -1
    assert gate(eng._h, a, a, b, b, b, b, b, 1, 4, 8, 0, None) == -1
    assert gate(eng._h, a, a, off, b, b, b, b, 1, 4, 8, 3, None) == -1
    assert gate(eng._h, a, a, b, b, b, b, off, 1, 4, 8, 3, None) == -1
    assert gate(eng._h, a, a, b, b, b, b, b, 1, 4, 8192, 3, None) == -1                  # two copies of the pitch pass 64 KB of LDS
    assert scale(eng._h, None, a, b, a, a, 1, 4, 8, None) == -1
    assert scale(eng._h, a, a, None, a, a, 1, 4, 8, None) == -1
    assert scale(eng._h, a, a, b, a, a, 0, 4, 8, None) == -1
    assert scale(eng._h, a, a, b, a, a, 1, 0, 8, None) == -1
    assert scale(eng._h, a, a, b, a, a, 1, 4, 20, None) == -1
    assert scale(eng._h, a, a, off, a, a, 1, 4, 8, None) == -1
    assert scale(eng._h, C.c_void_p(z.data_ptr() + 2), a, b, a, a, 1, 4, 8, None) == -1


# ------------------------------------------------------------------------------------------------
# SiLU global average pool
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,c,batch", [(49, 1280, 2), (1, 8, 1)])
def test_silu_global_pool_against_fp64(small_engine, dev, hw, c, batch):
    eng = small_engine
    g = torch.Generator().manual_seed(hw + c)
    x = torch.randn(batch, hw, c, generator=g) * 4.0
    x[..., : max(1, c // 4)] *= 1e-3
    x[:, :, -1] = -30.0 + torch.arange(hw)[None, :] * -3.0               # far negative: expf(-x) grows to +inf and silu goes to -0
    xh, xl = split(x.to(dev))
    oh = torch.full((batch * c + 64,), float("nan"), dtype=torch.float16, device=dev)
    ol = torch.full_like(oh, float("nan"))
    _lib.check(eng._h, eng._lib.mpx_global_avgpool_silu(eng._h, ptr(xh), ptr(xl), ptr(oh), ptr(ol), batch, hw, c, eng._stream()), "mpx_global_avgpool_silu")
    torch.cuda.synchronize()
    assert torch.isnan(oh[batch * c:]).all() and torch.isnan(ol[batch * c:]).all()
    x64 = merge(xh, xl).double()
    a = silu64(x64)
    want = a.mean(1)
    tol = ((hw + 4) * 2.0 ** -24 + 2.0 ** -22) * a.abs().mean(1) + 2.0 ** -24
    got = merge(oh[: batch * c].view(batch, c), ol[: batch * c].view(batch, c)).double()
    err = (got - want).abs()
    print("SiLU pool %d x %d batch %d: max err %.3e, worst err / bound %.3f; the plain mean is %.3f away"
          % (hw, c, batch, err.max().item(), (err / tol).max().item(), (x64.mean(1) - want).abs().max().item()))
    assert not torch.isnan(got).any() and (err <= tol).all()
    assert (x64.mean(1) - want).abs().max().item() > 0.01           # the plain pool of the same planes is a different number
    z = ptr(xh)
    assert eng._lib.mpx_global_avgpool_silu(eng._h, z, z, z, z, 1, 49, 12, None) == -1
    assert eng._lib.mpx_global_avgpool_silu(eng._h, z, z, z, z, 0, 49, 16, None) == -1
    assert eng._lib.mpx_global_avgpool_silu(eng._h, None, z, z, z, 1, 49, 16, None) == -1


# ------------------------------------------------------------------------------------------------
# per conv layer
# ------------------------------------------------------------------------------------------------
def _ref_layer(sd, d, x64, res64):
    """fp64 conv + BatchNorm (+ residual), NO activation: the SiLU belongs to the consumer.  [B][cout][ho][ho] on the device."""
    name, bn = d.name.decode(), d.bn_name.decode()
    dev = x64.device
    y = F.conv2d(x64, sd[name + ".weight"].double().reshape(d.cout, d.cin, d.ksize, d.ksize).to(dev), None, d.stride, d.pad)
    if bn:
        g, b, m, v = (sd["%s.%s" % (bn, k)].double().to(dev)[None, :, None, None] for k in ("weight", "bias", "running_mean", "running_var"))
        y = (y - m) / torch.sqrt(v + EPS) * g + b
    else:
        y = y + sd[name + ".bias"].double().to(dev)[None, :, None, None]
    if res64 is not None:
        y = y + res64
    assert d.relu == 0
    return y


def _check(eng, sd, i, batch, tile=-1):
    d = eng.layers[i]
    fields = "%d->%d k%d h%d K %d res %d " % (d.cin, d.cout, d.ksize, d.hin, d.k_packed, d.residual)
    ran, want = check_conv_layer(eng, i, batch, lambda d, x64, r64: _ref_layer(sd, d, x64, r64), tile, clamp=False, pitched=True, fields=fields)
    assert (want < -0.5).any()                  # the inputs are signed: a layer that applied ReLU would show
    return ran


def test_every_distinct_conv_shape_on_every_accepted_tile(small_engine, sd):
    """Every distinct (cin, cout, ksize, hin, residual) of the conv list on every tile it accepts: the stem (3x3 stride 2 pad 1 on the NHWC4
    staging), the K = 32 layers (one K step), the padded layers (16, 24, 40, 80, 112, 144, 240 channels), project layers with and without
    their residual, features.8 and the classifier.  Batch 2, so that an image index > 0 is covered; features.8 -- the one layer the 256-row
    tiles accept -- runs a second batch large enough for tile 9's and tile 10's own kernels
    (tile 13, one persistent workgroup per CU, needs a whole round of 256 tiles and hands 165 to tile 2)."""
    eng = small_engine
    seen, count, one_step, padded, with_res = set(), 0, 0, 0, 0
    for i, d in enumerate(eng.layers):
        key = (d.cin, d.cout, d.ksize, d.hin, d.residual)
        if key in seen:
            continue
        seen.add(key)
        accepted = accepted_tiles(eng, i)
        default = eng._lib.mpx_get_conv_tile(eng._h, i)
        assert default in accepted and GENERIC <= set(accepted), (d.name, accepted)
        if d.cin % 32 or d.cout % 32 and i != len(eng.layers) - 1:
            assert set(accepted) == GENERIC, (d.name, accepted)             # padded layers: the generic tiles only
            padded += 1
        one_step += d.k_packed == 32
        with_res += d.residual
        for t in accepted:
            batches = (2, 171) if (d.cout == 1280 and (t == default or t in FALLBACK)) else (2,)
            for batch in batches:
                ran = _check(eng, sd, i, batch, tile=t)
                assert ran & ((1 << t) | (1 << FALLBACK.get(t, t))), (d.name, t, ran)
                if t not in FALLBACK:
                    assert ran == 1 << t, (d.name, t, ran)
                if d.cout == 1280 and batch == 171 and t in (9, 10):
                    assert ran & (1 << t), (d.name, t, ran)                 # the kernel itself ran on K = 320
        count += 1
    print("distinct conv shapes checked: %d (K = 32: %d, padded: %d, with a residual: %d)" % (count, one_step, padded, with_res))
    assert count == 21 and one_step == 3 and padded == 15 and with_res == 5       # counted from the per-block table


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
def test_efficientnet_end_to_end(engine, sd, golden_dir):
    """Logits lens (tests/logits_lens.py): all 1000 logits of every row against fp64, bound 4 d_L with d_L = the fp32 CPU loop's distance.  Measured on one MI355X: efficientnet_b0 d_L 1.58e-05, engine 2.17e-05 (1.38)."""
    r = Reference(ref, sd)
    check_end_to_end(engine, ARCH, r, e2e_rows(r, ref.E2E_CASES, golden_dir),
                     "%(arch)s: yardstick distance %(d).3e over the 28 rows -> end-to-end bound %(bound).1e", peaks=True)


def test_a_mask_row_scores_the_same_bits_wherever_it_sits(engine, golden_dir):
    check_position_independence(engine, *ref.e2e_inputs(golden_dir, "felz"), (8, ((1, 0, (0,)), (37, 41, (0, 5, 36)), (700, 44, (3, 511, 512, 699)))))


# ------------------------------------------------------------------------------------------------
# API, profile and errors
# ------------------------------------------------------------------------------------------------
def test_api_on_an_efficientnet_engine(engine, sd, golden_dir):
    check_api(engine, Reference(ref, sd), *ref.e2e_inputs(golden_dir, "felz"))


def test_profile_lists_the_depthwise_and_se_launches(engine, dev):
    eng = engine
    img = torch.from_numpy(synth.make_images(1, kind="noise")[0]).to(dev)
    seg = torch.from_numpy(synth.grid_segments()).to(dev)
    onoff = torch.from_numpy(synth.random_onoff(4, 196)).to(dev)
    labels = torch.zeros(4, dtype=torch.int32, device=dev)
    eng.profile(True)
    eng.stage_masks(img, seg, onoff, 0)
    eng.forward(4, labels)
    eng.profile(False)
    prof = eng.collect_profile()
    assert len(prof["per_dw_ms"]) == len(eng.dwconvs) == 16 and all(ms > 0 for ms in prof["per_dw_ms"])
    assert len(prof["per_se_gate_ms"]) == len(eng.ses) == 16 and all(ms > 0 for ms in prof["per_se_gate_ms"])
    assert len(prof["per_se_scale_ms"]) == 16 and all(ms > 0 for ms in prof["per_se_scale_ms"])
    assert prof["per_norm_ms"] == [] and prof["avgpool2_ms"] == 0 and prof["per_shuffle_ms"] == [] and prof["per_clip_pool_ms"] == []
    assert prof["launches"]["pool"] == 16 + 16 + 16 + 1     # every depthwise layer, gate and scale, and the SiLU global pool
    assert prof["launches"]["conv"] == len(eng.layers) == 34
    assert prof["launches"]["head"] == 1


def test_efficientnet_error_paths(small_engine, mpx_lib, dev, sd):
    eng = small_engine
    with pytest.raises(ValueError):
        MaskedForwardEngine(ARCH, max_batch=2, device=0, stem="table")
    with pytest.raises(ValueError):
        eng.score_masks(synth.make_images(1)[0], synth.grid_segments(), synth.random_onoff(2, 196), 0, stem="table")
    z = torch.zeros(224, 224, dtype=torch.int32, device=dev)
    im = torch.zeros(224, 224, 3, dtype=torch.uint8, device=dev)
    on = torch.ones(1, 1, dtype=torch.uint8, device=dev)
    mean = (C.c_float * 3)(*scorer.MEAN)
    std = (C.c_float * 3)(*scorer.STD)
    assert eng._lib.mpx_stem_table_build(eng._h, ptr(im), None, ptr(z), 1, mean, std, None) == -2
    assert eng._lib.mpx_stem_table_apply(eng._h, ptr(on), 1, 1, 0, None) == -2
    buf = torch.zeros(64, dtype=torch.float16, device=dev)
    assert eng._lib.mpx_stem_conv_maxpool(eng._h, ptr(buf), ptr(buf), 1, None) == -2
    for bad in (10001, 10010, 10999):
        h = C.c_void_p()
        assert mpx_lib.mpx_create(bad, 2, 0, C.byref(h)) == -1 and not h.value
    se = _lib.SeDesc()
    assert eng._lib.mpx_se_info(eng._h, 16, C.byref(se)) == -1 and eng._lib.mpx_se_info(eng._h, -1, C.byref(se)) == -1
    a = C.c_int()
    assert eng._lib.mpx_conv_consumer_act(eng._h, 34, C.byref(a)) == -1 and eng._lib.mpx_dwconv_shape(eng._h, 16, None, None, None) == -1
    v = torch.ones(8192)
    vp = C.c_void_p(v.data_ptr())
    assert eng._lib.mpx_load_se(eng._h, 16, vp, vp, vp, vp) == -1
    assert eng._lib.mpx_load_se(eng._h, 0, vp, None, vp, vp) == -1
    fresh = MaskedForwardEngine(ARCH, max_batch=2, device=0)
    try:
        assert len(fresh.ses) == 16 and len(fresh.dwconvs) == 16
        fresh.load_state_dict(sd, only=[d.name.decode() for d in fresh.layers] + [d.name.decode() for d in fresh.dwconvs])   # no SE layer
        assert fresh._lib.mpx_weights_complete(fresh._h) == 0
        fresh.stage_masks(im, z, on, 0)
        labels = torch.zeros(1, dtype=torch.int32, device=dev)
        score = torch.zeros(1, device=dev)
        pred = torch.zeros(1, dtype=torch.int32, device=dev)
        assert fresh._lib.mpx_forward(fresh._h, ptr(labels), ptr(score), ptr(pred), None, 1, None) == -2       # missing SE weights
        with pytest.raises(KeyError):
            fresh.load_state_dict(synth.make_state_dict("mobilenet_v2"))
        with pytest.raises(KeyError):
            fresh.load_state_dict(sd, only=["features.2.0.block.9"])
        fresh.load_state_dict(sd, only=[d.name.decode() for d in fresh.ses])
        assert fresh._lib.mpx_weights_complete(fresh._h) == 1
        assert fresh._lib.mpx_forward(fresh._h, ptr(labels), ptr(score), ptr(pred), None, 1, None) == 0
        torch.cuda.synchronize()
    finally:
        fresh.close()
    # a MobileNetV2 engine has no SE layers, and its depthwise layers keep their shape
    r = MaskedForwardEngine("mobilenet_v2", max_batch=2, device=0)
    try:
        assert r._lib.mpx_num_se(r._h) == 0 and r.ses == [] and set(r.dw_ksizes) == {3}
        v3 = C.c_int(), C.c_int(), C.c_int()
        assert r._lib.mpx_dwconv_shape(r._h, 0, *[C.byref(x) for x in v3]) == 0 and [x.value for x in v3] == [3, 0, 0]
        a = C.c_int(-1)
        assert r._lib.mpx_conv_consumer_act(r._h, 0, C.byref(a)) == 0 and a.value == 0
    finally:
        r.close()
