"""MobileNetV2 on the MI355X (pytest -m gpu), through the C-ABI as tests/test_gpu_densenet.py does: the topology and the default tile of
every layer, the depthwise 3x3 + BN + ReLU6 kernel and the clamped global pool against fp64 with bounds derived from their roundings,
every distinct conv shape on every tile it accepts against an fp64 conv + BatchNorm of the same split inputs, the whole network against
the batch-1 fp32 CPU loop and the fp64 restatement (tests/mobilenet_ref.py), position independence of a mask row, the reference-named
API and the error paths.

Bounds.
  Depthwise, per element: |err| <= 2^-19 (|s| sum|w_i x_i| + |t|) + 2^-24.  An unfused nine-tap sum makes up to 9 products + 8 adds,
  the BatchNorm two more roundings, each 2^-24 relative to a partial result that sum|w_i x_i| (times |s|, plus |t|) bounds, and the
  re-split 2^-22: 23 x 2^-24 < 2^-19.  (The kernel fuses each tap into one fma and stays well inside.  Its BatchNorm compiles to ONE fma
  as well, one rounding where this count has two -- DESIGN.md 33 --, so the bound covers the kernel as it is and the two-rounding run form
  of csrc/mpx_dw.h alike.)  Wherever the fp64 value lies
  above 6 or below 0 by more than the bound the result must be exactly 6 or exactly 0.
  Clamped pool, per element: (hw 2^-24 + 2^-22) mean|min(x_i, 6)| + 2^-24 -- hw - 1 sequential fp32 adds and the division (2^-24 each,
  relative to at most sum|.|), the re-split (2^-22), and lo's fp16 subnormal step as the absolute floor.
  Per conv layer: 4e-6 sqrt(max(K, 4608) / 4608) of max(|want|, 1), the project's per-layer bound (every K here is <= 960: 4e-6).
  End to end: the fp32 batch-1 CPU loop is the yardstick.  With d = max |fp32 loop - fp64| over the 28 rows, the bound on |engine - fp64|
  and |engine - fp32 loop| is the project's 2e-5 when 4 d < 2e-5, else 4 d rounded up to one digit and never above 1e-4 (the AlexNet
  precedent).  The same argmax on EVERY row (tests/test_mobilenet_cpu.py asserts a top-two fp64 margin >= 1e-3 on exactly these rows).

End-to-end figures measured on one MI355X (rows of mobilenet_ref.E2E_CASES: 20 felzenszwalb + 8 grid masks), max |d| of a score,
felzenszwalb / grid:
    engine vs fp64 3.1e-06 / 5.9e-07   fp32 CPU loop vs fp64 1.6e-06 / 1.1e-06   engine vs fp32 CPU loop 3.2e-06 / 1.3e-06
    4 x 1.6e-06 < 2e-05: the bound is 2e-05.  The test prints them on every run."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import mobilenet_ref
from gpu_common import accepted_tiles, dev, FALLBACK, GENERIC, merge, pitch_of, ptr, split  # noqa: F401  (dev is a fixture)
from net_harness import check_api, check_conv_layer, check_end_to_end, check_position_independence, e2e_rows, Reference
from network_interpretation_imagenet_amd import _lib, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine
from oracle import scorer

pytestmark = pytest.mark.gpu

ARCH = "mobilenet_v2"
EPS = 1e-5


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
    """The unchanged default_tile rules, spelled out for the MobileNetV2 shapes."""
    if d.cout <= 64:
        return 1 if d.ksize >= 3 else 4             # the stem; the 1x1 layers onto 16 .. 64 channels
    if d.cout % 256 == 0 and d.cin % 64 == 0 and d.cin >= 128 and d.cout > d.cin:
        return 10                                   # features.18: 320 -> 1280
    if d.cout > d.cin:
        return 7                                    # every expand conv, and the widening project convs
    return 2                                        # the narrowing project convs with cout > 64, the classifier


def test_mobilenet_topology_and_default_tiles(small_engine):
    eng = small_engine
    convs, dws = mobilenet_ref.topology()
    assert len(convs) == 36 and len(dws) == 17
    assert [(d.name.decode(), d.bn_name.decode(), d.cin, d.cout, d.ksize, d.stride, d.pad, d.hin, d.hout, d.relu, d.residual) for d in eng.layers] == convs
    for d in eng.layers:
        assert d.cout_pad == -(-d.cout // 128) * 128
        assert d.k_packed == (96 if d.cin == 3 else pitch_of(d.cin))
    assert [(d.name.decode(), d.bn_name.decode(), d.channels, d.stride, d.hin) for d in eng.dwconvs] == dws
    assert all(d.pitch == pitch_of(d.channels) and d.clamp_in == 1 for d in eng.dwconvs)
    assert sorted({(d.channels, d.pitch) for d in eng.dwconvs if d.channels != d.pitch}) == [(144, 160)]
    assert eng.flops_per_forward == 2.0 * mobilenet_ref.MACS
    geo = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert eng._lib.mpx_geometry(eng._h, *[C.byref(v) for v in geo]) == 0 and [v.value for v in geo] == [224, 3, 1000, 1000]
    for i, d in enumerate(eng.layers):
        t = eng._lib.mpx_get_conv_tile(eng._h, i)
        assert t == _expected_default_tile(d), (d.name, t)
    assert eng.stem == "conv" and not eng.has_stem_table and eng._lib.mpx_weights_complete(eng._h) == 1
    assert eng._lib.mpx_num_bottleneck_tails(eng._h) == 0 and eng._lib.mpx_num_norms(eng._h) == 0


def test_mobilenet_default_max_batch_and_workspace(engine):
    eng = engine
    assert eng.max_batch == 512
    # per slot: three 112x112x96 split-fp16 buffers and the NHWC4 staging: 15.3 MB
    per_slot = 3 * 2 * 112 * 112 * 96 * 2 + 2 * 230 * 230 * 4 * 2
    w = sum(2 * d.cout_pad * d.k_packed * 2 for d in eng.layers)
    assert per_slot * 512 + w < eng.workspace_bytes < per_slot * 512 + w + (16 << 20)
    print("mobilenet_v2: %.2f MB per slot, workspace %.2f GB at max_batch 512" % (per_slot / 1e6, eng.workspace_bytes / 1e9))


# ------------------------------------------------------------------------------------------------
# depthwise 3x3 + BN + ReLU6
# ------------------------------------------------------------------------------------------------
def _dw_inputs(c, pitch, hin, batch, seed, corner, dev):
    """Planes with values above 6, exact zeros and small magnitudes; weights [c][3][3] (all the weight on one corner tap when `corner`
    is (ky, kx)); BatchNorm with both signs of gamma.  The pitch's padding channels carry finite garbage on the input side: their weights,
    scale and shift are zero."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, hin, hin, pitch, generator=g) * 3.0
    x[torch.rand(x.shape, generator=g) < 0.15] = 0.0
    x[torch.rand(x.shape, generator=g) < 0.10] *= 3.0                     # well above 6
    x[..., : max(1, c // 4)] *= 1e-3                                       # lo in fp16's subnormals
    w = torch.randn(c, 3, 3, generator=g) * (2.0 / 9) ** 0.5
    if corner is not None:
        w = torch.zeros(c, 3, 3)
        w[:, corner[0], corner[1]] = torch.randn(c, generator=g) + 2.0
    gamma = torch.empty(c).uniform_(0.5, 2.5, generator=g) * torch.where(torch.rand(c, generator=g) < 0.2, -1.0, 1.0)
    beta = torch.randn(c, generator=g) * 0.5
    mean = torch.randn(c, generator=g) * 0.3
    var = torch.empty(c).uniform_(0.3, 2.0, generator=g)
    s64 = gamma.double() / torch.sqrt(var.double() + EPS)
    t64 = beta.double() - mean.double() * s64
    wt = torch.zeros(9, pitch)
    wt[:, :c] = w.reshape(c, 9).t()
    sc = torch.zeros(pitch)
    sh = torch.zeros(pitch)
    sc[:c] = s64.float()
    sh[:c] = t64.float()
    return x.to(dev), w, wt.contiguous().to(dev), sc.to(dev), sh.to(dev)


def _dw_check(eng, xh, xl, w, wt, sc, sh, c, pitch, hin, stride, clamp, what, images=None):
    """Runs the kernel on the planes and checks `images` (all by default) against fp64.  -> worst err / bound."""
    dev = xh.device
    batch = xh.shape[0]
    ho = (hin - 1) // stride + 1
    guard = 64
    n_out = batch * ho * ho * pitch
    oh = torch.full((n_out + guard,), float("nan"), dtype=torch.float16, device=dev)
    ol = torch.full_like(oh, float("nan"))
    rc = eng._lib.mpx_dwconv3x3_bn_relu6(eng._h, ptr(xh), ptr(xl), ptr(wt), ptr(sc), ptr(sh), ptr(oh), ptr(ol), batch, hin, pitch, stride, int(clamp), eng._stream())
    _lib.check(eng._h, rc, "mpx_dwconv3x3_bn_relu6")
    torch.cuda.synchronize()
    assert torch.isnan(oh[n_out:]).all() and torch.isnan(ol[n_out:]).all()              # the neighbours behind the planes are untouched
    yh, yl = oh[:n_out].view(batch, ho, ho, pitch), ol[:n_out].view(batch, ho, ho, pitch)
    worst = 0.0
    for n in (range(batch) if images is None else images):
        got = merge(yh[n], yl[n]).double()
        assert not torch.isnan(got).any()
        if pitch > c:                                                                   # padded outputs: exact zeros, both planes
            assert (yh[n, ..., c:].view(torch.int16) == 0).all() and (yl[n, ..., c:].view(torch.int16) == 0).all(), what
        x64 = merge(xh[n, ..., :c], xl[n, ..., :c]).double().permute(2, 0, 1)[None]
        if clamp:
            x64 = x64.clamp_max(6.0)
        w64 = wt[:, :c].double().t().reshape(c, 1, 3, 3)
        s64, t64 = sc[:c].double()[None, :, None, None], sh[:c].double()[None, :, None, None]
        acc = F.conv2d(x64, w64, None, stride, 1, 1, c)
        mag = F.conv2d(x64.abs(), w64.abs(), None, stride, 1, 1, c)
        pre = (s64 * acc + t64)[0].permute(1, 2, 0)
        tol = (2.0 ** -19 * (s64.abs() * mag + t64.abs()) + 2.0 ** -24)[0].permute(1, 2, 0)
        want = pre.clamp(0.0, 6.0)
        g = got[..., :c]
        err = (g - want).abs()
        worst = max(worst, (err / tol).max().item())
        assert (g[pre > 6.0 + tol] == 6.0).all() and (g[pre < -tol] == 0.0).all(), what
        assert (pre > 6.0 + tol).any() and (pre < -tol).any(), what                    # both clamps of ReLU6 are exercised
    print("%s: worst err / bound %.3f" % (what, worst))
    assert worst <= 1.0, (what, worst)
    return worst


DW_CASES = [
    # channels, pitch, hin, stride, batch, clamp_in, corner tap
    (8, 8, 4, 1, 1, 1, None),
    (8, 8, 4, 2, 3, 0, None),             # 4 -> 2
    (8, 8, 5, 2, 1, 1, (0, 0)),           # 5 -> 3, all the weight on the top-left tap
    (24, 32, 7, 2, 3, 1, None),           # 7 -> 4, padded pitch
    (24, 32, 5, 1, 1, 0, (2, 2)),         # all the weight on the bottom-right tap
    (24, 32, 4, 2, 3, 1, (2, 2)),         # 4 -> 2: the bottom-right tap of the last output falls outside the map
    (144, 160, 7, 1, 3, 1, None),
    (144, 160, 4, 2, 1, 0, None),
    (144, 160, 5, 2, 3, 1, (0, 2)),
    (144, 160, 7, 2, 1, 1, (2, 0)),
    (96, 96, 7, 1, 37, 1, None),          # more units than one round of the capped grid's first blocks: the stride over the rest
]


@pytest.mark.parametrize("c,pitch,hin,stride,batch,clamp,corner", DW_CASES)
def test_depthwise_against_fp64(small_engine, dev, c, pitch, hin, stride, batch, clamp, corner):
    x, w, wt, sc, sh = _dw_inputs(c, pitch, hin, batch, seed=1000 * c + 10 * hin + stride, corner=corner, dev=dev)
    xh, xl = split(x)
    _dw_check(small_engine, xh, xl, w, wt, sc, sh, c, pitch, hin, stride, clamp,
              "depthwise C %d pitch %d %dx%d stride %d batch %d clamp %d corner %s" % (c, pitch, hin, hin, stride, batch, clamp, corner))


def test_depthwise_grid_cap_and_engine_layer_parameters(small_engine, dev, sd):
    """A launch far past the grid cap (2048 blocks of 256 units), and the device vectors mpx_load_dwconv made for a padded layer."""
    eng = small_engine
    c, pitch, hin, batch = 144, 160, 28, 40                    # 40 * 28 * 28 * 20 = 627200 units > 2048 * 256
    x, w, wt, sc, sh = _dw_inputs(c, pitch, hin, batch, seed=5, corner=None, dev=dev)
    xh, xl = split(x)
    _dw_check(eng, xh, xl, w, wt, sc, sh, c, pitch, hin, 1, 1, "depthwise 144 / 160 28x28 batch 40", images=(0, 17, 39))
    k = [d.channels for d in eng.dwconvs].index(144)
    d = eng.dwconvs[k]
    pw, ps, pt = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert eng._lib.mpx_dwconv_params(eng._h, k, C.byref(pw), C.byref(ps), C.byref(pt)) == 0

    def view(ptr, n):
        class _V:
            __cuda_array_interface__ = {"data": (ptr.value, False), "shape": (n,), "typestr": "<f4", "version": 2}
        return torch.as_tensor(_V(), device=dev).clone().cpu()

    got_w, got_s, got_t = view(pw, 9 * 160).view(9, 160), view(ps, 160), view(pt, 160)
    name, bn = d.name.decode(), d.bn_name.decode()
    assert torch.equal(got_w[:, :144], sd[name + ".weight"].reshape(144, 9).t()) and (got_w[:, 144:] == 0).all()
    s64 = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + EPS)
    assert torch.equal(got_s[:144], s64.float()) and torch.equal(got_t[:144], (sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * s64).float())
    assert (got_s[144:] == 0).all() and (got_t[144:] == 0).all()


def test_depthwise_planes_past_2_31_elements(small_engine, dev):
    """1800 images of a 56x56x384 map at stride 1: 2.17e9 elements per plane, so input and output offsets pass 2^31 (17 GB, allocated and
    freed here).  Not canonical splits: any (hi, lo) pair is a value.  Checked: the first image, the two around element 2^31, the last."""
    eng = small_engine
    c = pitch = 384
    hin, batch = 56, 1800
    per_img = hin * hin * pitch
    assert batch * per_img > 2 ** 31
    _x, w, wt, sc, sh = _dw_inputs(c, pitch, 4, 1, seed=3, corner=None, dev=dev)
    gen = torch.Generator(device=dev).manual_seed(9)
    xh = torch.empty(batch, hin, hin, pitch, dtype=torch.float16, device=dev)
    xl = torch.empty_like(xh)
    step = 200
    for lo in range(0, batch, step):
        xh[lo:lo + step] = (torch.randn(xh[lo:lo + step].shape, generator=gen, device=dev) * 4).half()
        xl[lo:lo + step] = (torch.randn(xl[lo:lo + step].shape, generator=gen, device=dev) * 1e-3).half()
    try:
        at = 2 ** 31 // per_img
        _dw_check(eng, xh, xl, w, wt, sc, sh, c, pitch, hin, 1, 1, "depthwise past 2^31 elements", images=(0, at - 1, at, batch - 1))
    finally:
        del xh, xl
        torch.cuda.empty_cache()


def test_depthwise_refuses_bad_arguments(small_engine, dev):
    eng = small_engine
    z = torch.zeros(4096, dtype=torch.float16, device=dev)
    f = torch.zeros(1024, dtype=torch.float32, device=dev)
    a, b = ptr(z), ptr(f)
    call = eng._lib.mpx_dwconv3x3_bn_relu6
    assert call(eng._h, a, a, b, b, b, a, a, 1, 4, 8, 1, 1, None) == 0
    torch.cuda.synchronize()
    assert call(eng._h, None, a, b, b, b, a, a, 1, 4, 8, 1, 1, None) == -1             # null planes
    assert call(eng._h, a, a, None, b, b, a, a, 1, 4, 8, 1, 1, None) == -1             # null weights
    assert call(eng._h, a, a, b, b, b, a, a, 0, 4, 8, 1, 1, None) == -1                # empty batch
    assert call(eng._h, a, a, b, b, b, a, a, 1, 0, 8, 1, 1, None) == -1                # empty map
    assert call(eng._h, a, a, b, b, b, a, a, 1, 4, 12, 1, 1, None) == -1               # pitch % 8
    assert call(eng._h, a, a, b, b, b, a, a, 1, 4, 8, 3, 1, None) == -1                # stride
    assert call(eng._h, C.c_void_p(z.data_ptr() + 2), a, b, b, b, a, a, 1, 4, 8, 1, 1, None) == -1      # misaligned


# ------------------------------------------------------------------------------------------------
# clamped global average pool
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,c,batch", [(49, 1280, 3), (49, 16, 5), (49, 1280, 67)])
def test_clamped_global_pool_against_fp64(small_engine, dev, hw, c, batch):
    eng = small_engine
    g = torch.Generator().manual_seed(hw + c)
    x = torch.randn(batch, hw, c, generator=g) * 4.0                     # a quarter of the values above 6 or below -6
    x[..., : c // 4] *= 1e-3
    xh, xl = split(x.to(dev))
    oh = torch.full((batch * c + 64,), float("nan"), dtype=torch.float16, device=dev)
    ol = torch.full_like(oh, float("nan"))
    _lib.check(eng._h, eng._lib.mpx_global_avgpool_clamp6(eng._h, ptr(xh), ptr(xl), ptr(oh), ptr(ol), batch, hw, c, eng._stream()), "mpx_global_avgpool_clamp6")
    torch.cuda.synchronize()
    assert torch.isnan(oh[batch * c:]).all() and torch.isnan(ol[batch * c:]).all()
    x64 = merge(xh, xl).double()
    assert (x64 > 6).any()
    cl = x64.clamp_max(6.0)
    want = cl.mean(1)
    tol = (hw * 2.0 ** -24 + 2.0 ** -22) * cl.abs().mean(1) + 2.0 ** -24
    got = merge(oh[: batch * c].view(batch, c), ol[: batch * c].view(batch, c)).double()
    err = (got - want).abs()
    print("clamped pool %d x %d batch %d: max err %.3e, worst err / bound %.3f; without the clamp the mean would move by %.3f"
          % (hw, c, batch, err.max().item(), (err / tol).max().item(), (x64.mean(1) - want).abs().max().item()))
    assert not torch.isnan(got).any() and (err <= tol).all()
    # the unclamped pool of the same planes is a different number: the clamp is what was tested
    assert (x64.mean(1) - want).abs().max().item() > 0.01
    z = ptr(xh)
    assert eng._lib.mpx_global_avgpool_clamp6(eng._h, z, z, z, z, 1, 49, 12, None) == -1
    assert eng._lib.mpx_global_avgpool_clamp6(eng._h, z, z, z, z, 0, 49, 16, None) == -1
    assert eng._lib.mpx_global_avgpool_clamp6(eng._h, None, z, z, z, 1, 49, 16, None) == -1


# ------------------------------------------------------------------------------------------------
# per conv layer
# ------------------------------------------------------------------------------------------------
def _ref_layer(sd, d, x64, res64):
    """fp64 conv + BatchNorm (+ residual) (+ ReLU -- not ReLU6: the clamp belongs to the consumer) on the device: [B][cout][ho][ho]."""
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
    return F.relu(y) if d.relu else y


def _check(eng, sd, i, batch, tile=-1):
    d = eng.layers[i]
    fields = "%d->%d k%d h%d K %d res %d " % (d.cin, d.cout, d.ksize, d.hin, d.k_packed, d.residual)
    return check_conv_layer(eng, i, batch, lambda d, x64, r64: _ref_layer(sd, d, x64, r64), tile, pitched=True, fields=fields)[0]


def test_every_distinct_conv_shape_on_every_accepted_tile(small_engine, sd):
    """Every distinct (cin, cout, ksize, hin, residual) of the network at batch 3 on every tile it accepts: the stem (3x3 stride 2 pad 1 on
    the NHWC4 staging), the K = 32 layers (one K step), the padded layers (16, 24, 144 channels), project layers with and without their
    residual, features.18 and the classifier.  features.18 -- the one layer the 256-row tiles accept -- runs a second batch large enough
    for tile 9's and tile 10's own kernels."""
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
            batches = (3, 171) if (d.cout == 1280 and (t == default or t in FALLBACK)) else (3,)
            for batch in batches:
                ran = _check(eng, sd, i, batch, tile=t)
                assert ran & ((1 << t) | (1 << FALLBACK.get(t, t))), (d.name, t, ran)
                if t not in FALLBACK:
                    assert ran == 1 << t, (d.name, t, ran)
                if d.cout == 1280 and batch == 171 and t in (9, 10):
                    assert ran & (1 << t), (d.name, t, ran)                 # the kernel itself ran on K = 320
        count += 1
    print("distinct conv shapes checked: %d (K = 32: %d, padded: %d, with a residual: %d)" % (count, one_step, padded, with_res))
    assert count >= 20 and one_step >= 3 and padded >= 5 and with_res >= 5


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
def test_mobilenet_end_to_end(engine, sd, golden_dir):
    """Logits lens (tests/logits_lens.py): all 1000 logits of every row against fp64, bound 4 d_L with d_L = the fp32 CPU loop's distance.  Measured on one MI355X: mobilenet_v2 d_L 1.55e-05, engine 1.61e-05 (1.03)."""
    ref = Reference(mobilenet_ref, sd)
    check_end_to_end(engine, ARCH, ref, e2e_rows(ref, mobilenet_ref.E2E_CASES, golden_dir),
                     "%(arch)s: yardstick distance %(d).3e over the 28 rows -> end-to-end bound %(bound).1e")


def test_a_mask_row_scores_the_same_bits_wherever_it_sits(engine, golden_dir):
    check_position_independence(engine, *mobilenet_ref.e2e_inputs(golden_dir, "felz"), (8, ((1, 0, (0,)), (37, 41, (0, 5, 36)), (700, 44, (3, 511, 512, 699)))))


# ------------------------------------------------------------------------------------------------
# API and errors
# ------------------------------------------------------------------------------------------------
def test_api_on_a_mobilenet_engine(engine, sd, golden_dir):
    check_api(engine, Reference(mobilenet_ref, sd), *mobilenet_ref.e2e_inputs(golden_dir, "felz"))


def test_profile_lists_the_depthwise_launches(engine, dev):
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
    assert len(prof["per_dw_ms"]) == len(eng.dwconvs) == 17 and all(ms > 0 for ms in prof["per_dw_ms"])
    assert prof["per_norm_ms"] == [] and prof["avgpool2_ms"] == 0
    assert prof["launches"]["pool"] == 17 + 1               # every depthwise layer and the clamped global pool
    assert prof["launches"]["conv"] == len(eng.layers) == 36


def test_mobilenet_error_paths(small_engine, mpx_lib, dev, sd):
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
    for bad in (6000, 6001, 6003, 6999):
        h = C.c_void_p()
        assert mpx_lib.mpx_create(bad, 2, 0, C.byref(h)) == -1 and not h.value
    dd = _lib.DwConvDesc()
    assert eng._lib.mpx_dwconv_info(eng._h, 17, C.byref(dd)) == -1 and eng._lib.mpx_dwconv_info(eng._h, -1, C.byref(dd)) == -1
    v = torch.ones(1024)
    vp = C.c_void_p(v.data_ptr())
    assert eng._lib.mpx_load_dwconv(eng._h, 17, vp, vp, vp, vp, vp, EPS) == -1
    assert eng._lib.mpx_load_dwconv(eng._h, 0, vp, None, vp, vp, vp, EPS) == -1
    fresh = MaskedForwardEngine(ARCH, max_batch=2, device=0)
    try:
        assert len(fresh.dwconvs) == 17
        fresh.load_state_dict(sd, only=[d.name.decode() for d in fresh.layers])      # every conv, none of the depthwise layers
        assert fresh._lib.mpx_weights_complete(fresh._h) == 0
        fresh.stage_masks(im, z, on, 0)
        labels = torch.zeros(1, dtype=torch.int32, device=dev)
        score = torch.zeros(1, device=dev)
        pred = torch.zeros(1, dtype=torch.int32, device=dev)
        assert fresh._lib.mpx_forward(fresh._h, ptr(labels), ptr(score), ptr(pred), None, 1, None) == -2
        with pytest.raises(KeyError):
            fresh.load_state_dict(synth.make_state_dict("resnet18"))
        with pytest.raises(KeyError):
            fresh.load_state_dict(sd, only=["features.2.conv.1.9"])
        fresh.load_state_dict(sd, only=[d.name.decode() for d in fresh.dwconvs])
        assert fresh._lib.mpx_weights_complete(fresh._h) == 1
    finally:
        fresh.close()
    # a ResNet engine has no depthwise layers
    r = MaskedForwardEngine("resnet18", max_batch=2, device=0)
    try:
        assert r._lib.mpx_num_dwconvs(r._h) == 0 and r.dwconvs == []
    finally:
        r.close()
