"""DenseNet-121 / 169 / 201 on the MI355X (pytest -m gpu), through the C-ABI as tests/test_gpu_alexnet.py does: the topology and the
default tile of every layer, every distinct conv shape on every tile it accepts against an fp64 conv + BatchNorm of the same split
inputs, the concat-append + BN + ReLU kernel and the 2x2 average pool against fp64 with bounds derived from their roundings, the whole
networks against the batch-1 fp32 CPU loop and the fp64 restatement (tests/densenet_ref.py), position independence of a mask row, the
reference-named API and the error paths.

Bounds.  Per layer: 4e-6 of max(|want|, 1), the project's per-layer bound.  Concat-append + BN + ReLU, per element:
|err| <= 2^-20 (|scale x| + |shift|) + 2^-24 -- scale and shift rounded to fp32, one multiply, one add (2^-24 each) and the re-split
(2^-22) sum to 2^-21 of that magnitude, the bound is twice that, and lo's fp16 subnormal step is the absolute floor.  Average pool:
2^-21 max|x_i| + 2^-24 (three fp32 adds and the re-split stay under 2^-22 + 3 * 2^-24).  End to end: 2e-5 on a score against the batch-1
fp32 CPU loop and against fp64 (the project's end-to-end bound; 1e-4 is the tolerance), and the same argmax on EVERY row
(tests/test_densenet_cpu.py asserts a top-two fp64 margin >= 1e-3 on exactly these rows).

End-to-end figures measured on one MI355X (rows of densenet_ref.E2E_CASES: 20 felzenszwalb + 8 grid masks per network), max |d| of a score,
felzenszwalb / grid; the fp32-loop-versus-fp64 distance is the yardstick:
                    engine vs fp64        fp32 CPU loop vs fp64    engine vs fp32 CPU loop    smallest fp64 top-two margin
    densenet121     8.4e-07 / 1.2e-06     5.0e-07 / 5.0e-07        9.8e-07 / 1.1e-06          0.48 / 1.74
    densenet169     2.8e-07 / 5.2e-07     2.0e-07 / 1.8e-07        4.0e-07 / 6.8e-07          0.37 / 0.13
    densenet201     2.2e-07 / 2.7e-07     2.3e-07 / 1.4e-07        1.6e-07 / 3.8e-07          0.0049 / 0.012"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import densenet_ref
from gpu_common import accepted_tiles, dev, FALLBACK, merge, ptr, SCORE_BOUND, SCORE_TOL, split  # noqa: F401  (dev is a fixture)
from net_harness import check_api, check_conv_layer, check_position_independence, Reference
from network_interpretation_imagenet_amd import _lib, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine
from logits_lens import LogitsLens
from oracle import scorer

pytestmark = pytest.mark.gpu

ARCHS = ("densenet121", "densenet169", "densenet201")
MACS = {"densenet121": 2834161664, "densenet169": 3359843328, "densenet201": 4291365888}
EPS = 1e-5


@pytest.fixture(scope="module")
def small_engines(mpx_lib, dev):
    """One engine per architecture with a small workspace, for everything that hands the kernels device pointers of its own."""
    engines = {}

    def get(arch):
        if arch not in engines:
            engines[arch] = MaskedForwardEngine(arch, max_batch=8, device=0).load_state_dict(synth.make_state_dict(arch))
        return engines[arch]

    yield get
    for e in engines.values():
        e.close()


def _expected_default_tile(d):
    """The unchanged default_tile rules, spelled out for the DenseNet shapes -- and conv2's own default, which the topology sets."""
    if d.cout == 32:
        return 6                                    # every conv2 (3x3, 128 -> 32): the patch kernel, this topology's own default
    if d.cout <= 64:
        return 1                                    # the stem
    if d.cout > d.cin:
        return 7                                    # conv1 of the first layers of block 1 (K = 64, 96): an expanding 1x1
    if d.cout % 256 == 0 and d.cin % 64 == 0:
        return 13                                   # transition2 / transition3 of densenet121
    return 2


# ------------------------------------------------------------------------------------------------
# topology
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ARCHS)
def test_densenet_topology_and_default_tiles(small_engines, arch):
    eng = small_engines(arch)
    convs, norms = densenet_ref.topology(arch)
    assert [d.name.decode() for d in eng.layers] == [c[0] for c in convs]
    assert [(d.cin, d.cout, d.ksize, d.stride, d.pad, d.hin, d.hout, d.relu) for d in eng.layers] == [c[1:] for c in convs]
    for d in eng.layers:
        name = d.name.decode()
        want_bn = "features.norm0" if name == "features.conv0" else (name[:-5] + "norm2" if name.endswith(".conv1") else "")
        assert d.bn_name.decode() == want_bn and d.residual == 0 and d.cout_pad == -(-d.cout // 128) * 128
        assert d.k_packed == (224 if d.cin == 3 else d.ksize * d.ksize * d.cin)
    assert [(n.name.decode(), n.channels, n.hw) for n in eng.norms] == norms
    assert eng.flops_per_forward == 2.0 * MACS[arch]
    geo = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert eng._lib.mpx_geometry(eng._h, *[C.byref(v) for v in geo]) == 0 and [v.value for v in geo] == [224, 3, 1000, 1000]
    tiles = [eng._lib.mpx_get_conv_tile(eng._h, i) for i in range(len(eng.layers))]
    by_shape = {}
    for d, t in zip(eng.layers, tiles):
        assert t == _expected_default_tile(d), (d.name, t)
        by_shape.setdefault((d.ksize, d.hout, t), []).append(d.cin)
    print(arch, "default tiles (ksize, hout, tile) -> cin range:", {k: (min(v), max(v), len(v)) for k, v in sorted(by_shape.items())})
    assert eng.stem == "conv" and not eng.has_stem_table and eng._lib.mpx_weights_complete(eng._h) == 1
    assert eng._lib.mpx_num_bottleneck_tails(eng._h) == 0


def test_densenet_default_max_batch_and_workspace(mpx_lib, dev):
    eng = MaskedForwardEngine("densenet121", device=0)
    try:
        assert eng.max_batch == 512
        # per slot: four 56x56x256 split-fp16 buffers, the NHWC4 staging, the pooled stem planes: 14.5 MB, a ResNet slot
        per_slot = 4 * 2 * 56 * 56 * 256 * 2 + 2 * 230 * 230 * 4 * 2 + 2 * 56 * 56 * 64 * 2
        w = sum(2 * d.cout_pad * d.k_packed * 2 for d in eng.layers)
        assert per_slot * 512 + w < eng.workspace_bytes < per_slot * 512 + w + (16 << 20)
        print("densenet121: %.2f MB per slot, workspace %.2f GB at max_batch 512" % (per_slot / 1e6, eng.workspace_bytes / 1e9))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------
# per layer
# ------------------------------------------------------------------------------------------------
def _ref_layer(sd, d, x_nchw64):
    """fp64 conv (+ BatchNorm from gamma, beta, mean, var) (+ ReLU) on the device, as an im2col GEMM: [B][cout][ho][ho]."""
    name, bn = d.name.decode(), d.bn_name.decode()
    dev = x_nchw64.device
    w = sd[name + ".weight"].double().reshape(d.cout, -1).to(dev)
    out = []
    for i in range(x_nchw64.shape[0]):
        cols = F.unfold(x_nchw64[i:i + 1], d.ksize, padding=d.pad, stride=d.stride)[0]     # [cin*k*k, L], (ci, ky, kx) like the OIHW rows
        out.append((w @ cols).view(1, d.cout, d.hout, d.hout))
    y = torch.cat(out)
    if bn:
        g, b, m, v = (sd["%s.%s" % (bn, k)].double().to(dev)[None, :, None, None] for k in ("weight", "bias", "running_mean", "running_var"))
        y = (y - m) / torch.sqrt(v + EPS) * g + b
    elif name == "classifier":
        y = y + sd["classifier.bias"].double().to(dev)[None, :, None, None]
    return F.relu(y) if d.relu else y


def _check(eng, sd, i, batch, tile=-1):
    d = eng.layers[i]
    fields = "%d->%d k%d h%d " % (d.cin, d.cout, d.ksize, d.hin)
    return check_conv_layer(eng, i, batch, lambda d, x64, _r64: _ref_layer(sd, d, x64), tile, fields=fields)[0]


def _distinct_shapes(eng, seen):
    """Layer indices of the conv shapes (cin, cout, ksize, hin) not in `seen`, first occurrence each; adds them to `seen`."""
    out = []
    for i, d in enumerate(eng.layers):
        key = (d.cin, d.cout, d.ksize, d.hin)
        if key not in seen:
            seen.add(key)
            out.append(i)
    return out


def _layer_batches(d):
    """A handful of images, and a batch whose tiles pass one round of a persistent / 256x256 kernel on 256 CUs (the transitions with
    cout % 256 == 0: 28x28 maps from 84 images, 14x14 maps with two cout tiles from 168) and do not fill a whole number of rounds."""
    if d.ksize == 1 and d.cout % 256 == 0 and d.hin > 1:
        return (3, 171)
    return (3, 37) if d.hin >= 28 else (3, 67)


def test_every_distinct_conv_shape_on_every_accepted_tile(small_engines):
    """All three networks: 106 distinct shapes (conv1 for every C = 64 + 32 k of every map size, K an odd multiple of 32 among them; conv2
    on four maps; the transitions; the stem; the classifiers).  Default tile at two batches, every other accepted tile at the small one."""
    seen = set()
    count = 0
    for arch in ("densenet201", "densenet169", "densenet121"):
        eng = small_engines(arch)
        sd = synth.make_state_dict(arch)
        for i in _distinct_shapes(eng, seen):
            d = eng.layers[i]
            default = eng._lib.mpx_get_conv_tile(eng._h, i)
            accepted = accepted_tiles(eng, i)
            assert default in accepted and {0, 1, 2, 4, 7} <= set(accepted), (d.name, accepted)
            small, large = _layer_batches(d)
            for t in accepted:
                for batch in ((small, large) if t == default or t in FALLBACK else (small,)):
                    if i == 0 and batch > eng.max_batch:
                        batch = eng.max_batch           # the stem reads the engine's own staging
                    ran = _check(eng, sd, i, batch, tile=t)
                    assert ran & ((1 << t) | (1 << FALLBACK.get(t, t))), (d.name, t, ran)
                    if t not in FALLBACK:
                        assert ran == 1 << t, (d.name, t, ran)
                    if t in (9, 13) and batch == large and not d.residual:
                        assert ran & (1 << t), (d.name, t, batch, ran)         # the 256x256 walk itself ran over whole rounds
            count += 1
    print("distinct conv shapes checked:", count)
    assert count >= 100


# ------------------------------------------------------------------------------------------------
# concat-append + BN + ReLU
# ------------------------------------------------------------------------------------------------
def _load_norm(eng, c, seed):
    """Random BatchNorm tensors into the first stand-alone norm of `eng` with `c` channels; -> (k, gamma, beta, mean, var as f64 device
    tensors, scale_ptr, shift_ptr)."""
    k = [n.channels for n in eng.norms].index(c)
    g = torch.Generator().manual_seed(seed)
    gamma = torch.empty(c).uniform_(0.5, 1.5, generator=g) * torch.where(torch.rand(c, generator=g) < 0.1, -1.0, 1.0)
    beta = torch.randn(c, generator=g) * 0.3
    mean = torch.randn(c, generator=g) * 0.3
    var = torch.empty(c).uniform_(0.3, 2.0, generator=g)
    _lib.check(eng._h, eng._lib.mpx_load_norm(eng._h, k, *[C.c_void_p(t.data_ptr()) for t in (gamma, beta, mean, var)], EPS), "mpx_load_norm")
    sc, sh = C.c_void_p(), C.c_void_p()
    assert eng._lib.mpx_norm_params(eng._h, k, C.byref(sc), C.byref(sh)) == 0 and sc.value and sh.value
    return k, [t.double().to(eng.device) for t in (gamma, beta, mean, var)], sc, sh


def _bn_bound_check(got, x64, gamma, beta, mean, var, what):
    """|relu(bn(x)) - got| <= 2^-20 (|scale x| + |shift|) + 2^-24 per element, fp64 BatchNorm from gamma, beta, mean, var."""
    scale = gamma / torch.sqrt(var + EPS)
    shift = beta - mean * scale
    want = F.relu((x64 - mean) / torch.sqrt(var + EPS) * gamma + beta)
    tol = 2.0 ** -20 * ((scale * x64).abs() + shift.abs()) + 2.0 ** -24
    err = (got.double() - want).abs()
    worst = (err / tol).max().item()
    print("%s: max err %.3e, worst err / bound %.3f, out range %.3f" % (what, err.max().item(), worst, want.max().item()))
    assert worst <= 1.0, (what, worst)


CAT_CASES = [
    # hw, batch, c_old, g, c_total, fresh_stride
    (56, 2, 0, 64, 256, 64),          # a block's input becomes the head of the concatenation
    (56, 1, 64, 32, 256, 32),         # C = 96: an odd multiple of 32
    (28, 3, 128, 32, 512, 32),
    (14, 5, 960, 32, 1024, 32),       # C = 992
    (14, 2, 256, 32, 1024, 128),      # a channel-strided source: the fresh channels are the head of wider pixels
    (7, 9, 512, 32, 1024, 32),
    (7, 1, 992, 32, 1024, 64),        # C = 1024 = c_total: the last layer of a block
    (1, 3, 32, 32, 96, 32),           # 3 pixels x 8 units: less than one wave
]


@pytest.mark.parametrize("hw,batch,c_old,g,c_total,fstride", CAT_CASES)
def test_concat_append_bn_relu(small_engines, dev, hw, batch, c_old, g, c_total, fstride):
    eng = small_engines("densenet121")
    sd = synth.make_state_dict("densenet121")
    npix, c = batch * hw * hw, c_old + g
    gen = torch.Generator().manual_seed(hw * 1000 + c)
    raw = (torch.randn(npix, c_total, generator=gen) * 2).to(dev)
    raw[:, : c_total // 4] *= 1e-3                                                      # small magnitudes: lo in fp16's subnormals
    fresh = (torch.randn(npix, fstride, generator=gen) * 2).to(dev)
    rh, rl = split(raw)
    fh, fl = split(fresh)
    rh0, rl0 = rh.clone(), rl.clone()
    guard = 64
    oh = torch.full((npix * c + guard,), float("nan"), dtype=torch.float16, device=dev)
    ol = torch.full_like(oh, float("nan"))
    k, (gamma, beta, mean, var), sc, sh = _load_norm(eng, c, seed=c)
    try:
        rc = eng._lib.mpx_concat_bn_relu(eng._h, ptr(fh), ptr(fl), g, fstride, ptr(rh), ptr(rl), c_total, c_old, sc, sh, ptr(oh), ptr(ol), c, npix, eng._stream())
        _lib.check(eng._h, rc, "mpx_concat_bn_relu")
        torch.cuda.synchronize()
        # the append: bit for bit, and nothing else of the concatenation touched
        assert torch.equal(rh[:, c_old:c].view(torch.int16), fh[:, :g].view(torch.int16)) and torch.equal(rl[:, c_old:c].view(torch.int16), fl[:, :g].view(torch.int16))
        keep = torch.ones(c_total, dtype=torch.bool, device=dev)
        keep[c_old:c] = False
        assert torch.equal(rh[:, keep].view(torch.int16), rh0[:, keep].view(torch.int16)) and torch.equal(rl[:, keep].view(torch.int16), rl0[:, keep].view(torch.int16))
        assert torch.isnan(oh[npix * c:]).all() and torch.isnan(ol[npix * c:]).all()          # nothing behind the dense operand
        x64 = torch.cat([merge(rh0[:, :c_old], rl0[:, :c_old]), merge(fh[:, :g], fl[:, :g])], 1).double()
        got = merge(oh[: npix * c].view(npix, c), ol[: npix * c].view(npix, c))
        assert not torch.isnan(got).any()
        _bn_bound_check(got, x64, gamma, beta, mean, var, "concat+bn+relu hw %d C %d of %d" % (hw, c, c_total))
        # the two-launch form (append only, then normalise only) gives the same bits
        rh2, rl2 = rh0.clone(), rl0.clone()
        oh2 = torch.full_like(oh, float("nan"))
        ol2 = torch.full_like(oh, float("nan"))
        assert eng._lib.mpx_concat_bn_relu(eng._h, ptr(fh), ptr(fl), g, fstride, ptr(rh2), ptr(rl2), c_total, c_old, None, None, None, None, 0, npix, eng._stream()) == 0
        assert eng._lib.mpx_concat_bn_relu(eng._h, None, None, 0, 0, ptr(rh2), ptr(rl2), c_total, 0, sc, sh, ptr(oh2), ptr(ol2), c, npix, eng._stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(rh2.view(torch.int16), rh.view(torch.int16)) and torch.equal(rl2.view(torch.int16), rl.view(torch.int16))
        assert torch.equal(oh2[: npix * c].view(torch.int16), oh[: npix * c].view(torch.int16)) and torch.equal(ol2[: npix * c].view(torch.int16), ol[: npix * c].view(torch.int16))
    finally:
        name = eng.norms[k].name.decode()
        t = [sd["%s.%s" % (name, key)] for key in ("weight", "bias", "running_mean", "running_var")]
        eng._lib.mpx_load_norm(eng._h, k, *[C.c_void_p(v.data_ptr()) for v in t], EPS)      # the engine's own statistics again


def test_concat_append_bn_relu_refuses_bad_arguments(small_engines, dev):
    eng = small_engines("densenet121")
    z = torch.zeros(4096, dtype=torch.float16, device=dev)
    f = torch.zeros(1024, dtype=torch.float32, device=dev)
    a = ptr(z)
    call = eng._lib.mpx_concat_bn_relu
    assert call(eng._h, a, a, 32, 32, a, a, 64, 32, ptr(f), ptr(f), a, a, 64, 4, None) == 0
    torch.cuda.synchronize()
    assert call(eng._h, a, a, 32, 32, None, None, 64, 32, ptr(f), ptr(f), a, a, 64, 4, None) == -1        # no raw planes
    assert call(eng._h, a, a, 12, 32, a, a, 64, 32, ptr(f), ptr(f), a, a, 44, 4, None) == -1              # g % 8
    assert call(eng._h, a, a, 32, 32, a, a, 64, 48, ptr(f), ptr(f), a, a, 80, 4, None) == -1              # c_old + g > c_total
    assert call(eng._h, a, a, 32, 16, a, a, 64, 32, ptr(f), ptr(f), a, a, 64, 4, None) == -1              # fresh_stride < g
    assert call(eng._h, a, a, 32, 32, a, a, 64, 32, ptr(f), ptr(f), a, a, 32, 4, None) == -1              # c_norm != c_old + g
    assert call(eng._h, a, a, 32, 32, a, a, 64, 32, None, None, a, a, 64, 4, None) == -1                # out planes without scale / shift
    assert call(eng._h, a, a, 32, 32, a, a, 64, 32, ptr(f), ptr(f), a, a, 64, 0, None) == -1              # no pixels
    assert call(eng._h, None, None, 0, 0, a, a, 64, 0, None, None, None, None, 0, 4, None) == -1        # nothing to do
    assert call(eng._h, C.c_void_p(z.data_ptr() + 2), a, 32, 32, a, a, 64, 32, ptr(f), ptr(f), a, a, 64, 4, None) == -1      # misaligned


def test_concat_append_bn_relu_planes_past_2_31_elements(small_engines, dev):
    """2,200,000 pixels of a 1024-channel concatenation: 2.25e9 elements per plane, so raw and output offsets pass 2^31 (9 GB of raw planes,
    9 GB of output planes, allocated and freed here).  Not canonical splits: any (hi, lo) pair is a value."""
    eng = small_engines("densenet121")
    sd = synth.make_state_dict("densenet121")
    npix, c_total, c_old, g = 2200000, 1024, 992, 32
    assert npix * c_total > 2 ** 31
    gen = torch.Generator(device=dev).manual_seed(9)
    rh = torch.empty(npix, c_total, dtype=torch.float16, device=dev)
    rl = torch.empty_like(rh)
    step = 200000
    for lo in range(0, npix, step):
        rh[lo:lo + step] = (torch.randn(rh[lo:lo + step].shape, generator=gen, device=dev) * 2).half()
        rl[lo:lo + step] = (torch.randn(rl[lo:lo + step].shape, generator=gen, device=dev) * 1e-3).half()
    fh = (torch.randn(npix, g, generator=gen, device=dev) * 2).half()
    fl = (torch.randn(npix, g, generator=gen, device=dev) * 1e-3).half()
    oh = torch.full((npix, c_total), float("nan"), dtype=torch.float16, device=dev)
    ol = torch.full_like(oh, float("nan"))
    k, (gamma, beta, mean, var), sc, sh = _load_norm(eng, c_total, seed=1)
    try:
        tail_h, tail_l = rh[-1000:, :c_old].clone(), rl[-1000:, :c_old].clone()
        rc = eng._lib.mpx_concat_bn_relu(eng._h, ptr(fh), ptr(fl), g, g, ptr(rh), ptr(rl), c_total, c_old, sc, sh, ptr(oh), ptr(ol), c_total, npix, eng._stream())
        _lib.check(eng._h, rc, "mpx_concat_bn_relu")
        torch.cuda.synchronize()
        assert torch.equal(rh[:, c_old:].view(torch.int16), fh.view(torch.int16)) and torch.equal(rl[:, c_old:].view(torch.int16), fl.view(torch.int16))
        assert torch.equal(rh[-1000:, :c_old].view(torch.int16), tail_h.view(torch.int16)) and torch.equal(rl[-1000:, :c_old].view(torch.int16), tail_l.view(torch.int16))
        for lo in (0, 1000000, 2097152 - 500, npix - 1000):          # 2097152 x 1024 = 2^31: the pixels on both sides of it, and the last ones
            x64 = merge(rh[lo:lo + 1000], rl[lo:lo + 1000]).double()
            _bn_bound_check(merge(oh[lo:lo + 1000], ol[lo:lo + 1000]), x64, gamma, beta, mean, var, "pixels %d.." % lo)
    finally:
        del rh, rl, oh, ol, fh, fl
        torch.cuda.empty_cache()
        name = eng.norms[k].name.decode()
        t = [sd["%s.%s" % (name, key)] for key in ("weight", "bias", "running_mean", "running_var")]
        eng._lib.mpx_load_norm(eng._h, k, *[C.c_void_p(v.data_ptr()) for v in t], EPS)


# ------------------------------------------------------------------------------------------------
# 2x2 stride-2 average pool
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hin,c,batch", [(56, 128, 3), (28, 256, 5), (14, 512, 41), (14, 896, 2), (14, 640, 1), (2, 8, 1)])
def test_avgpool2x2s2_against_fp64(small_engines, dev, hin, c, batch):
    eng = small_engines("densenet121")
    ho = hin // 2
    g = torch.Generator().manual_seed(hin + c)
    x = torch.randn(batch, hin, hin, c, generator=g) * 3
    x[..., : c // 4] *= 1e-3
    xh, xl = split(x.to(dev))
    oh = torch.full((batch, ho, ho, c), float("nan"), dtype=torch.float16, device=dev)
    ol = torch.full_like(oh, float("nan"))
    _lib.check(eng._h, eng._lib.mpx_avgpool2x2s2(eng._h, ptr(xh), ptr(xl), ptr(oh), ptr(ol), batch, hin, c, eng._stream()), "mpx_avgpool2x2s2")
    torch.cuda.synchronize()
    x64 = merge(xh, xl).double().permute(0, 3, 1, 2)
    want = F.avg_pool2d(x64, 2, 2).permute(0, 2, 3, 1)
    mx = F.max_pool2d(x64.abs(), 2, 2).permute(0, 2, 3, 1)
    err = (merge(oh, ol).double() - want).abs()
    tol = 2.0 ** -21 * mx + 2.0 ** -24
    print("avgpool %dx%dx%d: max err %.3e, worst err / bound %.3f" % (hin, hin, c, err.max().item(), (err / tol).max().item()))
    assert not torch.isnan(merge(oh, ol)).any() and (err <= tol).all()


def test_avgpool2x2s2_refuses_bad_shapes(small_engines, dev):
    eng = small_engines("densenet121")
    z = torch.zeros(4096, dtype=torch.float16, device=dev)
    args = (ptr(z), ptr(z), ptr(z), ptr(z))
    assert eng._lib.mpx_avgpool2x2s2(eng._h, *args, 1, 7, 8, None) == -1       # odd
    assert eng._lib.mpx_avgpool2x2s2(eng._h, *args, 1, 0, 8, None) == -1       # zero extent
    assert eng._lib.mpx_avgpool2x2s2(eng._h, *args, 0, 8, 8, None) == -1       # empty batch
    assert eng._lib.mpx_avgpool2x2s2(eng._h, *args, 1, 8, 12, None) == -1      # c % 8
    assert eng._lib.mpx_avgpool2x2s2(eng._h, *args, 1, 8, 0, None) == -1


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ARCHS)
def test_densenet_end_to_end(mpx_lib, dev, golden_dir, arch):
    """Logits lens (tests/logits_lens.py): all 1000 logits of every row against fp64, bound 4 d_L with d_L = the fp32 CPU loop's distance.  Measured on one MI355X: densenet121 d_L 3.99e-06, engine 6.51e-06 (1.63); densenet169 d_L 4.18e-06, engine 9.63e-06 (2.30);
    densenet201 d_L 5.42e-06, engine 9.94e-06 (1.83)."""
    lens = LogitsLens(arch)
    sd = synth.make_state_dict(arch)
    eng = MaskedForwardEngine(arch, device=0).load_state_dict(sd)          # the default max_batch
    try:
        assert eng.max_batch == 512
        for kind, m, seed in densenet_ref.E2E_CASES:
            img, seg = densenet_ref.e2e_inputs(golden_dir, kind)
            x = scorer.to_tensor_normalize(img)
            label, prob = densenet_ref.predict(sd, arch, x)
            assert 0.05 <= prob.max() <= 0.85
            S = len(np.unique(seg))
            onoff = synth.random_onoff(m, S, seed=seed)
            _o, score, pred, logits = eng.score_masks(img, seg, onoff, label, return_logits=True)
            ref_score, ref_pred, ref_logits = densenet_ref.score_masks_reference_loop(sd, arch, x, seg, onoff, label, return_logits=True)
            s64, logits64 = densenet_ref.score_masks_fp64(sd, arch, x, seg, onoff, label)
            lens.add(kind, logits, ref_logits, logits64)
            top2 = np.sort(logits64, axis=1)[:, -2:]
            gap = top2[:, 1] - top2[:, 0]
            err_engine = float(np.abs(score.astype(np.float64) - s64).max())
            err_cpu = float(np.abs(ref_score.astype(np.float64) - s64).max())
            err_both = float(np.abs(score.astype(np.float64) - ref_score.astype(np.float64)).max())
            print("%s %s: %d masks, S %d, label %d, scores %.4f..%.4f" % (arch, kind, m, S, label, ref_score.min(), ref_score.max()))
            print("%s %s: max|d| engine vs fp64 %.3e, fp32 CPU loop vs fp64 (the yardstick) %.3e, engine vs fp32 CPU loop %.3e, smallest fp64 logit gap %.4f"
                  % (arch, kind, err_engine, err_cpu, err_both, gap.min()))
            assert err_both <= SCORE_TOL and err_engine <= SCORE_TOL
            assert err_both <= SCORE_BOUND and err_engine <= SCORE_BOUND
            assert gap.min() >= 1e-3
            assert (pred == logits64.argmax(1)).all() and (pred == ref_pred).all()         # every row
            p_label, _ = eng.predict(img)
            assert p_label == label
        lens.check()
    finally:
        eng.close()


@pytest.fixture(scope="module")
def eng121(mpx_lib, dev):
    e = MaskedForwardEngine("densenet121", device=0).load_state_dict(synth.make_state_dict("densenet121"))
    yield e
    e.close()


def test_a_mask_row_scores_the_same_bits_wherever_it_sits(eng121, golden_dir):
    check_position_independence(eng121, *densenet_ref.e2e_inputs(golden_dir, "felz"),
                                (8, ((1, 0, (0,)), (37, 41, (0, 5, 36)), (512, 43, (0, 255, 511)), (700, 44, (3, 511, 512, 699)))))


# ------------------------------------------------------------------------------------------------
# API and errors
# ------------------------------------------------------------------------------------------------
def test_api_on_a_densenet_engine(eng121, golden_dir):
    ref = Reference(densenet_ref, synth.make_state_dict("densenet121"), "densenet121")
    check_api(eng121, ref, *densenet_ref.e2e_inputs(golden_dir, "felz"), predict=False)


def test_profile_lists_the_new_ops(eng121, dev):
    eng = eng121
    img = torch.from_numpy(synth.make_images(1, kind="noise")[0]).to(dev)
    seg = torch.from_numpy(synth.grid_segments()).to(dev)
    onoff = torch.from_numpy(synth.random_onoff(4, 196)).to(dev)
    labels = torch.zeros(4, dtype=torch.int32, device=dev)
    eng.profile(True)
    eng.stage_masks(img, seg, onoff, 0)
    eng.forward(4, labels)
    eng.profile(False)
    prof = eng.collect_profile()
    assert len(prof["per_norm_ms"]) == len(eng.norms) == 62 and all(ms > 0 for ms in prof["per_norm_ms"])
    assert prof["avgpool2_ms"] > 0
    assert prof["launches"]["pool"] == 62 + 3 + 1          # every norm, three transitions' pools, the global average pool
    assert prof["launches"]["conv"] == len(eng.layers)      # the stem + max pool is one launch booked on layer 0


def test_densenet_error_paths(small_engines, mpx_lib, dev):
    eng = small_engines("densenet121")
    with pytest.raises(ValueError):
        MaskedForwardEngine("densenet121", max_batch=2, device=0, stem="table")
    with pytest.raises(ValueError):
        eng.score_masks(synth.make_images(1)[0], synth.grid_segments(), synth.random_onoff(2, 196), 0, stem="table")
    z = torch.zeros(224, 224, dtype=torch.int32, device=dev)
    im = torch.zeros(224, 224, 3, dtype=torch.uint8, device=dev)
    on = torch.ones(1, 1, dtype=torch.uint8, device=dev)
    mean = (C.c_float * 3)(*scorer.MEAN)
    std = (C.c_float * 3)(*scorer.STD)
    assert eng._lib.mpx_stem_table_build(eng._h, ptr(im), None, ptr(z), 1, mean, std, None) == -2
    assert eng._lib.mpx_stem_table_apply(eng._h, ptr(on), 1, 1, 0, None) == -2
    for bad in (5000, 5161, 5122, 5999):
        h = C.c_void_p()
        assert mpx_lib.mpx_create(bad, 2, 0, C.byref(h)) == -1 and not h.value
    nd = _lib.NormDesc()
    assert eng._lib.mpx_norm_info(eng._h, len(eng.norms), C.byref(nd)) == -1 and eng._lib.mpx_norm_info(eng._h, -1, C.byref(nd)) == -1
    v = torch.ones(64)
    vp = C.c_void_p(v.data_ptr())
    assert eng._lib.mpx_load_norm(eng._h, len(eng.norms), vp, vp, vp, vp, EPS) == -1
    assert eng._lib.mpx_load_norm(eng._h, 0, vp, None, vp, vp, EPS) == -1
    sd = synth.make_state_dict("densenet121")
    fresh = MaskedForwardEngine("densenet121", max_batch=2, device=0)
    try:
        assert len(fresh.norms) == 62
        fresh.load_state_dict(sd, only=[d.name.decode() for d in fresh.layers])      # every conv, none of the stand-alone norms
        assert fresh._lib.mpx_weights_complete(fresh._h) == 0
        fresh.stage_masks(im, z, on, 0)
        labels = torch.zeros(1, dtype=torch.int32, device=dev)
        score = torch.zeros(1, device=dev)
        pred = torch.zeros(1, dtype=torch.int32, device=dev)
        assert fresh._lib.mpx_forward(fresh._h, ptr(labels), ptr(score), ptr(pred), None, 1, None) == -2
        with pytest.raises(KeyError):
            fresh.load_state_dict(synth.make_state_dict("resnet18"))
        with pytest.raises((KeyError, ValueError)):
            fresh.load_state_dict(synth.make_state_dict("densenet169"))      # denseblock3 has more layers; shapes differ from block 3 on
        fresh.load_state_dict(sd)
        assert fresh._lib.mpx_weights_complete(fresh._h) == 1
    finally:
        fresh.close()
    # a ResNet engine has no stand-alone norms
    r = MaskedForwardEngine("resnet18", max_batch=2, device=0)
    try:
        assert r._lib.mpx_num_norms(r._h) == 0 and r.norms == []
    finally:
        r.close()
