"""The pointwise block tail (csrc/mpx_btail.h, BtPwCfg; mpx_pointwise_tail): layer2's conv3 + identity and the next block's conv1 in
ONE launch.  Shapes are ResNet-50's layer2.1.conv3 + layer2.2.conv1 with synth weights; one image is 784 pixels = 6 tiles of 128
and a 16-pixel ragged tile, so a batch of 3 has tiles that straddle images and ends raggedly too (2352 = 18 * 128 + 48).

Worst values measured on an MI355X (printed by the tests):
    against the fp64 chain:                block output 1.04e-7 / 1.08e-7, next conv1 4.5e-7 / 5.9e-7 at B = 1 / 3
    against the layer-by-layer kernels:    block output 1.08e-7, next conv1 1.9e-7 at B = 169 (1036 tiles on 512 workgroups)
(relative to the tensor's largest value; the bound is 4e-6)
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_common import dev, merge, ptr as _p, split  # noqa: F401  (dev is a fixture)
from network_interpretation_imagenet_amd import _lib, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine

pytestmark = pytest.mark.gpu

KERNEL_TOL = 4e-6       # the project's per-kernel bound (tests/test_gpu_parity.py), relative to max(|reference|, 1)
HW = 28 * 28


def _bits(t):
    return t.view(torch.int16)


@pytest.fixture(scope="module")
def sd50():
    return synth.make_state_dict("resnet50")


@pytest.fixture(scope="module")
def eng50(mpx_lib, dev, sd50):
    e = MaskedForwardEngine("resnet50", max_batch=24, device=0).load_state_dict(sd50)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pair(eng50):
    """(conv3 index, next conv1 index) of layer2.1.conv3 + layer2.2.conv1"""
    names = [d.name.decode() for d in eng50.layers]
    c3, n1 = eng50.pointwise_tails()[0]
    assert names[c3] == "layer2.1.conv3" and names[n1] == "layer2.2.conv1"
    return c3, n1


def _make_inputs(batch, dev, seed):
    g = torch.Generator().manual_seed(seed)
    t2 = torch.randn(batch, 28, 28, 128, generator=g).clamp_min(0) * 1.5
    x = torch.randn(batch, 28, 28, 512, generator=g).clamp_min(0) * 1.5
    return split(t2.to(dev)), split(x.to(dev))


def _run_tail(eng, c3, t, x, batch, sentinel_rows=1):
    """One launch on the first `batch` images of t / x into NaN-filled planes with `sentinel_rows` images behind them."""
    dev = t[0].device
    nan = lambda c: torch.full((batch + sentinel_rows, 28, 28, c), float("nan"), dtype=torch.float16, device=dev)
    oh, ol, zh, zl = nan(512), nan(512), nan(128), nan(128)
    rc = eng._lib.mpx_pointwise_tail(eng._h, c3, _p(t[0]), _p(t[1]), _p(x[0]), _p(x[1]), _p(oh), _p(ol), _p(zh), _p(zl), batch, eng._stream())
    _lib.check(eng._h, rc, "mpx_pointwise_tail")
    torch.cuda.synchronize()
    for q in (oh, ol, zh, zl):
        assert torch.isnan(q[batch:]).all(), "written past M"
        assert not torch.isnan(q[:batch]).any()
    return oh[:batch], ol[:batch], zh[:batch], zl[:batch]


@pytest.fixture(scope="module")
def three(eng50, pair, dev, sd50):
    """Inputs of three images, the launch on all three, and the fp64 chain of the two layers on the same split inputs (the block output
    rounded to hi + lo where the layer-by-layer path stores it) -- computed once, read by the tests below."""
    c3, n1 = pair
    t, x = _make_inputs(3, dev, 7001)
    got = _run_tail(eng50, c3, t, x, 3)

    def conv_bn(d, inp):
        name, bn = d.name.decode(), d.bn_name.decode()
        y = F.conv2d(inp, sd50[name + ".weight"].double(), None, d.stride, d.pad)
        sc = sd50[bn + ".weight"].double() / torch.sqrt(sd50[bn + ".running_var"].double() + 1e-5)
        return (y - sd50[bn + ".running_mean"].double().view(1, -1, 1, 1)) * sc.view(1, -1, 1, 1) + sd50[bn + ".bias"].double().view(1, -1, 1, 1)

    t2u = merge(*t).cpu().double().permute(0, 3, 1, 2)
    xu = merge(*x).cpu().double().permute(0, 3, 1, 2)
    out = F.relu(conv_bn(eng50.layers[c3], t2u) + xu)
    oh, ol = split(out.float())
    z = F.relu(conv_bn(eng50.layers[n1], merge(oh, ol).double()))
    return {"t": t, "x": x, "got": got, "out64": out.permute(0, 2, 3, 1), "z64": z.permute(0, 2, 3, 1)}


def _rel(got, want):
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1.0)


@pytest.mark.parametrize("batch", [1, 3])
def test_pointwise_tail_vs_fp64_chain(eng50, pair, three, batch):
    """relu(bn3(conv3(t2)) + identity) and relu(bn1'(conv1'(out))) against the fp64 chain, each within the per-kernel bound; B = 1 is
    6 tiles + a 16-pixel ragged one, B = 3 has tiles that straddle images.  Nothing is written behind M (sentinel image of NaNs)."""
    if batch == 3:
        oh, ol, zh, zl = three["got"]
    else:
        oh, ol, zh, zl = _run_tail(eng50, pair[0], [q[:1].contiguous() for q in three["t"]], [q[:1].contiguous() for q in three["x"]], 1)
    e_out = _rel(merge(oh, ol).cpu().double(), three["out64"][:batch])
    e_z = _rel(merge(zh, zl).cpu().double(), three["z64"][:batch])
    print("pointwise tail vs fp64 chain, B = %d: block output %.3e, next conv1 %.3e" % (batch, e_out, e_z))
    assert e_out <= KERNEL_TOL and e_z <= KERNEL_TOL


@pytest.mark.parametrize("k", [0, 1, 2])
def test_pointwise_tail_position_independence(eng50, pair, three, k):
    """Image k of the B = 3 call is bit-equal to the same image scored alone: its tiles start at other pixels of it (784 k mod 128 =
    0, 16, 32) and it shares tiles with its neighbours."""
    alone = _run_tail(eng50, pair[0], [q[k:k + 1].contiguous() for q in three["t"]], [q[k:k + 1].contiguous() for q in three["x"]], 1)
    for a, b in zip(alone, three["got"]):
        assert torch.equal(_bits(a[0]), _bits(b[k]))


def test_pointwise_tail_several_tiles_per_workgroup(eng50, pair, dev):
    """The grid is min(2 workgroups per CU, tiles) and workgroup g walks tiles g, g + grid, ...: the smallest B with more than 2 * grid
    tiles whose last tile is ragged gives workgroups with three tiles and a launch that ends raggedly (256 CUs: B = 169, 1036 tiles,
    the last of 16 pixels).  Against the layer-by-layer kernels (mpx_conv_bn_act twice) on the same inputs within the per-kernel bound
    (two summation orders of the same arithmetic), and bit-identical launch to launch."""
    c3, n1 = pair
    grid = 2 * torch.cuda.get_device_properties(dev).multi_processor_count
    batch = next(b for b in range(1, 100000) if -(-b * HW // 128) > 2 * grid and (b * HW) % 128)
    tiles = -(-batch * HW // 128)
    assert (tiles - 1) // grid + 1 >= 3
    gen = torch.Generator(device="cuda").manual_seed(11)
    mk = lambda c: split(torch.randn(batch, 28, 28, c, device=dev, generator=gen).clamp_min(0) * 1.5)
    t, x = mk(128), mk(512)
    a = _run_tail(eng50, c3, t, x, batch)
    b = _run_tail(eng50, c3, t, x, batch)
    for u, v in zip(a, b):
        assert torch.equal(_bits(u), _bits(v)), "run-to-run difference"
    rh = torch.empty(batch, 28, 28, 512, dtype=torch.float16, device=dev)
    rl, qh = torch.empty_like(rh), torch.empty(batch, 28, 28, 128, dtype=torch.float16, device=dev)
    ql = torch.empty_like(qh)
    _lib.check(eng50._h, eng50._lib.mpx_conv_bn_act(eng50._h, c3, _p(t[0]), _p(t[1]), _p(x[0]), _p(x[1]), _p(rh), _p(rl), None, batch, eng50._stream()), "conv3")
    _lib.check(eng50._h, eng50._lib.mpx_conv_bn_act(eng50._h, n1, _p(rh), _p(rl), None, None, _p(qh), _p(ql), None, batch, eng50._stream()), "conv1")
    torch.cuda.synchronize()
    want_out, want_z = merge(rh, rl), merge(qh, ql)
    e_out = float((merge(a[0], a[1]) - want_out).abs().max() / want_out.abs().max().clamp_min(1.0))
    e_z = float((merge(a[2], a[3]) - want_z).abs().max() / want_z.abs().max().clamp_min(1.0))
    print("pointwise tail vs layer by layer, B = %d (%d tiles on %d workgroups): block output %.3e, next conv1 %.3e" % (batch, tiles, grid, e_out, e_z))
    assert e_out <= KERNEL_TOL and e_z <= KERNEL_TOL


def _scores(eng, n=24, seed=6):
    img = synth.make_images(1, seed=9, kind="noise")[0]
    _o, s, p = eng.score_masks(img, synth.grid_segments(), synth.random_onoff(n, 196, seed=seed), 17)
    return s, p


def test_forward_pointwise_tails_vs_mask_3(eng50):
    """ResNet-50, 24 masks: the default forward against the launch plan without the pointwise tails (mask 3) -- two summation orders of
    the same arithmetic.  A tile override on a pair's conv3 sends THAT pair through its two layers: tile 7 sums in the order of these
    layers' default kernel, so with both pairs overridden the forward is bit-equal to mask 3, and with one it is neither plan."""
    s_pt, p_pt = _scores(eng50)
    eng50.set_fusion(3)
    try:
        s_3, p_3 = _scores(eng50)
    finally:
        eng50.set_fusion(True)
    assert np.abs(s_pt - s_3).max() <= 2e-6 and (p_pt == p_3).all()
    assert not (s_pt == s_3).all()                  # they really are two code paths
    try:
        eng50.set_conv_tile("layer2.1.conv3", 7)
        s_one, p_one = _scores(eng50)
        eng50.set_conv_tile("layer2.2.conv3", 7)
        s_both, _p2 = _scores(eng50)
    finally:
        eng50.set_conv_tile("layer2.1.conv3", -1)
        eng50.set_conv_tile("layer2.2.conv3", -1)
    assert (s_both == s_3).all(), "a pair with a tile override must run the layer-by-layer kernels"
    assert not (s_one == s_pt).all() and not (s_one == s_3).all()       # layer2.1's pair layer by layer, layer2.2's in one launch
    assert np.abs(s_one - s_3).max() <= 2e-6 and (p_one == p_3).all()
    # the conv1 side of a pair: layer2.2.conv1 on another tile takes ITS pair (layer2.1.conv3 + layer2.2.conv1) apart; with layer2.2.conv3 on
    # tile 7 as well both pairs run layer by layer, i.e. mask 3's plan with that one layer on that tile
    assert eng50.conv_tile("layer2.2.conv1") != 7
    try:
        eng50.set_conv_tile("layer2.2.conv1", 7)
        eng50.set_conv_tile("layer2.2.conv3", 7)
        s_c1, _p4 = _scores(eng50)
        eng50.set_conv_tile("layer2.2.conv3", -1)
        eng50.set_fusion(3)
        s_c1_3, _p5 = _scores(eng50)
    finally:
        eng50.set_fusion(True)
        eng50.set_conv_tile("layer2.2.conv1", -1)
        eng50.set_conv_tile("layer2.2.conv3", -1)
    assert (s_c1 == s_c1_3).all(), "a tile override on the pair's conv1 must take the pair apart"
    s_again, _p3 = _scores(eng50)
    assert (s_again == s_pt).all()


@pytest.mark.parametrize("arch,n", [("resnet50", 2), ("resnet101", 2), ("resnet152", 6), ("resnet18", 0), ("vgg11", 0)])
def test_num_pointwise_tails(mpx_lib, dev, arch, n):
    eng = MaskedForwardEngine(arch, max_batch=1, device=0)
    try:
        pairs = eng.pointwise_tails()
        assert eng._lib.mpx_num_pointwise_tails(eng._h) == n and len(pairs) == n
        names = [d.name.decode() for d in eng.layers]
        assert [(names[a], names[b]) for a, b in pairs] == [("layer2.%d.conv3" % k, "layer2.%d.conv1" % (k + 1)) for k in range(1, n + 1)]
        assert eng._lib.mpx_pointwise_tail_info(eng._h, n, None, None) == -1
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["layer2.2.conv1", "layer2.1.conv3"])
def test_reload_is_seen_by_the_pointwise_tail(mpx_lib, dev, sd50, name):
    """The launch reads the packed planes of its two layers: after load_state_dict(only=[one of them]) the fused forward is bit-equal to
    a fresh engine loaded with the new weights, and it differs from before."""
    rng = np.random.default_rng(5)
    sd2 = dict(sd50)
    w = sd50[name + ".weight"]
    sd2[name + ".weight"] = (w * torch.from_numpy(rng.uniform(0.5, 1.5, size=tuple(w.shape)).astype(np.float32))).contiguous()
    eng = MaskedForwardEngine("resnet50", max_batch=12, device=0).load_state_dict(sd50)
    fresh = MaskedForwardEngine("resnet50", max_batch=12, device=0).load_state_dict(sd2)
    try:
        before, _p0 = _scores(eng, 12, 32)
        eng.load_state_dict(sd2, only=[name])
        after, _p1 = _scores(eng, 12, 32)
        want, _p2 = _scores(fresh, 12, 32)
        assert not (after == before).all()
        assert (after == want).all(), "the pointwise tail did not follow the reloaded %s" % name
    finally:
        eng.close()
        fresh.close()


def test_pointwise_tail_argument_errors(eng50, pair, dev):
    lib, h = eng50._lib, eng50._h
    c3 = pair[0]
    bufs = [torch.zeros(HW * c, dtype=torch.float16, device=dev) for c in (128, 128, 512, 512, 512, 512, 128, 128)]
    ptrs = [_p(b) for b in bufs]
    assert lib.mpx_pointwise_tail(h, c3 + 1, *ptrs, 1, None) == -1 and b"pointwise_tail" in lib.mpx_last_error(h)      # not a conv3 of a pair
    assert lib.mpx_pointwise_tail(h, -1, *ptrs, 1, None) == -1 and b"layer -1 is not the conv3" in lib.mpx_last_error(h)
    assert lib.mpx_pointwise_tail(h, c3, *ptrs, 0, None) == -1 and b"empty batch" in lib.mpx_last_error(h)
    for k in range(8):
        q = list(ptrs)
        q[k] = None
        assert lib.mpx_pointwise_tail(h, c3, *q, 1, None) == -1 and b"null planes" in lib.mpx_last_error(h)
    for a, b in ((4, 2), (5, 3), (6, 0), (4, 5), (7, 1)):          # out = x, out_lo = x_lo, next = t2, out_hi = out_lo, next_lo = t2_lo
        q = list(ptrs)
        q[a] = q[b]
        assert lib.mpx_pointwise_tail(h, c3, *q, 1, None) == -1 and b"overlap" in lib.mpx_last_error(h)
    q = list(ptrs)
    q[4] = C.c_void_p(bufs[2].data_ptr() + 256)                     # partial overlap of out_hi with x_hi
    assert lib.mpx_pointwise_tail(h, c3, *q, 1, None) == -1 and b"x_hi and out_hi overlap" in lib.mpx_last_error(h)
    assert lib.mpx_pointwise_tail(h, c3, *ptrs, 1, None) == 0      # distinct buffers: accepted
    torch.cuda.synchronize()
