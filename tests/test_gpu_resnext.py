"""ResNeXt-50 32x4d / ResNeXt-101 32x8d on the GPU (run on the MI355X box: pytest -m gpu): the grouped 3x3 kernel (csrc/mpx_gconv.h, tile 16)
on every distinct grouped shape of both networks behind fences and inside the per-element bound of tests/gconv_draws.py, group isolation
and position independence bit for bit, the dense layers on their default tiles and the conv3 + downsample launches against fp64, the
descriptors, tiles and refusals, and both networks end to end on the rows tests/test_resnext_cpu.py holds the weights to.

The grouped launch does not cap its grid (ceil(M / 16) workgroups in x, a quarter of the channel blocks in y), so there is no capped-grid
case to run."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gconv_draws as gd
import resnext_ref as ref
from gpu_common import dev, Fenced, GENERIC, layer_bound, layer_index, merge, ptr, round_up_one_digit, SCORE_BOUND, SCORE_TOL, split  # noqa: F401  (dev is a fixture)
from logits_lens import LogitsLens
from net_harness import stage_stem_input
from network_interpretation_imagenet_amd import _lib, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine
from oracle import scorer

pytestmark = pytest.mark.gpu

ARCHS = ("resnext50_32x4d", "resnext101_32x8d")
DENSE_TILES = (0, 1, 2, 4, 6, 7, 9, 10, 12, 13, 14)
EPS = 1e-5


@pytest.fixture(scope="module")
def engines(dev):
    """One small engine per network, with its synthetic weights."""
    out = {a: MaskedForwardEngine(a, max_batch=8, device=0).load_state_dict(synth.make_state_dict(a)) for a in ARCHS}
    yield out
    for e in out.values():
        e.close()


def _launch_grouped(eng, d, x_hi, x_lo, batch):
    """mpx_conv_bn_act of grouped layer d over `batch` images -> fenced (hi, lo); the grouped kernel and nothing else must have run."""
    i = layer_index(eng, d.name)
    rows = batch * d.hout * d.hout
    hi, lo = Fenced(rows, d.width, eng.device), Fenced(rows, d.width, eng.device)
    rc = eng._lib.mpx_conv_bn_act(eng._h, i, ptr(x_hi), ptr(x_lo), None, None, ptr(hi.payload), ptr(lo.payload), None, batch, eng._stream())
    _lib.check(eng._h, rc, "mpx_conv_bn_act(%s, batch %d)" % (d.name, batch))
    mask = eng._lib.mpx_last_conv_kernels(eng._h)
    torch.cuda.synchronize()
    assert mask == 1 << gd.TILE, "%s ran kernels %#x" % (d.name, mask)
    for plane, which in ((hi, "hi"), (lo, "lo")):
        assert plane.problems() == [], "%s %s batch %d, %s plane: %s" % (d.arch, d.name, batch, which, "; ".join(plane.problems()))
    return hi, lo


# ------------------------------------------------------------------------------------------------
# 1. every distinct grouped layer of both networks, behind fences, inside the per-element bound
# ------------------------------------------------------------------------------------------------
CASES = gd.all_cases()


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("d", CASES, ids=["%s-%s" % (d.arch, d.name) for d in CASES])
def test_grouped_layer_behind_fences_inside_the_per_element_bound(engines, d, batch):
    """(cg, stride, map) of every grouped layer: 32x4d stride 1 cg 4@56, 8@28, 16@14, 32@7 and stride 2 cg 8@56, 16@28, 32@14; 32x8d the
    same maps with twice the cg.  On the 7 x 7 maps a row is shorter than the MFMA's 16 pixels (a wave's pixels run on into the next rows
    and images); the stride-2 layers read odd windows (the last row's and column's windows hang over the map by the padding alone)."""
    eng = engines[d.arch]
    e = eng.layers[layer_index(eng, d.name)]
    assert (e.cin, e.cout, e.ksize, e.stride, e.pad, e.hin, e.hout, e.relu, e.residual) == (d.width, d.width, 3, d.stride, 1, d.hin, d.hout, 1, 0)
    sd = synth.make_state_dict(d.arch)
    x = gd.draws(d, batch, device=eng.device)
    pre, want, b = (t.reshape(-1, d.width) for t in gd.reference(sd, d, x[2]))
    gd.preconditions(want)
    hi, lo = _launch_grouped(eng, d, x[0], x[1], batch)
    got = hi.payload.double() + lo.payload.double()
    assert not torch.isnan(got).any()
    err, tol = (got - want).abs(), gd.tol(d, b)
    ratio = (err / tol).max().item()
    worst = torch.argmax(err / tol).item()
    print("%s %s cg %d stride %d map %d batch %d: worst err / tol %.3f (pixel row %d, channel %d), C %g; max norm %.2e"
          % (d.arch, d.name, d.cg, d.stride, d.hin, batch, ratio, worst // d.width, worst % d.width, gd.C_TOL[(d.arch, d.name)],
             err.max().item() / max(want.abs().max().item(), 1.0)))
    assert ratio <= 1.0, "%d elements over their bound, worst err / tol %.3f at pixel row %d, channel %d" % (
        int((err > tol).sum()), ratio, worst // d.width, worst % d.width)
    neg = pre < -tol
    assert neg.any() and (hi.payload_bits[neg] == 0).all() and (lo.payload_bits[neg] == 0).all(), "a clearly negative pre-activation is not +0 in both planes"


# ------------------------------------------------------------------------------------------------
# 2. group isolation, bit for bit
# ------------------------------------------------------------------------------------------------
ISOLATION = [("resnext50_32x4d", "layer1.0.conv2"), ("resnext50_32x4d", "layer4.1.conv2")]      # cg = 4 (four groups per MFMA tile), cg = 32


@pytest.mark.parametrize("arch,name", ISOLATION)
def test_changing_one_groups_input_changes_that_groups_output_only(engines, arch, name):
    eng, d = engines[arch], gd.layer(arch, name)
    x_hi, x_lo, _x = gd.draws(d, 2, device=eng.device)
    base_hi, base_lo = _launch_grouped(eng, d, x_hi, x_lo, 2)
    for g in (0, 5, 31):
        y_hi, y_lo = x_hi.clone(), x_lo.clone()
        ch = slice(g * d.cg, (g + 1) * d.cg)
        y_hi[..., ch] = (y_hi[..., ch].float() * -1.5 + 0.25).half()
        y_lo[..., ch] = 0
        hi, lo = _launch_grouped(eng, d, y_hi, y_lo, 2)
        other = torch.ones(d.width, dtype=torch.bool, device=eng.device)
        other[ch] = False
        assert torch.equal(hi.payload_bits[:, other], base_hi.payload_bits[:, other]) and torch.equal(lo.payload_bits[:, other], base_lo.payload_bits[:, other]), \
            "%s: changing the input of group %d changed another group's output" % (name, g)
        assert not torch.equal(hi.payload_bits[:, ch], base_hi.payload_bits[:, ch]), "%s: group %d does not read its own input" % (name, g)


@pytest.mark.parametrize("arch,name", ISOLATION)
def test_weights_in_one_group_alone_give_exact_zeros_elsewhere(engines, arch, name):
    """Non-zero weights in one group, a shift of 0 (beta = running_mean = 0): every other group's output is +0 in both planes, and the
    group's own output is what the reference says."""
    eng, d = engines[arch], gd.layer(arch, name)
    sd = synth.make_state_dict(arch)
    x_hi, x_lo, x = gd.draws(d, 2, device=eng.device)
    try:
        for g in (1, 30):
            ch = slice(g * d.cg, (g + 1) * d.cg)
            mod = dict(sd)
            w = torch.zeros_like(sd[name + ".weight"])
            w[ch] = sd[name + ".weight"][ch]
            mod[name + ".weight"] = w
            mod[d.bn_name + ".bias"] = torch.zeros(d.width)
            mod[d.bn_name + ".running_mean"] = torch.zeros(d.width)
            eng.load_state_dict(mod, only=[name])
            hi, lo = _launch_grouped(eng, d, x_hi, x_lo, 2)
            other = torch.ones(d.width, dtype=torch.bool, device=eng.device)
            other[ch] = False
            assert (hi.payload_bits[:, other] == 0).all() and (lo.payload_bits[:, other] == 0).all(), "%s: group %d's weights reach another group" % (name, g)
            _pre, want, b = (t.reshape(-1, d.width) for t in gd.reference(mod, d, x))
            got = hi.payload.double() + lo.payload.double()
            assert (want[:, ch] > 0).any() and ((got - want).abs() <= gd.tol(d, b)).all()
    finally:
        eng.load_state_dict(sd, only=[name])


# ------------------------------------------------------------------------------------------------
# 3. position independence
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,name", [("resnext50_32x4d", "layer4.1.conv2"), ("resnext50_32x4d", "layer4.0.conv2"), ("resnext101_32x8d", "layer3.0.conv2")])
def test_image_0_has_the_same_bits_alone_and_at_index_2_of_a_batch_of_3(engines, arch, name):
    """A stride-1 layer on 7 x 7 maps (49 pixels per image: a wave's 16 pixels straddle images) and two stride-2 layers."""
    eng, d = engines[arch], gd.layer(arch, name)
    x_hi, x_lo, _x = gd.draws(d, 3, device=eng.device)
    a_hi, a_lo = _launch_grouped(eng, d, x_hi[:1].contiguous(), x_lo[:1].contiguous(), 1)
    order = [1, 2, 0]
    b_hi, b_lo = _launch_grouped(eng, d, x_hi[order].contiguous(), x_lo[order].contiguous(), 3)
    n = d.hout * d.hout
    assert torch.equal(a_hi.payload_bits, b_hi.payload_bits[2 * n:]) and torch.equal(a_lo.payload_bits, b_lo.payload_bits[2 * n:])


# ------------------------------------------------------------------------------------------------
# 5. the dense layers on their default tiles, the conv3 + downsample launches
# ------------------------------------------------------------------------------------------------
def _bn(sd, bn, dev):
    s = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + EPS)
    return s.to(dev), (sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * s).to(dev)


def _dense_key(d):
    return (d.cin, d.cout, d.ksize, d.stride, d.hin, d.residual)


def _dense_want(sd, d, x64, res64):
    """fp64 conv + BatchNorm (+ residual) (+ ReLU) as one matrix product per tap: [B][hout][hout][cout] on the device."""
    name, bn = d.name.decode(), d.bn_name.decode()
    dev = x64.device
    w = sd[name + ".weight"].double().reshape(d.cout, d.cin, d.ksize, d.ksize).to(dev)
    xc = F.pad(x64, (0, 0, d.pad, d.pad, d.pad, d.pad)) if d.pad else x64
    s, ho = d.stride, d.hout
    acc = None
    for ky in range(d.ksize):
        for kx in range(d.ksize):
            y = xc[:, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (ho - 1) + 1:s, :].reshape(-1, d.cin) @ w[:, :, ky, kx].t()
            acc = y if acc is None else acc + y
    if bn:
        sc, sh = _bn(sd, bn, dev)
        acc = acc * sc + sh
    else:
        acc = acc + sd[name + ".bias"].double().to(dev)
    acc = acc.view(x64.shape[0], ho, ho, d.cout)
    if res64 is not None:
        acc = acc + res64
    return torch.relu(acc) if d.relu else acc


def _run_dense(eng, sd, i, batch):
    d = eng.layers[i]
    dev = eng.device
    last = i == len(eng.layers) - 1
    g = torch.Generator(device=dev).manual_seed(1000 * i + batch)
    xh, xl = split(torch.randn(batch, d.hin, d.hin, d.cin, generator=g, device=dev).clamp_min(-0.5) * 1.5)
    rh = rl = None
    if d.residual:
        rh, rl = split(torch.randn(batch, d.hout, d.hout, d.cout, generator=g, device=dev))
    if i == 0:      # the stem reads the engine's padded NHWC4 staging: write the interior, zero border and 4th channel
        stage_stem_input(eng, xh, xl, batch)
        in_h = in_l = None
    else:
        in_h, in_l = xh, xl
    if last:
        out = torch.full((batch, d.cout), float("nan"), dtype=torch.float32, device=dev)
        rc = eng._lib.mpx_conv_bn_act(eng._h, i, ptr(in_h), ptr(in_l), None, None, None, None, ptr(out), batch, eng._stream())
        _lib.check(eng._h, rc, "mpx_conv_bn_act")
        torch.cuda.synchronize()
        got = out.double().view(batch, 1, 1, d.cout)
    else:
        oh = torch.full((batch + 1, d.hout, d.hout, d.cout), float("nan"), dtype=torch.float16, device=dev)
        ol = torch.full_like(oh, float("nan"))
        rc = eng._lib.mpx_conv_bn_act(eng._h, i, ptr(in_h), ptr(in_l), ptr(rh), ptr(rl), ptr(oh), ptr(ol), None, batch, eng._stream())
        _lib.check(eng._h, rc, "mpx_conv_bn_act")
        torch.cuda.synchronize()
        assert torch.isnan(oh[batch]).all() and torch.isnan(ol[batch]).all(), "%s wrote past its last pixel" % d.name.decode()
        got = merge(oh[:batch], ol[:batch]).double()
    ran = eng._lib.mpx_last_conv_kernels(eng._h)
    want = _dense_want(sd, d, merge(xh, xl).double(), merge(rh, rl).double() if d.residual else None)
    return got, want, ran


def _check_dense(eng, sd, i, batch):
    d = eng.layers[i]
    tile = eng._lib.mpx_get_conv_tile(eng._h, i)
    got, want, ran = _run_dense(eng, sd, i, batch)
    assert not torch.isnan(got).any(), d.name
    err, scale = (got - want).abs().max().item(), want.abs().max().item()
    bound = layer_bound(d, scale, k=d.cin * d.ksize * d.ksize)
    print("%s %s %d->%d k%d s%d h%d res %d default tile %d batch %d: max err %.3e (scale %.2f, bound %.3e), kernels 0x%x"
          % (eng.arch, d.name.decode(), d.cin, d.cout, d.ksize, d.stride, d.hin, d.residual, tile, batch, err, scale, bound, ran))
    assert err <= bound, "%s batch %d: max err %.3e (scale %.2f, bound %.3e)" % (d.name.decode(), batch, err, scale, bound)
    return tile, ran


def test_every_distinct_dense_shape_on_its_default_tile(engines):
    """ResNeXt-50's distinct dense shapes (the stem and fc included) at batch 5, the 32x8d shapes it does not have at batch 2."""
    seen, counts = set(), {}
    for arch, batch in zip(ARCHS, (5, 2)):
        eng, sd = engines[arch], synth.make_state_dict(arch)
        n = 0
        for i, d in enumerate(eng.layers):
            if eng.groups[i] > 1 or _dense_key(d) in seen:
                continue
            seen.add(_dense_key(d))
            _check_dense(eng, sd, i, batch)
            n += 1
        counts[arch] = n
    print("distinct dense shapes checked: %s" % counts)
    # 32x4d: the stem, fc, and per stage the conv1 of block 0, the conv1 of the other blocks, conv3 and the downsample conv: 2 + 4 * 4.
    # 32x8d adds its four conv3 (square, with a residual), 256 -> 512 @ 56, 512 -> 1024 @ 28, 1024 -> 2048 @ 14 and 2048 -> 2048 @ 7; its
    # other shapes (the downsample convs, 64 -> 256, 256 -> 256 @ 56, 512 -> 512 @ 28, 1024 -> 1024 @ 14) are 32x4d's
    assert counts == {"resnext50_32x4d": 18, "resnext101_32x8d": 8}


def _run_dual(eng, sd, stage, batch):
    i, j = layer_index(eng, "layer%d.0.conv3" % stage), layer_index(eng, "layer%d.0.downsample.0" % stage)
    d3, dd = eng.layers[i], eng.layers[j]
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(77 * stage + batch)
    t2 = split(torch.randn(batch, d3.hin, d3.hin, d3.cin, generator=g, device=dev).clamp_min(0) * 1.5)
    x = split(torch.randn(batch, dd.hin, dd.hin, dd.cin, generator=g, device=dev).clamp_min(0) * 1.5)
    oh = torch.full((batch + 1, d3.hout, d3.hout, d3.cout), float("nan"), dtype=torch.float16, device=dev)
    ol = torch.full_like(oh, float("nan"))
    rc = eng._lib.mpx_conv_dual_bn_act(eng._h, i, ptr(t2[0]), ptr(t2[1]), ptr(x[0]), ptr(x[1]), ptr(oh), ptr(ol), batch, eng._stream())
    _lib.check(eng._h, rc, "mpx_conv_dual_bn_act")
    ran = eng._lib.mpx_last_conv_kernels(eng._h)
    torch.cuda.synchronize()
    assert torch.isnan(oh[batch]).all() and torch.isnan(ol[batch]).all(), "the dual launch wrote past its last pixel"
    w3 = sd[d3.name.decode() + ".weight"].double().reshape(d3.cout, d3.cin).to(dev)
    wd = sd[dd.name.decode() + ".weight"].double().reshape(dd.cout, dd.cin).to(dev)
    s3, b3 = _bn(sd, d3.bn_name.decode(), dev)
    sds, bds = _bn(sd, dd.bn_name.decode(), dev)
    y3 = merge(*t2).double().reshape(-1, d3.cin) @ w3.t()
    yd = merge(*x)[:, ::dd.stride, ::dd.stride, :].double().reshape(-1, dd.cin) @ wd.t()
    want = torch.relu(y3 * s3 + b3 + yd * sds + bds).reshape(batch, d3.hout, d3.hout, d3.cout)
    got = merge(oh[:batch], ol[:batch]).double()
    assert not torch.isnan(got).any()
    err, scale = (got - want).abs().max().item(), want.abs().max().item()
    bound = layer_bound(d3, scale, k=d3.cin + dd.cin)
    print("%s layer%d.0 conv3 + downsample (k1, k2) = (%d, %d) batch %d: max err %.3e (scale %.2f, bound %.3e), kernels 0x%x"
          % (eng.arch, stage, d3.cin, dd.cin, batch, err, scale, bound, ran))
    assert err <= bound
    return d3.cin, dd.cin, ran


def test_the_dual_launches_of_both_networks(engines):
    sd = synth.make_state_dict(ARCHS[0])
    assert [_run_dual(engines[ARCHS[0]], sd, s, 5)[:2] for s in (1, 2, 3, 4)] == [(128, 64), (256, 256), (512, 512), (1024, 1024)]
    sd = synth.make_state_dict(ARCHS[1])
    assert [_run_dual(engines[ARCHS[1]], sd, s, 2)[:2] for s in (1, 2, 3, 4)] == [(256, 64), (512, 256), (1024, 512), (2048, 1024)]


def _round_batch(eng, hout, cout, tp, rounds=1):
    """The smallest batch whose tiles of 256 channels x tp pixels fill `rounds` rounds of one tile per CU: from there on a persistent
    kernel runs the launch itself instead of handing it to a small-tile kernel."""
    n_c = cout // 256
    b = 1
    while -(-b * hout * hout // tp) * n_c < rounds * eng.num_cus:
        b += 1
    return b


def _round_batch_13(eng, hout, cout):
    """The same for tile 13 through mpx_conv_bn_act, whose launch hands the images behind the last whole round of tiles to tile 2 when that
    remainder is under half a round (launch_conv): the images that stay must still fill a round."""
    n_c, howo, cus = cout // 256, hout * hout, eng.num_cus
    b = 1
    while True:
        total = -(-b * howo // 256) * n_c
        rounds, rest = divmod(total, cus)
        n_a = rounds * cus // n_c * 256 // howo
        kept = n_a if (rounds >= 1 and rest > 0 and 2 * rest <= cus and 1 <= n_a < b) else b
        if -(-kept * howo // 256) * n_c >= cus:
            return b
        b += 1


def test_the_persistent_kernels_themselves_run_the_shapes_new_to_them(engines):
    """default_tile hands the persistent kernels (13, 10, 14) and the dual form of 13 shapes that no served ResNet has; at batch 5 / 2 they
    pass them on to the small-tile kernels.  Here every such shape runs at the smallest batch that fills the kernel's round(s) of tiles --
    what a forward at the default max_batch does -- the kernel itself must have run, and the result is held to the same fp64 bound."""
    TP = {13: 256, 10: 128, 14: 64}
    seen, ran_by_tile = set(), {}
    for arch in ARCHS:
        eng, sd = engines[arch], synth.make_state_dict(arch)
        for i, d in enumerate(eng.layers):
            tile = eng._lib.mpx_get_conv_tile(eng._h, i)
            if eng.groups[i] > 1 or tile not in TP or _dense_key(d) in seen:
                continue
            seen.add(_dense_key(d))
            # the weights-in-registers kernel serves the residual add + ReLU; without a residual operand it hands the launch to tile 10
            own = 10 if (tile == 14 and not d.residual) else tile
            batch = _round_batch_13(eng, d.hout, d.cout) if own == 13 else _round_batch(eng, d.hout, d.cout, TP[own], 2 if own == 14 else 1)
            _tile, ran = _check_dense(eng, sd, i, batch)
            assert ran & (1 << own), "%s %s at batch %d ran kernels %#x, not tile %d's" % (arch, d.name.decode(), batch, ran, own)
            ran_by_tile.setdefault(own, []).append((d.cin, d.cout, d.hin))
        for stage in (1, 2, 3, 4):
            d3 = eng.layers[layer_index(eng, "layer%d.0.conv3" % stage)]
            _k1, _k2, ran = _run_dual(eng, sd, stage, _round_batch(eng, d3.hout, d3.cout, 256))
            assert ran == 1 << 13, "%s layer%d.0 ran kernels %#x, not the persistent dual kernel" % (arch, stage, ran)
    print("persistent kernels on shapes of their own: %s" % ran_by_tile)
    assert sorted(ran_by_tile[13]) == sorted([(256, 256, 56), (512, 512, 28), (1024, 1024, 14), (2048, 1024, 7), (512, 256, 28), (1024, 512, 14),
                                             (2048, 2048, 7)])
    assert sorted(ran_by_tile[14]) == [(256, 512, 28)]
    assert sorted(ran_by_tile[10]) == sorted([(128, 256, 56), (512, 1024, 14), (1024, 2048, 7), (256, 512, 56), (512, 1024, 28), (1024, 2048, 14)])


def _split_batch(eng, hout, cout):
    """The smallest batch at which launch_conv splits a launch of the 256x256 rows (tiles 9 and 13): at least one whole round of tiles, a
    remainder of at most half a round, and at least one image in each part."""
    n_c, howo, cus = cout // 256, hout * hout, eng.num_cus
    b = 1
    while True:
        rounds, rest = divmod(-(-b * howo // 256) * n_c, cus)
        if rounds >= 1 and 0 < rest and 2 * rest <= cus and 1 <= rounds * cus // n_c * 256 // howo < b:
            return b
        b += 1


def test_the_square_conv3_layers_of_32x8d_on_tile_9_with_the_split_launch(engines):
    """32x8d's conv3 layers are square 1x1 layers with a residual operand: tile 9, the 256x256 kernel with one workgroup per tile.  At a
    batch whose last round of tiles is under half full, launch_conv sends the images of the whole rounds to that kernel and the rest to
    tile 2, each with its part of the residual planes: both kernels must have run, on all four shapes."""
    eng, sd = engines[ARCHS[1]], synth.make_state_dict(ARCHS[1])
    shapes = []
    for stage in (1, 2, 3, 4):
        i = layer_index(eng, "layer%d.1.conv3" % stage)
        d = eng.layers[i]
        assert d.residual == 1 and d.cin == d.cout and eng._lib.mpx_get_conv_tile(eng._h, i) == 9
        batch = _split_batch(eng, d.hout, d.cout)
        _tile, ran = _check_dense(eng, sd, i, batch)
        assert ran == (1 << 9 | 1 << 2), "%s at batch %d ran kernels %#x, not the split launch" % (d.name.decode(), batch, ran)
        shapes.append((d.cin, d.hin))
    assert shapes == [(256, 56), (512, 28), (1024, 14), (2048, 7)]


# ------------------------------------------------------------------------------------------------
# 6. descriptors, tiles, refusals, tails
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ARCHS)
def test_descriptors_groups_tiles_and_tails(engines, arch):
    eng = engines[arch]
    lib, h = eng._lib, eng._h
    topo = ref.topology(arch)
    assert len(eng.layers) == len(topo) == lib.mpx_num_convs(h)
    n_grouped = 0
    for i, (d, t) in enumerate(zip(eng.layers, topo)):
        name, bn, cin, cout, k, stride, pad, hin, hout, relu, res, groups = t
        assert (d.name.decode(), d.bn_name.decode(), d.cin, d.cout, d.ksize, d.stride, d.pad, d.hin, d.hout, d.relu, d.residual) == t[:11], name
        g = C.c_int()
        assert lib.mpx_conv_groups(h, i, C.byref(g)) == 0 and g.value == groups == eng.groups[i], name
        pitch, off = C.c_int(), C.c_int()
        assert lib.mpx_conv_in_slice(h, i, C.byref(pitch), C.byref(off), None, None) == 0 and (pitch.value, off.value) == (4 if cin == 3 else cin, 0)
        assert lib.mpx_conv_out_slice(h, i, C.byref(pitch), C.byref(off)) == 0 and (pitch.value, off.value) == (cout, 0)
        tile = lib.mpx_get_conv_tile(h, i)
        if groups > 1:
            n_grouped += 1
            cb = max(cin // groups, 16)
            assert d.k_packed == (9 * cb + 31) // 32 * 32 and d.cout_pad == cout and d.k_packed in (160, 288, 576)
            assert tile == 16
            for other in DENSE_TILES:            # a grouped layer accepts no dense tile ...
                assert lib.mpx_set_conv_tile(h, i, other) == -1 and b"grouped" in lib.mpx_last_error(h), (name, other)
            assert lib.mpx_set_conv_tile(h, i, 16) == 0 and lib.mpx_set_conv_tile(h, i, -1) == 0 and lib.mpx_get_conv_tile(h, i) == 16
        else:
            assert d.k_packed == (224 if cin == 3 else k * k * cin) and d.cout_pad == -(-cout // 128) * 128
            assert lib.mpx_set_conv_tile(h, i, 16) == -1 and b"grouped" in lib.mpx_last_error(h), name      # ... and tile 16 no dense layer
            assert lib.mpx_get_conv_tile(h, i) == tile
            accepted = [t_ for t_ in DENSE_TILES if lib.mpx_set_conv_tile(h, i, t_) == 0]
            assert GENERIC <= set(accepted) and 6 not in accepted and 12 not in accepted, (name, accepted)      # no dense 3x3 layer behind the stem
            assert lib.mpx_set_conv_tile(h, i, -1) == 0 and lib.mpx_get_conv_tile(h, i) == tile and tile in accepted
        for unknown in (15, 17):
            assert lib.mpx_set_conv_tile(h, i, unknown) == -1 and b"product ids" in lib.mpx_last_error(h)
    assert n_grouped == len(gd.grouped_layers(arch))
    g = C.c_int()
    assert lib.mpx_conv_groups(h, len(topo), C.byref(g)) == -1 and lib.mpx_conv_groups(h, -1, C.byref(g)) == -1 and lib.mpx_conv_groups(h, 0, None) == -1
    assert lib.mpx_num_bottleneck_tails(h) == 0 and lib.mpx_num_pointwise_tails(h) == 0
    assert abs(eng.flops_per_forward - 2.0 * ref.macs(arch)) <= 1e-9 * eng.flops_per_forward
    assert eng.has_stem_table and eng.stem == "table"
    # the public packer sees the descriptor alone and stays the dense packer: it refuses a grouped layer's descriptor
    d = eng.layers[layer_index(eng, "layer1.0.conv2")]
    w = np.zeros((d.cout, d.cin // 32, 3, 3), dtype=np.float32)
    v = np.ones(d.cout, dtype=np.float32)
    hi = np.zeros(d.cout_pad * d.k_packed, dtype=np.uint16)
    pp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.mpx_pack_conv_weights(C.byref(d), pp(w), None, pp(v), pp(v), pp(v), pp(v), EPS, pp(hi), pp(hi.copy()), pp(v.copy()), pp(v.copy())) == -1


def test_groups_is_one_on_every_layer_of_another_engine(dev):
    eng = MaskedForwardEngine("resnet18", max_batch=2, device=0)
    try:
        assert eng.groups == [1] * len(eng.layers)
        assert eng._lib.mpx_set_conv_tile(eng._h, 1, 16) == -1 and b"grouped" in eng._lib.mpx_last_error(eng._h)
    finally:
        eng.close()


def test_a_grouped_layer_refuses_a_residual_operand_and_wrong_weight_shapes(engines):
    eng = engines[ARCHS[0]]
    d = gd.layer(ARCHS[0], "layer4.1.conv2")
    i = layer_index(eng, d.name)
    x_hi, x_lo, _x = gd.draws(d, 1, device=eng.device)
    out = torch.zeros(49, d.width, dtype=torch.float16, device=eng.device)
    rc = eng._lib.mpx_conv_bn_act(eng._h, i, ptr(x_hi), ptr(x_lo), ptr(out), ptr(out), ptr(out), ptr(out.clone()), None, 1, eng._stream())
    assert rc == -1 and b"residual" in eng._lib.mpx_last_error(eng._h)
    sd = dict(synth.make_state_dict(ARCHS[0]))
    sd[d.name + ".weight"] = torch.zeros(d.width, d.width, 3, 3)           # the dense shape
    with pytest.raises(ValueError, match="expected"):
        eng.load_state_dict(sd, only=[d.name])


def test_default_max_batch_and_bytes_per_slot(dev):
    """Default max_batch 512; 14.5 MB per slot for 32x4d (a ResNet slot), 27.3 MB for 32x8d (four 56 x 56 x 512 buffers)."""
    for arch, mb in ((ARCHS[0], 14.5), (ARCHS[1], 27.3)):
        small = MaskedForwardEngine(arch, max_batch=8, device=0)
        big = MaskedForwardEngine(arch, max_batch=72, device=0)
        try:
            per_slot = (big.workspace_bytes - small.workspace_bytes) / 64 / 1e6
            print("%s: %.2f MB per slot" % (arch, per_slot))
            assert abs(per_slot - mb) < 0.1
        finally:
            small.close()
            big.close()
    eng = MaskedForwardEngine(ARCHS[0], device=0)
    try:
        assert eng.max_batch == 512
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------
# 7. end to end
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ARCHS)
def test_resnext_end_to_end(engines, golden_dir, arch):
    """resnext50_32x4d: 8 felzenszwalb + 4 grid rows through BOTH stagings (K0 + the MFMA stem, and the stem table); resnext101_32x8d: 4
    rows.  Scores by the MobileNetV2 rule (d = max |fp32 CPU loop - fp64|: bound 2e-5 when 4 d < 2e-5, else 4 d rounded up to one digit,
    never above 1e-4), all logits through the logits lens (4 d_L), every argmax equal.  Measured on one MI355X: resnext50_32x4d engine vs
    fp64 5.2e-06, yardstick 4.1e-06, engine vs fp32 CPU loop 7.9e-06 (bound 2e-5), logits d_L 2.2e-05, engine 3.8e-05 (1.78); resnext101_32x8d
    2.8e-06, 1.1e-06, 2.4e-06, logits 1.0e-05, 1.9e-05 (1.86)."""
    eng, sd = engines[arch], synth.make_state_dict(arch)
    lens = LogitsLens(arch)
    rows = []
    for kind, (img, seg, onoff, label, s64, logits64) in ref.e2e_rows(golden_dir, arch).items():
        x = scorer.to_tensor_normalize(img)
        ref_score, ref_pred, ref_logits = ref.score_masks_reference_loop(sd, arch, x, seg, onoff, label, return_logits=True)
        top2 = np.sort(logits64, axis=1)[:, -2:]
        gap = top2[:, 1] - top2[:, 0]
        peaks = F.softmax(torch.from_numpy(logits64), 1).max(1)[0].numpy()
        assert gap.min() >= 1e-3 and peaks.min() >= 0.05 and peaks.max() <= 0.95      # every row: tests/test_resnext_cpu.py holds the weights to it
        err_cpu = float(np.abs(ref_score.astype(np.float64) - s64).max())
        for stem in (("conv", "table") if arch == ARCHS[0] else ("conv",)):
            _o, score, pred, logits = eng.score_masks(img, seg, onoff, label, return_logits=True, stem=stem)
            lens.add("%s stem=%s" % (kind, stem), logits, ref_logits, logits64)
            err_engine = float(np.abs(score.astype(np.float64) - s64).max())
            err_both = float(np.abs(score.astype(np.float64) - ref_score.astype(np.float64)).max())
            print("%s %s stem=%s: %d masks, label %d, scores %.4f..%.4f" % (arch, kind, stem, len(s64), label, ref_score.min(), ref_score.max()))
            print("%s %s stem=%s: max|d| engine vs fp64 %.3e, fp32 CPU loop vs fp64 (the yardstick) %.3e, engine vs fp32 CPU loop %.3e, smallest fp64 logit gap %.4f"
                  % (arch, kind, stem, err_engine, err_cpu, err_both, gap.min()))
            rows.append((kind, stem, err_engine, err_cpu, err_both, pred, ref_pred, logits64.argmax(1)))
        p_label, _ = eng.predict(img)
        assert p_label == label
    d = max(r[3] for r in rows)
    bound = SCORE_BOUND if 4 * d < SCORE_BOUND else min(round_up_one_digit(4 * d), SCORE_TOL)
    print("%s: yardstick distance %.3e over %d rows -> end-to-end bound %.1e" % (arch, d, sum(len(r[5]) for r in rows), bound))
    for kind, stem, err_engine, _err_cpu, err_both, pred, ref_pred, arg64 in rows:
        assert err_engine <= bound and err_both <= bound, (kind, stem, err_engine, err_both, bound)
        assert (pred == arg64).all() and (pred == ref_pred).all()          # every row
    lens.check()
