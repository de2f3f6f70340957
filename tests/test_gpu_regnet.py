"""RegNetX-400MF .. -8GF on the GPU (run on the MI355X box: pytest -m gpu): the any-width grouped 3x3 kernel (csrc/mpx_gconvw.h, tile 18) on
every distinct grouped shape of the five networks behind fences and inside the per-element bound of tests/regnet_draws.py, the pad channels,
group isolation and position independence bit for bit, the cross-check against tile 16, the dense shapes new to the other kernels against
fp64, the descriptors, tiles and refusals, and the five networks end to end on the rows tests/test_regnet_cpu.py holds the weights to.

The grouped launch does not cap its grid (ceil(M / 16) workgroups in x, a quarter of the units in y), so there is no capped-grid case to run."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import regnet_draws as gd
import regnet_ref as ref
from gpu_common import dev, Fenced, GENERIC, layer_bound, layer_index, merge, ptr, split  # noqa: F401  (dev is a fixture)
from net_harness import check_api, check_end_to_end, check_position_independence, Reference, stage_stem_input
from network_interpretation_imagenet_amd import _lib, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine

pytestmark = pytest.mark.gpu

ARCHS = ref.ARCHS
DENSE_TILES = (0, 1, 2, 4, 6, 7, 9, 10, 12, 13, 14)
EPS = 1e-5


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


def _pitches(eng, i):
    pin, pout, off = C.c_int(), C.c_int(), C.c_int()
    assert eng._lib.mpx_conv_in_slice(eng._h, i, C.byref(pin), C.byref(off), None, None) == 0 and off.value == 0
    assert eng._lib.mpx_conv_out_slice(eng._h, i, C.byref(pout), C.byref(off)) == 0 and off.value == 0
    return pin.value, pout.value


def _sentinel(shape, dev):
    return torch.full(shape, gd.SENTINEL_BITS, dtype=torch.int16, device=dev).view(torch.float16)


def _at_pitch(x, pitch, pad_sentinel=False):
    """[..., width] -> contiguous [..., pitch] with the pad channels zero (or the NaN sentinel)."""
    out = _sentinel(x.shape[:-1] + (pitch,), x.device) if pad_sentinel else torch.zeros(x.shape[:-1] + (pitch,), dtype=x.dtype, device=x.device)
    out[..., :x.shape[-1]] = x
    return out.contiguous()


def _launch_grouped(eng, d, x_hi, x_lo, batch, tile=gd.TILE, pad_sentinel=False):
    """mpx_conv_bn_act of grouped layer d over `batch` images (x_*: [batch][hin][hin][width], placed into planes at the layer's input pitch)
    -> fenced (hi, lo) at the output pitch; the kernel of `tile` and nothing else must have run.  Every pad channel of the output is +0."""
    i = layer_index(eng, d.name)
    pin, pout = _pitches(eng, i)
    assert pin == pout == ref.pitch(d.width)
    rows = batch * d.hout * d.hout
    xh, xl = _at_pitch(x_hi, pin, pad_sentinel), _at_pitch(x_lo, pin, pad_sentinel)
    hi, lo = Fenced(rows, pout, eng.device), Fenced(rows, pout, eng.device)
    rc = eng._lib.mpx_conv_bn_act(eng._h, i, ptr(xh), ptr(xl), None, None, ptr(hi.payload), ptr(lo.payload), None, batch, eng._stream())
    _lib.check(eng._h, rc, "mpx_conv_bn_act(%s, batch %d)" % (d.name, batch))
    mask = eng._lib.mpx_last_conv_kernels(eng._h)
    torch.cuda.synchronize()
    assert mask == 1 << tile, "%s ran kernels %#x" % (d.name, mask)
    for plane, which in ((hi, "hi"), (lo, "lo")):
        assert plane.problems() == [], "%s %s batch %d, %s plane: %s" % (d.arch, d.name, batch, which, "; ".join(plane.problems()))
        assert (plane.payload_bits[:, d.width:] == 0).all(), "%s %s: a pad channel of the %s plane is not +0" % (d.arch, d.name, which)
    return hi, lo


# ------------------------------------------------------------------------------------------------
# 1. every distinct grouped layer of the five networks, behind fences, inside the per-element bound
# ------------------------------------------------------------------------------------------------
CASES = [(d, b) for d in gd.all_cases() for b in gd.batches(d)]


@pytest.mark.parametrize("d,batch", CASES, ids=["%s-%s-b%d" % (d.arch, d.name, b) for d, b in CASES])
def test_grouped_layer_behind_fences_inside_the_per_element_bound(engines, sds, d, batch):
    """(cg, groups, stride, map) of every grouped layer: cg 16 / 24 / 48 / 120, 2 .. 42 groups (3, 7, 9, 17, 21, 25, 38 among them: a ragged last
    workgroup), stride 2 on 112 .. 14 maps and stride 1 on 56 .. 7.  On the 14 x 14 and 7 x 7 output maps M = 196 / 49 / 147 / 588 is no multiple of 16."""
    eng = engines[d.arch]
    i = layer_index(eng, d.name)
    e = eng.layers[i]
    assert (e.cin, e.cout, e.ksize, e.stride, e.pad, e.hin, e.hout, e.relu, e.residual) == (d.width, d.width, 3, d.stride, 1, d.hin, d.hout, 1, 0)
    assert eng.groups[i] == d.groups and eng._lib.mpx_get_conv_tile(eng._h, i) == gd.TILE
    x = gd.draws(d, batch, device=eng.device)
    pre, want, b = (t.reshape(-1, d.width) for t in gd.reference(sds[d.arch], d, x[2]))
    gd.preconditions(want)
    hi, lo = _launch_grouped(eng, d, x[0], x[1], batch)
    got = hi.payload[:, :d.width].double() + lo.payload[:, :d.width].double()
    assert not torch.isnan(got).any()
    err, tol = (got - want).abs(), gd.tol(d, b)
    ratio = (err / tol).max().item()
    worst = torch.argmax(err / tol).item()
    print("%s %s cg %d groups %d stride %d map %d batch %d: worst err / tol %.3f (pixel row %d, channel %d), C %g; max norm %.2e"
          % (d.arch, d.name, d.cg, d.groups, d.stride, d.hin, batch, ratio, worst // d.width, worst % d.width, gd.C_TOL[(d.arch, d.name)],
             err.max().item() / max(want.abs().max().item(), 1.0)))
    assert ratio <= 1.0, "%d elements over their bound, worst err / tol %.3f at pixel row %d, channel %d" % (
        int((err > tol).sum()), ratio, worst // d.width, worst % d.width)
    neg = pre < -tol
    assert neg.any() and (hi.payload_bits[:, :d.width][neg] == 0).all() and (lo.payload_bits[:, :d.width][neg] == 0).all(), \
        "a clearly negative pre-activation is not +0 in both planes"


# ------------------------------------------------------------------------------------------------
# 2. the pad channels
# ------------------------------------------------------------------------------------------------
PADDED = [("regnet_x_1_6gf", "trunk_output.block1.block1-1.f.b.0"),        # width 72 at pitch 96
          ("regnet_x_400mf", "trunk_output.block4.block4-1.f.b.0"),        # width 400 at pitch 416
          ("regnet_x_8gf", "trunk_output.block3.block3-1.f.b.0")]          # width 720 at pitch 736


@pytest.mark.parametrize("arch,name", PADDED)
def test_pad_channels_are_written_as_zero_and_never_read(engines, arch, name):
    """The output planes are prefilled with the NaN sentinel: every pad channel [width, pitch) comes back as +0 in both planes
    (_launch_grouped asserts it).  Input pad channels filled with the sentinel change no output bit."""
    eng, d = engines[arch], gd.layer(arch, name)
    assert d.width in (72, 400, 720) and ref.pitch(d.width) - d.width in (24, 16)
    x_hi, x_lo, _x = gd.draws(d, 2, device=eng.device)
    a_hi, a_lo = _launch_grouped(eng, d, x_hi, x_lo, 2)
    b_hi, b_lo = _launch_grouped(eng, d, x_hi, x_lo, 2, pad_sentinel=True)
    assert torch.equal(a_hi.payload_bits, b_hi.payload_bits) and torch.equal(a_lo.payload_bits, b_lo.payload_bits)


# ------------------------------------------------------------------------------------------------
# 3. group isolation, bit for bit
# ------------------------------------------------------------------------------------------------
ISOLATION = [("regnet_x_1_6gf", "trunk_output.block3.block3-1.f.b.0", (0, 5, 16)),      # cg = 24: two row fragments, the second half empty
             ("regnet_x_8gf", "trunk_output.block3.block3-1.f.b.0", (0, 3, 5))]         # cg = 120: two chunks of four fragments


@pytest.mark.parametrize("arch,name,groups", ISOLATION)
def test_changing_one_groups_input_changes_that_groups_output_only(engines, arch, name, groups):
    eng, d = engines[arch], gd.layer(arch, name)
    x_hi, x_lo, _x = gd.draws(d, 2, device=eng.device)
    base_hi, base_lo = _launch_grouped(eng, d, x_hi, x_lo, 2)
    for g in groups:
        y_hi, y_lo = x_hi.clone(), x_lo.clone()
        ch = slice(g * d.cg, (g + 1) * d.cg)
        y_hi[..., ch] = (y_hi[..., ch].float() * -1.5 + 0.25).half()
        y_lo[..., ch] = 0
        hi, lo = _launch_grouped(eng, d, y_hi, y_lo, 2)
        other = torch.ones(hi.cout, dtype=torch.bool, device=eng.device)
        other[ch] = False
        assert torch.equal(hi.payload_bits[:, other], base_hi.payload_bits[:, other]) and torch.equal(lo.payload_bits[:, other], base_lo.payload_bits[:, other]), \
            "%s: changing the input of group %d changed another group's output" % (name, g)
        assert not torch.equal(hi.payload_bits[:, ch], base_hi.payload_bits[:, ch]), "%s: group %d does not read its own input" % (name, g)


@pytest.mark.parametrize("arch,name,groups", ISOLATION)
def test_weights_in_one_group_alone_give_exact_zeros_elsewhere(engines, sds, arch, name, groups):
    """Non-zero weights in one group, a shift of 0 (beta = running_mean = 0): every other group's output is +0 in both planes, and the
    group's own output is what the reference says."""
    eng, d, sd = engines[arch], gd.layer(arch, name), sds[arch]
    x_hi, x_lo, x = gd.draws(d, 2, device=eng.device)
    try:
        for g in groups[1:]:
            ch = slice(g * d.cg, (g + 1) * d.cg)
            mod = dict(sd)
            w = torch.zeros_like(sd[name + ".weight"])
            w[ch] = sd[name + ".weight"][ch]
            mod[name + ".weight"] = w
            mod[d.bn_name + ".bias"] = torch.zeros(d.width)
            mod[d.bn_name + ".running_mean"] = torch.zeros(d.width)
            eng.load_state_dict(mod, only=[name])
            hi, lo = _launch_grouped(eng, d, x_hi, x_lo, 2)
            other = torch.ones(hi.cout, dtype=torch.bool, device=eng.device)
            other[ch] = False
            assert (hi.payload_bits[:, other] == 0).all() and (lo.payload_bits[:, other] == 0).all(), "%s: group %d's weights reach another group" % (name, g)
            _pre, want, b = (t.reshape(-1, d.width) for t in gd.reference(mod, d, x))
            got = hi.payload[:, :d.width].double() + lo.payload[:, :d.width].double()
            assert (want[:, ch] > 0).any() and ((got - want).abs() <= gd.tol(d, b)).all()
    finally:
        eng.load_state_dict(sd, only=[name])


# ------------------------------------------------------------------------------------------------
# 4. position independence
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,name", [("regnet_x_400mf", "trunk_output.block4.block4-1.f.b.0"), ("regnet_x_1_6gf", "trunk_output.block4.block4-0.f.b.0"),
                                       ("regnet_x_8gf", "trunk_output.block4.block4-0.f.b.0")])
def test_image_0_has_the_same_bits_alone_and_at_index_2_of_a_batch_of_3(engines, arch, name):
    """Layers on 7 x 7 output maps (49 pixels per image: a wave's 16 pixels straddle images), stride 1 and 2, cg 16, 24 and 120."""
    eng, d = engines[arch], gd.layer(arch, name)
    x_hi, x_lo, _x = gd.draws(d, 3, device=eng.device)
    a_hi, a_lo = _launch_grouped(eng, d, x_hi[:1].contiguous(), x_lo[:1].contiguous(), 1)
    order = [1, 2, 0]
    b_hi, b_lo = _launch_grouped(eng, d, x_hi[order].contiguous(), x_lo[order].contiguous(), 3)
    n = d.hout * d.hout
    assert torch.equal(a_hi.payload_bits, b_hi.payload_bits[2 * n:]) and torch.equal(a_lo.payload_bits, b_lo.payload_bits[2 * n:])


# ------------------------------------------------------------------------------------------------
# 5. the cross-check against tile 16
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,name", [("regnet_x_400mf", "trunk_output.block2.block2-0.f.b.0"), ("regnet_x_400mf", "trunk_output.block2.block2-1.f.b.0"),
                                       ("regnet_x_800mf", "trunk_output.block2.block2-1.f.b.0")])
def test_tile_16_gives_the_same_bits_where_the_shape_is_one_of_its_own(engines, arch, name):
    """cg = 16, width 64 / 128 (a multiple of 64: 4 / 8 groups, pitch = width): mpx_set_conv_tile(i, 16) on such a RegNetX layer runs
    gconv3x3_f16x3_kernel<16> on the layer's own packed planes (for cg = 16 the two plane layouts coincide).  Identical bits."""
    eng, d = engines[arch], gd.layer(arch, name)
    i = layer_index(eng, d.name)
    assert d.cg == 16 and d.width % 64 == 0
    x_hi, x_lo, _x = gd.draws(d, 3, device=eng.device)
    a_hi, a_lo = _launch_grouped(eng, d, x_hi, x_lo, 3)
    try:
        assert eng._lib.mpx_set_conv_tile(eng._h, i, 16) == 0, eng._lib.mpx_last_error(eng._h)
        b_hi, b_lo = _launch_grouped(eng, d, x_hi, x_lo, 3, tile=16)
    finally:
        assert eng._lib.mpx_set_conv_tile(eng._h, i, -1) == 0 and eng._lib.mpx_get_conv_tile(eng._h, i) == gd.TILE
    assert torch.equal(a_hi.payload_bits, b_hi.payload_bits) and torch.equal(a_lo.payload_bits, b_lo.payload_bits)


# ------------------------------------------------------------------------------------------------
# 6. the dense shapes new to the other kernels
# ------------------------------------------------------------------------------------------------
def _bn(sd, bn, dev):
    s = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + EPS)
    return s.to(dev), (sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * s).to(dev)


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
    sc, sh = _bn(sd, bn, dev)
    acc = (acc * sc + sh).view(x64.shape[0], ho, ho, d.cout)
    if res64 is not None:
        acc = acc + res64
    return torch.relu(acc) if d.relu else acc


def _run_dense(eng, sd, i, batch):
    """Layer i on its current tile, on planes at its pitches (pad channels of the input and the residual +0) -> (got, want, kernels)."""
    d, dev = eng.layers[i], eng.device
    pin, pout = _pitches(eng, i)
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
    oh, ol = _sentinel((batch + 1, d.hout, d.hout, pout), dev), _sentinel((batch + 1, d.hout, d.hout, pout), dev)
    res_h, res_l = (_at_pitch(rh, pout), _at_pitch(rl, pout)) if d.residual else (None, None)
    rc = eng._lib.mpx_conv_bn_act(eng._h, i, ptr(in_h), ptr(in_l), ptr(res_h), ptr(res_l), ptr(oh), ptr(ol), None, batch, eng._stream())
    _lib.check(eng._h, rc, "mpx_conv_bn_act")
    ran = eng._lib.mpx_last_conv_kernels(eng._h)
    torch.cuda.synchronize()
    assert torch.isnan(oh[batch]).all() and torch.isnan(ol[batch]).all(), "%s wrote past its last pixel" % d.name.decode()
    assert (oh[:batch, ..., d.cout:].view(torch.int16) == 0).all() and (ol[:batch, ..., d.cout:].view(torch.int16) == 0).all(), "pad channels are not +0"
    got = merge(oh[:batch, ..., :d.cout], ol[:batch, ..., :d.cout]).double()
    want = _dense_want(sd, d, merge(xh, xl).double(), merge(rh, rl).double() if d.residual else None)
    return got, want, ran


DENSE = [("regnet_x_400mf", "stem.0", 3, 32, 3, 0),
         ("regnet_x_1_6gf", "trunk_output.block1.block1-1.f.a.0", 72, 72, 1, 0),        # pitch 96
         ("regnet_x_1_6gf", "trunk_output.block1.block1-1.f.c.0", 72, 72, 1, 1),
         ("regnet_x_400mf", "trunk_output.block4.block4-1.f.a.0", 400, 400, 1, 0),      # pitch 416
         ("regnet_x_400mf", "trunk_output.block4.block4-1.f.c.0", 400, 400, 1, 1),
         ("regnet_x_1_6gf", "trunk_output.block1.block1-0.proj.0", 32, 72, 1, 0),       # 1x1 stride 2
         ("regnet_x_400mf", "trunk_output.block4.block4-0.proj.0", 160, 400, 1, 0),
         ("regnet_x_8gf", "trunk_output.block1.block1-0.f.b.0", 80, 80, 3, 0),          # the dense 3x3 of 8GF, stride 2 on 112 x 112 ...
         ("regnet_x_8gf", "trunk_output.block1.block1-1.f.b.0", 80, 80, 3, 0)]          # ... and stride 1 on 56 x 56


@pytest.mark.parametrize("arch,name,cin,cout,k,res", DENSE, ids=["%s-%s" % (a, n) for a, n, *_ in DENSE])
def test_dense_shape_on_its_default_tile_and_on_every_tile_that_accepts_it(engines, sds, arch, name, cin, cout, k, res):
    eng, sd = engines[arch], sds[arch]
    i = layer_index(eng, name)
    d = eng.layers[i]
    assert (d.cin, d.cout, d.ksize, d.residual) == (cin, cout, k, res) and eng.groups[i] == 1
    default = eng._lib.mpx_get_conv_tile(eng._h, i)
    accepted = [t for t in DENSE_TILES if eng._lib.mpx_set_conv_tile(eng._h, i, t) == 0]
    assert default in accepted and GENERIC <= set(accepted)
    batch = 1 if d.hin >= 112 else 3
    try:
        for tile in accepted:
            assert eng._lib.mpx_set_conv_tile(eng._h, i, tile) == 0
            got, want, ran = _run_dense(eng, sd, i, batch)
            assert not torch.isnan(got).any(), (name, tile)
            err, scale = (got - want).abs().max().item(), want.abs().max().item()
            bound = layer_bound(d, scale, k=d.cin * d.ksize * d.ksize)
            print("%s %s %d->%d k%d s%d h%d res %d tile %d%s batch %d: max err %.3e (scale %.2f, bound %.3e), kernels 0x%x"
                  % (arch, name, d.cin, d.cout, d.ksize, d.stride, d.hin, d.residual, tile, " (default)" if tile == default else "", batch, err, scale, bound, ran))
            assert err <= bound, "%s tile %d: max err %.3e (scale %.2f, bound %.3e)" % (name, tile, err, scale, bound)
    finally:
        assert eng._lib.mpx_set_conv_tile(eng._h, i, -1) == 0 and eng._lib.mpx_get_conv_tile(eng._h, i) == default


# ------------------------------------------------------------------------------------------------
# 7. descriptors, groups, tiles, refusals, workspace
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ARCHS)
def test_descriptors_groups_tiles_and_refusals(engines, arch):
    eng = engines[arch]
    lib, h = eng._lib, eng._h
    topo = ref.topology(arch)
    assert len(eng.layers) == len(topo) == lib.mpx_num_convs(h) == ref.TABLE[arch][7]
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
            ok16 = cg == 16 and cin % 64 == 0      # ... and tile 16 where the shape is one of that kernel's (pitch = width follows from width % 64 == 0)
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
    assert n_grouped == len(gd.grouped_layers(arch))
    assert sorted(set(on_16)) == {"regnet_x_400mf": [64], "regnet_x_800mf": [64, 128]}.get(arch, [])
    assert lib.mpx_num_bottleneck_tails(h) == 0 and lib.mpx_num_pointwise_tails(h) == 0
    assert abs(eng.flops_per_forward - 2.0 * ref.TABLE[arch][6]) <= 1e-9 * eng.flops_per_forward
    assert not eng.has_stem_table and eng.stem == "conv"
    # staging is K0 only: the stem-table and stem + pool entry points return MPX_E_STATE
    lab = torch.zeros(224, 224, dtype=torch.int32, device=eng.device)
    assert lib.mpx_stem_table_build(h, None, None, ptr(lab), 1, None, None, None) == -2 and b"RegNetX" in lib.mpx_last_error(h)
    out = torch.zeros(8, dtype=torch.float16, device=eng.device)
    assert lib.mpx_stem_conv_maxpool(h, ptr(out), ptr(out), 1, None) == -2 and b"7x7 stem" in lib.mpx_last_error(h)


def test_unknown_ids_in_the_regnet_range_are_refused(dev):
    lib = _lib.load()
    known = {ref.TABLE[a][0] for a in ARCHS}
    for arch_id in (14000, 14001, 14005, 14040, 14160, 14320, 14999):
        assert arch_id not in known
        h = C.c_void_p()
        assert lib.mpx_create(arch_id, 2, 0, C.byref(h)) == -1 and not h.value


def test_tile_18_is_refused_on_every_layer_of_other_engines(dev):
    for arch, grouped in (("resnet18", None), ("resnext50_32x4d", "layer1.0.conv2")):
        eng = MaskedForwardEngine(arch, max_batch=2, device=0)
        try:
            assert eng._lib.mpx_set_conv_tile(eng._h, 1, 18) == -1 and b"grouped" in eng._lib.mpx_last_error(eng._h)
            if grouped:
                i = layer_index(eng, grouped)
                assert eng._lib.mpx_set_conv_tile(eng._h, i, 18) == -1 and b"grouped" in eng._lib.mpx_last_error(eng._h)
                assert eng._lib.mpx_get_conv_tile(eng._h, i) == 16
        finally:
            eng.close()


def test_a_grouped_layer_refuses_a_residual_operand_and_wrong_weight_shapes(engines, sds):
    arch = "regnet_x_1_6gf"
    eng = engines[arch]
    d = gd.layer(arch, "trunk_output.block4.block4-1.f.b.0")
    i = layer_index(eng, d.name)
    pitch = ref.pitch(d.width)
    x = torch.zeros(1, d.hin, d.hin, pitch, dtype=torch.float16, device=eng.device)
    out = torch.zeros(49, pitch, dtype=torch.float16, device=eng.device)
    rc = eng._lib.mpx_conv_bn_act(eng._h, i, ptr(x), ptr(x), ptr(out), ptr(out), ptr(out), ptr(out.clone()), None, 1, eng._stream())
    assert rc == -1 and b"residual" in eng._lib.mpx_last_error(eng._h)
    for shape in ((d.width, d.width, 3, 3), (d.width, 16, 3, 3)):           # the dense shape; another group width
        sd = dict(sds[arch])
        sd[d.name + ".weight"] = torch.zeros(shape)
        with pytest.raises(ValueError, match="expected"):
            eng.load_state_dict(sd, only=[d.name])


@pytest.mark.parametrize("arch", ARCHS)
def test_default_max_batch_and_bytes_per_slot(dev, arch):
    """Default max_batch 512.  Bytes per slot from the plan: the padded NHWC4 staging, four activation buffers of the largest map at its
    pitch, the pooled planes, the logits -- two split-fp16 planes each; every plane is rounded up to 256 bytes once per engine."""
    act = max(c[8] * c[8] * ref.pitch(c[3]) for c in ref.topology(arch)[:-1])
    feat = ref.TABLE[arch][1][3]
    want = 2 * 2 * 230 * 230 * 4 + 4 * 2 * 2 * act + 2 * 2 * ref.pitch(feat) + 4 * 1000
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
        eng = MaskedForwardEngine(arch, device=0)
        try:
            assert eng.max_batch == 512
        finally:
            eng.close()


# ------------------------------------------------------------------------------------------------
# 8. end to end
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ARCHS)
def test_regnet_end_to_end(engines, sds, golden_dir, arch):
    """400MF: 8 felzenszwalb + 4 grid rows; 800MF / 1.6GF / 3.2GF: 4 + 2; 8GF: 3.  Scores by the MobileNetV2 rule (d = max |fp32 CPU loop - fp64|:
    bound 2e-5 when 4 d < 2e-5, else 4 d rounded up to one digit, never above 1e-4), all logits through the logits lens (4 d_L), every argmax
    equal."""
    rows = [(kind,) + row for kind, row in ref.e2e_rows(golden_dir, arch).items()]
    check_end_to_end(engines[arch], arch, Reference(ref, sds[arch], arch), rows,
                     "%(arch)s: yardstick distance %(d).3e over %(n)d rows -> end-to-end bound %(bound).1e", segments=False, peaks=True)


@pytest.mark.parametrize("arch", ("regnet_x_400mf", "regnet_x_8gf"))
def test_a_mask_row_scores_the_same_bits_wherever_it_sits(engines, golden_dir, arch):
    check_position_independence(engines[arch], *ref.e2e_inputs(golden_dir, "felz"), (3, ((1, 0, (0,)), (8, 41, (0, 5, 7)), (13, 44, (3, 8, 12)))))


def test_api_on_a_regnet_engine(engines, sds, golden_dir):
    arch = "regnet_x_400mf"
    check_api(engines[arch], Reference(ref, sds[arch], arch), *ref.e2e_inputs(golden_dir, "grid"),
              rows=4, same_pred=True, heatmaps=0, predict=False, table_step=None, validate=None)


@pytest.mark.parametrize("arch", ("regnet_x_400mf", "regnet_x_8gf"))
def test_profile_lists_one_row_per_conv_the_grouped_layers_among_them(engines, dev, arch):
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
    assert len(prof["per_conv_ms"]) == len(eng.layers) and all(ms > 0 for ms in prof["per_conv_ms"])      # no conv rides in another's launch
    grouped = [ms for ms, g in zip(prof["per_conv_ms"], eng.groups) if g > 1]
    assert len(grouped) == len(gd.grouped_layers(arch))
    assert prof["launches"]["conv"] == len(eng.layers) and prof["launches"]["head"] == 1
