"""The DUAL form of the persistent 256x256 kernel (csrc/mpx_conv256p.h): a bottleneck stage's first conv3 with its downsample branch
K-concatenated (mpx_conv_dual_bn_act, the launch mpx_forward makes for layer2.0 / layer3.0 / layer4.0), reported as tile id 13.

Every case allocates the output planes one image longer than the batch and prefills them with NaN: the batch must come back finite, the
extra image untouched.  Every case is compared bit for bit (sign of zero included) with tile 7's dual kernel on the same inputs, which the
kernel must reproduce (same order of summation, same epilogue arithmetic).

Tolerance of the fp64 comparison: the project's 4e-6 x max(|want|, 1) of test_conv_with_fused_downsample (split-fp16 operands, 22-bit
products, fp32 accumulation over K <= 1536)."""

import pytest
import torch

from gpu_common import layer_index as _index, merge, ptr as _p, split
from network_interpretation_imagenet_amd import _lib, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng101(mpx_lib):
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = MaskedForwardEngine("resnet101", max_batch=8, device=0).load_state_dict(synth.make_state_dict("resnet101"))
    yield e
    e.close()


def _inputs(eng, stage, batch):
    i, j = _index(eng, "layer%d.0.conv3" % stage), _index(eng, "layer%d.0.downsample.0" % stage)
    d3, dd = eng.layers[i], eng.layers[j]
    g = torch.Generator(device=eng.device).manual_seed(1000 * stage + batch)
    t2 = torch.randn(batch, d3.hin, d3.hin, d3.cin, generator=g, device=eng.device).clamp_min(0) * 1.5
    x = torch.randn(batch, dd.hin, dd.hin, dd.cin, generator=g, device=eng.device).clamp_min(0) * 1.5
    return i, d3, dd, split(t2), split(x)


def _launch(eng, i, d3, t2, x, batch, tile):
    """mpx_conv_dual_bn_act with the main layer on `tile` (-1: its default): (output planes of batch + 1 images, kernels that ran)."""
    oh = torch.full((batch + 1, d3.hout, d3.hout, d3.cout), float("nan"), dtype=torch.float16, device=eng.device)
    ol = torch.full_like(oh, float("nan"))
    eng.set_conv_tile(i, tile)
    try:
        rc = eng._lib.mpx_conv_dual_bn_act(eng._h, i, _p(t2[0]), _p(t2[1]), _p(x[0]), _p(x[1]), _p(oh), _p(ol), batch, eng._stream())
        _lib.check(eng._h, rc, "mpx_conv_dual_bn_act")
        mask = eng._lib.mpx_last_conv_kernels(eng._h)
        torch.cuda.synchronize()
    finally:
        eng.set_conv_tile(i, -1)
    return oh, ol, mask


def _check_extent(oh, ol, batch):
    for plane in (oh, ol):
        assert torch.isfinite(plane[:batch]).all(), "a pixel of the batch was not written"
        assert torch.isnan(plane[batch]).all(), "the launch wrote past its last pixel"


def _same_bits(a, b):
    return torch.equal(a, b) and torch.equal(torch.signbit(a), torch.signbit(b))


def _new_against_tile7(eng, stage, batch):
    i, d3, dd, t2, x = _inputs(eng, stage, batch)
    oh, ol, mask = _launch(eng, i, d3, t2, x, batch, -1)
    assert mask == 1 << 13, "layer%d.0 at batch %d ran kernels %#x, not the persistent dual kernel" % (stage, batch, mask)
    _check_extent(oh, ol, batch)
    rh, rl, mask7 = _launch(eng, i, d3, t2, x, batch, 7)
    assert mask7 == 1 << 7, mask7
    _check_extent(rh, rl, batch)
    assert _same_bits(oh[:batch], rh[:batch]) and _same_bits(ol[:batch], rl[:batch]), "not bit-identical to tile 7's dual kernel"
    return d3, dd, t2, x, oh, ol


def _bn(sd, d, dev):
    bn = d.bn_name.decode()
    sc = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + 1e-5)
    return sc.to(dev), (sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * sc).to(dev)


@pytest.mark.parametrize("stage,batch", [(2, 43), (3, 85), (4, 170)])
def test_dual256p_against_fp64(eng101, stage, batch):
    """The smallest batches that give one round of 256 tiles (264 each), with a ragged last pixel tile (131.7 / 65.1 / 32.5 pixel tiles);
    layer4.0's tiles straddle its 49-pixel images.  Against relu(bn3(conv3(t2)) + bn_ds(conv_ds(x))) in fp64 on the same split inputs."""
    d3, dd, t2, x, oh, ol = _new_against_tile7(eng101, stage, batch)
    sd = synth.make_state_dict("resnet101")
    dev = eng101.device
    w3 = sd[d3.name.decode() + ".weight"].double().reshape(d3.cout, d3.cin).to(dev)
    wd = sd[dd.name.decode() + ".weight"].double().reshape(dd.cout, dd.cin).to(dev)
    s3, b3 = _bn(sd, d3, dev)
    sds, bds = _bn(sd, dd, dev)
    y3 = merge(*t2).double().reshape(-1, d3.cin) @ w3.t()
    yd = merge(*x)[:, ::dd.stride, ::dd.stride, :].double().reshape(-1, dd.cin) @ wd.t()
    want = torch.relu(y3 * s3 + b3 + yd * sds + bds).reshape(batch, d3.hout, d3.hout, d3.cout)
    got = merge(oh[:batch], ol[:batch]).double()
    err = (got - want).abs().max().item()
    bound = 4e-6 * max(want.abs().max().item(), 1.0)
    print("layer%d.0 batch %d: max |err| %.3e, bound %.3e" % (stage, batch, err, bound))
    assert err <= bound, "layer%d.0: %.3e > %.3e" % (stage, err, bound)


@pytest.mark.parametrize("stage,batch", [(4, 347), (3, 200)])
def test_dual256p_several_tiles_per_workgroup(eng101, stage, batch):
    """layer4.0 at 347 images: 67 pixel tiles x 8 = 536 tiles, two to three per workgroup; layer3.0 at 200: 616 tiles.  The ring runs on
    across tile boundaries, so the operand switch of the NEXT tile happens while this one still computes."""
    _new_against_tile7(eng101, stage, batch)


@pytest.mark.parametrize("stage", [2, 3, 4])
def test_dual256p_small_batch_keeps_tile7(eng101, stage):
    """Under one round of tiles the launch stays with tile 7's dual kernel."""
    batch = 5
    i, d3, dd, t2, x = _inputs(eng101, stage, batch)
    oh, ol, mask = _launch(eng101, i, d3, t2, x, batch, -1)
    assert mask == 1 << 7, mask
    _check_extent(oh, ol, batch)
    rh, rl, mask7 = _launch(eng101, i, d3, t2, x, batch, 7)
    assert mask7 == 1 << 7, mask7
    assert _same_bits(oh[:batch], rh[:batch]) and _same_bits(ol[:batch], rl[:batch])


def test_dual256p_forward_equals_tile7_forward(mpx_lib):
    """ResNet-50 at 170 slots (1042 / 524 / 264 tiles on the three fused launches): scores and predictions of the default forward equal
    those of a forward with the three main layers forced to tile 7, bit for bit.  mpx_last_conv_kernels speaks of ONE conv call, so what
    the forward's fused launches ran is read from the same launches made through mpx_conv_dual_bn_act at the same batch."""
    batch = 170
    eng = MaskedForwardEngine("resnet50", max_batch=batch, device=0, stem="conv").load_state_dict(synth.make_state_dict("resnet50"))
    try:
        dev = eng.device
        img = torch.from_numpy(synth.make_images(1, kind="noise")[0]).to(dev)
        seg = torch.from_numpy(synth.grid_segments()).to(dev)
        onoff = torch.from_numpy(synth.random_onoff(batch, 196)).to(dev)
        labels = torch.zeros(batch, dtype=torch.int32, device=dev)
        mains = [_index(eng, "layer%d.0.conv3" % s) for s in (2, 3, 4)]

        def forward(tile):
            for i in mains:
                eng.set_conv_tile(i, tile)
            try:
                eng.stage_masks(img, seg, onoff, 0)
                score, pred = eng.forward(batch, labels)
                torch.cuda.synchronize()
            finally:
                for i in mains:
                    eng.set_conv_tile(i, -1)
            return score.clone(), pred.clone()

        s_new, p_new = forward(-1)
        s_old, p_old = forward(7)
        assert torch.isfinite(s_new).all()
        assert _same_bits(s_new, s_old) and torch.equal(p_new, p_old)
        for stage in (2, 3, 4):
            i, d3, dd, t2, x = _inputs(eng, stage, batch)
            assert _launch(eng, i, d3, t2, x, batch, -1)[2] == 1 << 13, "layer%d.0 does not take the persistent dual kernel by default" % stage
    finally:
        eng.close()
