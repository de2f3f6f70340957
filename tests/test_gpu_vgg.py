"""The VGG family on the MI355X (pytest -m gpu), through the C-ABI as tests/test_gpu_parity.py does: every conv layer of vgg16 and
vgg16_bn (and vgg11's first layer) against an fp64 conv of the same split inputs, the 2x2 max pool bit for bit, the first layer
straight from K0, whole networks against the batch-1 fp32 CPU loop (tests/vgg_ref.py), a batch whose 224x224x64 planes pass 4 GiB,
the reference-named API and the error paths.

The fp64 yardstick of the per-layer checks runs on the device as an im2col GEMM (F.unfold + matmul in float64, image by image): the
same sum as F.conv2d in fp64, at a cost that lets every layer run at ragged batches."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vgg_ref
from gpu_common import accepted_tiles, dev, FALLBACK, LAYER_TOL, merge, ptr, SCORE_TOL, split  # noqa: F401  (dev is a fixture)
from net_harness import check_conv_layer
from network_interpretation_imagenet_amd import _lib, api, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine
from logits_lens import LogitsLens
from oracle import scorer

pytestmark = pytest.mark.gpu

SCORE_TOL_TIGHT = 2e-5
_ENGINES = {}


@pytest.fixture(scope="module")
def engines(mpx_lib, dev):
    yield _ENGINES
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _engine(engines, arch, max_batch=100):
    key = (arch, max_batch)
    if key not in engines:
        engines[key] = MaskedForwardEngine(arch, max_batch=max_batch, device=0).load_state_dict(synth.make_state_dict(arch))
    return engines[key]


# ------------------------------------------------------------------------------------------------
# per layer
# ------------------------------------------------------------------------------------------------
def _ref_layer(sd, d, x_nchw64):
    """fp64 conv (+ bias) (+ BN) (+ ReLU) on the device: [B][cout][ho][ho]."""
    name, bn = d.name.decode(), d.bn_name.decode()
    dev = x_nchw64.device
    w = sd[name + ".weight"].double().reshape(d.cout, -1).to(dev)
    b = sd[name + ".bias"].double().to(dev)
    out = []
    for i in range(x_nchw64.shape[0]):
        cols = F.unfold(x_nchw64[i:i + 1], d.ksize, padding=d.pad)[0]        # [cin*k*k, L], (ci, ky, kx) like the OIHW rows
        out.append((w @ cols + b[:, None]).view(1, d.cout, d.hout, d.hout))
    y = torch.cat(out)
    if bn:
        g = lambda s: sd["%s.%s" % (bn, s)].double().to(dev).view(1, -1, 1, 1)
        y = (y - g("running_mean")) * (g("weight") / torch.sqrt(g("running_var") + 1e-5)) + g("bias")
    return F.relu(y) if d.relu else y


def _check(eng, i, batch, tile=-1):
    sd = synth.make_state_dict(eng.arch)
    return check_conv_layer(eng, i, batch, lambda d, x64, _r64: _ref_layer(sd, d, x64), tile, fields=None)[0]


VGG16_CONVS = ["features.%d" % i for i in (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)] + ["classifier.0", "classifier.3", "classifier.6"]
VGG16_BN_CONVS = ["features.%d" % i for i in (0, 3, 7, 10, 14, 17, 20, 24, 27, 30, 34, 37, 40)] + ["classifier.0", "classifier.3", "classifier.6"]


def test_vgg16_topology_and_default_tiles(engines):
    for arch, names in (("vgg16", VGG16_CONVS), ("vgg16_bn", VGG16_BN_CONVS)):
        eng = _engine(engines, arch)
        assert [d.name.decode() for d in eng.layers] == names
        bns = [d.bn_name.decode() for d in eng.layers]
        if arch == "vgg16":
            assert all(b == "" for b in bns)
        else:
            assert bns[:13] == ["features.%d" % (int(n.split(".")[1]) + 1) for n in names[:13]] and bns[13:] == ["", "", ""]
        tiles = [eng._lib.mpx_get_conv_tile(eng._h, i) for i in range(16)]
        print(arch, "default tiles", dict(zip(names, tiles)))
        assert tiles[0] == 1 and tiles[1] == 1
    eng = _engine(engines, "vgg16")
    macs = sum(d.hout * d.hout * d.cout * d.cin * d.ksize * d.ksize for d in eng.layers)
    assert eng.flops_per_forward == 2.0 * macs
    assert abs(eng.flops_per_forward / 30.94e9 - 1) < 0.01
    geo = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert eng._lib.mpx_geometry(eng._h, *[C.byref(v) for v in geo]) == 0 and [v.value for v in geo] == [224, 3, 1000, 1000]


@pytest.mark.parametrize("arch,name", [(a, n) for a, ns in (("vgg16", VGG16_CONVS), ("vgg16_bn", VGG16_BN_CONVS)) for n in ns]
                         + [("vgg11", "features.0")])
def test_vgg_every_layer_default_tile(engines, arch, name):
    eng = _engine(engines, arch)
    i = [d.name.decode() for d in eng.layers].index(name)
    tile = eng._lib.mpx_get_conv_tile(eng._h, i)
    for batch in (1, 3, 41):
        ran = _check(eng, i, batch)
        assert ran & ((1 << tile) | (1 << FALLBACK.get(tile, tile))), (name, batch, tile, ran)


@pytest.mark.parametrize("name", VGG16_CONVS)
def test_vgg16_every_accepted_tile(engines, name):
    eng = _engine(engines, "vgg16")
    i = [d.name.decode() for d in eng.layers].index(name)
    accepted = accepted_tiles(eng, i)
    assert {0, 1, 2, 4, 7} <= set(accepted)
    for t in accepted:
        ran = _check(eng, i, 3, tile=t)
        assert ran & ((1 << t) | (1 << FALLBACK.get(t, t))), (name, t, ran)
        if t not in FALLBACK:
            assert ran == 1 << t, (name, t, ran)
    print(name, "accepted tiles", accepted)


@pytest.mark.parametrize("name,tile,batch", [("features.24", 12, 97), ("features.17", 12, 67), ("features.21", 12, 41)])
def test_vgg16_persistent_patch_kernel_over_whole_rounds(engines, name, tile, batch):
    """A batch that fills at least one persistent round of the 3x3 patch kernel: the persistent walk itself must run."""
    eng = _engine(engines, "vgg16")
    i = [d.name.decode() for d in eng.layers].index(name)
    if eng._lib.mpx_set_conv_tile(eng._h, i, tile) != 0:
        eng._lib.mpx_set_conv_tile(eng._h, i, -1)
        pytest.fail("%s does not take tile %d" % (name, tile))
    eng._lib.mpx_set_conv_tile(eng._h, i, -1)
    ran = _check(eng, i, batch, tile=tile)
    assert ran & (1 << tile), (name, ran)


# ------------------------------------------------------------------------------------------------
# 2x2 max pool
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hin,c,batch", [(224, 64, 3), (112, 128, 5), (56, 256, 1), (28, 512, 7), (14, 512, 41)])
def test_maxpool2x2s2_bit_exact(engines, dev, hin, c, batch):
    eng = _engine(engines, "vgg16")
    g = torch.Generator().manual_seed(hin + c)
    x = torch.randn(batch, hin, hin, c, generator=g) * 3
    x[:, ::2, ::2, : c // 2] = x[:, 1::2, 1::2, : c // 2]      # ties: equal values in one window
    x[0, :, :, :8] = -torch.rand(hin, hin, 8, generator=g) - 1  # all-negative windows
    xh, xl = split(x.to(dev))
    oh = torch.full((batch, hin // 2, hin // 2, c), float("nan"), dtype=torch.float16, device=dev)
    ol = torch.full_like(oh, float("nan"))
    rc = eng._lib.mpx_maxpool2x2s2(eng._h, ptr(xh), ptr(xl), ptr(oh), ptr(ol), batch, hin, c, eng._stream())
    _lib.check(eng._h, rc, "mpx_maxpool2x2s2")
    torch.cuda.synchronize()
    want = F.max_pool2d(merge(xh, xl).permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert torch.equal(merge(oh, ol), want)
    assert eng._lib.mpx_maxpool2x2s2(eng._h, ptr(xh), ptr(xl), ptr(oh), ptr(ol), batch, hin + 1, c, None) == -1
    assert eng._lib.mpx_maxpool2x2s2(eng._h, ptr(xh), ptr(xl), ptr(oh), ptr(ol), batch, hin, c - 4, None) == -1


# ------------------------------------------------------------------------------------------------
# the first layer straight from K0
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg_kind,m", [("felz", 9), ("grid", 5)])
def test_first_layer_from_stage_masks(engines, dev, golden_dir, seg_kind, m):
    eng = _engine(engines, "vgg16_bn")
    img = synth.make_images(1)[0]
    seg = (np.load(os.path.join(golden_dir, "segments_blobs.npz"))["segments"][0].astype(np.int32) if seg_kind == "felz"
           else synth.grid_segments())
    s = int(seg.max()) + 1
    onoff = torch.from_numpy(synth.random_onoff(m, s, seed=m)).to(dev)
    xf = torch.empty(m, 3, 224, 224, dtype=torch.float32, device=dev)
    eng.stage_masks(torch.from_numpy(img).to(dev), torch.from_numpy(seg).to(dev), onoff, 0, xf)
    d = eng.layers[0]
    oh = torch.full((m, 224, 224, 64), float("nan"), dtype=torch.float16, device=dev)
    ol = torch.full_like(oh, float("nan"))
    _lib.check(eng._h, eng._lib.mpx_conv_bn_act(eng._h, 0, None, None, None, None, ptr(oh), ptr(ol), None, m, eng._stream()), "conv")
    torch.cuda.synchronize()
    staged = merge(*split(xf)).double()                 # what the staging holds: the masked normalised image rounded to hi + lo
    want = _ref_layer(synth.make_state_dict("vgg16_bn"), d, staged).permute(0, 2, 3, 1)
    err = (merge(oh, ol).double() - want).abs().max().item()
    assert err <= LAYER_TOL * max(want.abs().max().item(), 1.0), err


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,m", [("vgg11", 16), ("vgg16", 20), ("vgg16_bn", 20), ("vgg19_bn", 16)])
def test_vgg_end_to_end_vs_batch1_cpu_loop(engines, dev, golden_dir, arch, m):
    """Logits lens (tests/logits_lens.py): all 1000 logits of every row against fp64, bound 4 d_L with d_L = the fp32 CPU loop's distance.  Measured on one MI355X: vgg11 d_L 1.64e-05, engine 3.24e-05 (1.97); vgg16 d_L 1.67e-05, engine 3.83e-05 (2.30);
    vgg16_bn d_L 1.31e-05, engine 3.00e-05 (2.30); vgg19_bn d_L 1.26e-05, engine 3.59e-05 (2.85)."""
    g = np.load(os.path.join(golden_dir, "segments_blobs.npz"))
    img = synth.make_images(2, seed=int(g["image_seed"]))[0]
    seg = g["segments"][0].astype(np.int64)
    sd = synth.make_state_dict(arch)
    x = scorer.to_tensor_normalize(img)
    label, prob = vgg_ref.predict(sd, arch, x)
    assert 0.05 < prob.max() < 0.99 and (prob > 1e-3).sum() >= 3          # non-degenerate softmax
    S = len(np.unique(seg))
    onoff = synth.random_onoff(m, S, seed=11)
    eng = _engine(engines, arch, 100 if arch in ("vgg16", "vgg16_bn") else 32)
    _o, score, pred, logits = eng.score_masks(img, seg, onoff, label, return_logits=True)
    ref_score, ref_pred, ref_logits = vgg_ref.score_masks_reference_loop(sd, arch, x, seg, onoff, label, return_logits=True)
    err = float(np.abs(score.astype(np.float64) - ref_score).max())
    print("%s: %d masks, label %d, max|d| %.3e, scores %.4f..%.4f" % (arch, m, label, err, ref_score.min(), ref_score.max()))
    assert err <= SCORE_TOL and err <= SCORE_TOL_TIGHT
    assert (pred == ref_pred).all()
    p_label, _ = eng.predict(img)
    assert p_label == label
    _s64, logits64 = vgg_ref.score_masks_fp64(sd, arch, x, seg, onoff, label)
    lens = LogitsLens(arch)
    lens.add("felz", logits, ref_logits, logits64)
    lens.check()


def test_vgg16_batch_past_4gib_planes(engines, dev):
    """max_batch 672: one fp16 plane of the 224x224x64 maps is 672 * 3.2 M elements > 2^31 (4.3 GB)."""
    arch = "vgg16"
    sd = synth.make_state_dict(arch)
    B = 672
    big = MaskedForwardEngine(arch, max_batch=B, device=0).load_state_dict(sd)
    try:
        assert B * 224 * 224 * 64 > 2 ** 31
        small = _engine(engines, arch, 24)
        img = synth.make_images(1, seed=5)[0]
        seg = synth.grid_segments()
        onoff = synth.random_onoff(B, 196, seed=21)
        onoff[0] = 1
        onoff[400] = onoff[3]
        onoff[671] = onoff[3]
        label, _ = big.predict(img)
        _o, score, pred, logits = big.score_masks(img, seg, onoff, label, return_logits=True)
        assert np.isfinite(logits).all()
        assert score[3] == score[400] == score[671] and pred[3] == pred[400] == pred[671]
        _o, s24, p24 = small.score_masks(img, seg, onoff[:24], label)
        assert np.array_equal(s24, score[:24]) and np.array_equal(p24, pred[:24])
        # the all-ones mask is the unmasked image
        p_label, prob = big.predict(img)
        assert p_label == pred[0] == label and abs(float(score[0]) - float(prob[label])) <= 1e-6
    finally:
        big.close()


# ------------------------------------------------------------------------------------------------
# API and errors
# ------------------------------------------------------------------------------------------------
def test_api_on_a_vgg16_engine(engines, dev, golden_dir):
    arch = "vgg16"
    sd = synth.make_state_dict(arch)
    g = np.load(os.path.join(golden_dir, "segments_blobs.npz"))
    img = synth.make_images(2, seed=int(g["image_seed"]))[0]
    seg = g["segments"][0].astype(np.int64)
    x = scorer.to_tensor_normalize(img)
    label, _ = vgg_ref.predict(sd, arch, x)
    eng = _engine(engines, arch)
    api.configure(eval_img_index=1, segmenter=lambda _img_show: seg, mask_dir=None, seed=None)
    loader = [(x[None], torch.tensor([label]))]
    for f in (0, 3, 9):
        got = api.sample_loss([f], loader, eng, None)
        want, _ = scorer_score_one(sd, arch, scorer.apply_mask(x, scorer.window_mask_u8(seg, f)), label)
        assert abs(float(got) - float(want)) <= SCORE_TOL_TIGHT
    many = api.validate_many(list(loader), eng, None, [1], num_mask_samples=40, rng=random.Random(3))
    one = api.validate(list(loader), eng, None, 1, num_mask_samples=40, rng=random.Random(3))
    assert many == {1: one}


def scorer_score_one(sd, arch, masked_chw, label):
    with torch.no_grad():
        logits = vgg_ref.forward(vgg_ref.cast(sd, torch.float32), torch.from_numpy(masked_chw[None]), arch)
    return F.softmax(logits, 1).numpy()[0][label], int(logits.argmax(1)[0])


def test_vgg_error_paths(engines, mpx_lib, dev):
    eng = _engine(engines, "vgg16")
    with pytest.raises(ValueError):
        MaskedForwardEngine("vgg16", max_batch=2, device=0, stem="table")
    with pytest.raises(ValueError, match="max_batch"):
        MaskedForwardEngine("vgg16")                                    # no default size for a VGG engine
    assert eng.stem == "conv" and eng.stem_for_rows(4096) == "conv"
    with pytest.raises(ValueError):
        eng.stem_planes(1)
    z = torch.zeros(224, 224, dtype=torch.int32, device=dev)
    im = torch.zeros(224, 224, 3, dtype=torch.uint8, device=dev)
    mean = (C.c_float * 3)(*scorer.MEAN)
    std = (C.c_float * 3)(*scorer.STD)
    assert eng._lib.mpx_stem_table_build(eng._h, ptr(im), None, ptr(z), 1, mean, std, None) == -2
    assert eng._lib.mpx_stem_conv_maxpool(eng._h, ptr(z), ptr(z), 1, None) == -2
    hi, lo = C.c_void_p(1), C.c_void_p(1)
    assert eng._lib.mpx_stem_planes(eng._h, C.byref(hi), C.byref(lo)) == 0 and not hi.value and not lo.value
    h = C.c_void_p()
    assert mpx_lib.mpx_create(3014, 2, 0, C.byref(h)) == -1
    fresh = MaskedForwardEngine("vgg16", max_batch=2, device=0)
    try:
        with pytest.raises(KeyError):
            fresh.load_state_dict(synth.make_state_dict("resnet18"))
    finally:
        fresh.close()
    # workspace: two 224x224x64 split planes + the NHWC4 staging per slot, plus weights
    per_slot = 2 * 2 * 224 * 224 * 64 * 2 + 2 * 230 * 230 * 4 * 2
    w = sum(2 * d.cout_pad * d.k_packed * 2 for d in eng.layers)
    assert per_slot * 100 + w < eng.workspace_bytes < per_slot * 100 + w + (16 << 20)
