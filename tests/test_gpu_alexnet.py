"""AlexNet on the MI355X (pytest -m gpu), through the C-ABI as tests/test_gpu_vgg.py does: the topology, every layer on every tile it
accepts against an fp64 conv of the same split inputs, the unpadded 3x3 stride-2 max pool bit for bit (one case with planes past 2^31
elements), the 11x11 first layer straight from K0, the whole network against the batch-1 fp32 CPU loop and the fp64 restatement
(tests/alexnet_ref.py), position independence of a mask row, the reference-named API and the error paths.

The fp64 yardstick of the per-layer checks runs on the device as an im2col GEMM (F.unfold + matmul in float64, image by image): the
same sum as F.conv2d in fp64.

End-to-end figures measured on one MI355X on the 64 masks of test_alexnet_end_to_end (felzenszwalb fixture, seed 11), which set
SCORE_TOL_TIGHT = 4 x the larger of the first two (2.3e-5), rounded up to one digit (the factor covers other seeds and boxes):
    engine vs fp64 restatement           max |d| = 5.720e-06
    batch-1 fp32 CPU loop vs fp64        max |d| = 2.994e-06
    engine vs batch-1 fp32 CPU loop      max |d| = 6.586e-06
    smallest fp64 top-1 - top-2 logit gap 0.0011 (no mask under 1e-3)"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import alexnet_ref
from gpu_common import accepted_tiles, dev, FALLBACK, LAYER_TOL, merge, ptr, SCORE_TOL, split  # noqa: F401  (dev is a fixture)
from net_harness import check_api, check_conv_layer, check_position_independence, Reference
from network_interpretation_imagenet_amd import _lib, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine, rank_segments
from logits_lens import LogitsLens
from oracle import scorer

pytestmark = pytest.mark.gpu

ARCH = "alexnet"
SCORE_TOL_TIGHT = 3e-5      # from the measurement in the module docstring
CONVS = ["features.0", "features.3", "features.6", "features.8", "features.10", "classifier.1", "classifier.4", "classifier.6"]
MACS = 714188480
BATCHES = (5, 197)          # 197 images of a 13x13 map: 131 pixel tiles of 256, more than one persistent round and not a whole number of them


@pytest.fixture(scope="module")
def eng(mpx_lib, dev):
    e = MaskedForwardEngine(ARCH, device=0).load_state_dict(synth.make_state_dict(ARCH))      # the default max_batch
    yield e
    e.close()


def _felz(golden_dir):
    g = np.load(os.path.join(golden_dir, "felzenszwalb_skimage0183.npz"))
    return g["blobs224/image"], g["blobs224/labels"].astype(np.int64)


# ------------------------------------------------------------------------------------------------
# topology
# ------------------------------------------------------------------------------------------------
def test_alexnet_topology(eng):
    assert eng.max_batch == 512
    assert [d.name.decode() for d in eng.layers] == CONVS
    assert all(d.bn_name.decode() == "" for d in eng.layers)
    shapes = [(d.cin, d.cout, d.ksize, d.stride, d.pad, d.hin, d.hout, d.relu) for d in eng.layers]
    assert shapes == [(3, 64, 11, 4, 2, 224, 55, 1), (64, 192, 5, 1, 2, 27, 27, 1), (192, 384, 3, 1, 1, 13, 13, 1),
                      (384, 256, 3, 1, 1, 13, 13, 1), (256, 256, 3, 1, 1, 13, 13, 1), (256, 4096, 6, 1, 0, 6, 1, 1),
                      (4096, 4096, 1, 1, 0, 1, 1, 1), (4096, 1000, 1, 1, 0, 1, 1, 0)]
    assert eng.layers[0].k_packed == 704 and [d.cout_pad for d in eng.layers[:5]] == [128, 256, 384, 256, 256]
    assert eng.flops_per_forward == 2.0 * MACS
    geo = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert eng._lib.mpx_geometry(eng._h, *[C.byref(v) for v in geo]) == 0 and [v.value for v in geo] == [224, 3, 1000, 1000]
    tiles = [eng._lib.mpx_get_conv_tile(eng._h, i) for i in range(len(CONVS))]
    print("default tiles", dict(zip(CONVS, tiles)))
    # workspace: two 55x55x64 split planes + the NHWC4 staging per slot, plus weights
    per_slot = 2 * 2 * 55 * 55 * 64 * 2 + 2 * 230 * 230 * 4 * 2
    w = sum(2 * d.cout_pad * d.k_packed * 2 for d in eng.layers)
    assert per_slot * 512 + w < eng.workspace_bytes < per_slot * 512 + w + (16 << 20)


# ------------------------------------------------------------------------------------------------
# per layer
# ------------------------------------------------------------------------------------------------
def _ref_layer(sd, d, x_nchw64):
    """fp64 conv + bias (+ ReLU) on the device: [B][cout][ho][ho]."""
    name = d.name.decode()
    dev = x_nchw64.device
    w = sd[name + ".weight"].double().reshape(d.cout, -1).to(dev)
    b = sd[name + ".bias"].double().to(dev)
    out = []
    for i in range(x_nchw64.shape[0]):
        cols = F.unfold(x_nchw64[i:i + 1], d.ksize, padding=d.pad, stride=d.stride)[0]     # [cin*k*k, L], (ci, ky, kx) like the OIHW rows
        out.append((w @ cols + b[:, None]).view(1, d.cout, d.hout, d.hout))
    y = torch.cat(out)
    return F.relu(y) if d.relu else y


def _check(eng, i, batch, tile=-1):
    sd = synth.make_state_dict(ARCH)
    return check_conv_layer(eng, i, batch, lambda d, x64, _r64: _ref_layer(sd, d, x64), tile)[0]


@pytest.mark.parametrize("name", CONVS)
def test_alexnet_every_layer_default_tile(eng, name):
    i = CONVS.index(name)
    tile = eng._lib.mpx_get_conv_tile(eng._h, i)
    for batch in BATCHES:
        ran = _check(eng, i, batch)
        assert ran & ((1 << tile) | (1 << FALLBACK.get(tile, tile))), (name, batch, tile, ran)


@pytest.mark.parametrize("name", CONVS)
def test_alexnet_every_accepted_tile(eng, name):
    i = CONVS.index(name)
    accepted = accepted_tiles(eng, i)
    assert {0, 1, 2, 4, 7} <= set(accepted)
    if name in ("features.6", "features.8", "features.10"):
        assert {6, 12} <= set(accepted)         # the patch kernels take the odd 13x13 maps
    for t in accepted:
        for batch in BATCHES:
            ran = _check(eng, i, batch, tile=t)
            assert ran & ((1 << t) | (1 << FALLBACK.get(t, t))), (name, t, ran)
            if t not in FALLBACK:
                assert ran == 1 << t, (name, t, ran)
    print(name, "accepted tiles", accepted)


@pytest.mark.parametrize("name", ["features.6", "features.8", "features.10"])
def test_alexnet_persistent_patch_kernel_over_whole_rounds(eng, name):
    """197 images of a 13x13 map are 131 pixel tiles x 2 or 3 cout tiles >= 256: the persistent walk itself must run (cout 384 = three
    cout tiles, a grid of 240 workgroups)."""
    i = CONVS.index(name)
    ran = _check(eng, i, 197, tile=12)
    assert ran & (1 << 12), (name, ran)


# ------------------------------------------------------------------------------------------------
# 3x3 stride-2 max pool without padding
# ------------------------------------------------------------------------------------------------
def _pool_input(batch, hin, c, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, hin, hin, c, generator=g) * 3                    # signed
    x[..., : c // 4] = torch.round(x[..., : c // 4])                         # small integers: exact ties everywhere, zeros among them
    x[:, 0:hin - 1:2, 0:hin - 1:2, c // 4: c // 2] = x[:, 1::2, 1::2, c // 4: c // 2]     # equal values inside one window
    x[0, :, :, :8] = -torch.rand(hin, hin, 8, generator=g) - 1               # all-negative windows
    x[-1, :, :, 8:16] = 0                                                    # all-zero windows
    return x


@pytest.mark.parametrize("hin,c,batch", [(55, 64, 3), (27, 192, 5), (13, 256, 41), (7, 8, 2), (3, 16, 1)])
def test_maxpool3x3s2p0_bit_exact(eng, dev, hin, c, batch):
    ho = (hin - 3) // 2 + 1
    xh, xl = split(_pool_input(batch, hin, c, hin + c).to(dev))
    oh = torch.full((batch, ho, ho, c), float("nan"), dtype=torch.float16, device=dev)
    ol = torch.full_like(oh, float("nan"))
    rc = eng._lib.mpx_maxpool3x3s2p0(eng._h, ptr(xh), ptr(xl), ptr(oh), ptr(ol), batch, hin, c, eng._stream())
    _lib.check(eng._h, rc, "mpx_maxpool3x3s2p0")
    torch.cuda.synchronize()
    want = F.max_pool2d(merge(xh, xl).permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1)
    assert tuple(want.shape) == (batch, ho, ho, c)
    assert torch.equal(merge(oh, ol), want)


def test_maxpool3x3s2p0_refuses_bad_shapes(eng, dev):
    z = torch.zeros(64, dtype=torch.float16, device=dev)
    args = (ptr(z), ptr(z), ptr(z), ptr(z))
    assert eng._lib.mpx_maxpool3x3s2p0(eng._h, *args, 1, 1, 8, None) == -1      # hin < 3
    assert eng._lib.mpx_maxpool3x3s2p0(eng._h, *args, 1, 56, 8, None) == -1     # even hin
    assert eng._lib.mpx_maxpool3x3s2p0(eng._h, *args, 1, 55, 12, None) == -1    # c % 8 != 0


def test_maxpool3x3s2p0_planes_past_2_31_elements(eng, dev):
    """11100 images of the 55x55x64 map: 2.149e9 elements per input plane, so input offsets pass 2^31 (8.6 GB of input planes,
    2.0 GB of output planes, allocated and freed here).  Not canonical splits: any (hi, lo) pair is a value."""
    B, hin, c, ho = 11100, 55, 64, 27
    assert B * hin * hin * c > 2 ** 31
    g = torch.Generator(device=dev).manual_seed(9)
    xh = torch.empty(B, hin, hin, c, dtype=torch.float16, device=dev)
    xl = torch.empty_like(xh)
    for lo in range(0, B, 1000):
        xh[lo:lo + 1000] = (torch.randn(xh[lo:lo + 1000].shape, generator=g, device=dev) * 3).half()
        xl[lo:lo + 1000] = (torch.randn(xl[lo:lo + 1000].shape, generator=g, device=dev) * 1e-3).half()
    oh = torch.full((B, ho, ho, c), float("nan"), dtype=torch.float16, device=dev)
    ol = torch.full_like(oh, float("nan"))
    try:
        rc = eng._lib.mpx_maxpool3x3s2p0(eng._h, ptr(xh), ptr(xl), ptr(oh), ptr(ol), B, hin, c, eng._stream())
        _lib.check(eng._h, rc, "mpx_maxpool3x3s2p0")
        torch.cuda.synchronize()
        for lo in list(range(0, B, 1000))[::3] + [B - 100]:         # every third block of 1000 images, and the last images
            hi = min(lo + 1000, B)
            want = F.max_pool2d(merge(xh[lo:hi], xl[lo:hi]).permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1)
            assert torch.equal(merge(oh[lo:hi], ol[lo:hi]), want), lo
    finally:
        del xh, xl, oh, ol
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------
# the first layer straight from K0
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg_kind,m", [("felz", 9), ("grid", 5)])
def test_first_layer_from_stage_masks(eng, dev, golden_dir, seg_kind, m):
    if seg_kind == "felz":
        img, seg = _felz(golden_dir)
        seg = rank_segments(seg)[0].astype(np.int32)
    else:
        img, seg = synth.make_images(1)[0], synth.grid_segments()
    s = int(seg.max()) + 1
    onoff = torch.from_numpy(synth.random_onoff(m, s, seed=m)).to(dev)
    xf = torch.empty(m, 3, 224, 224, dtype=torch.float32, device=dev)
    eng.stage_masks(torch.from_numpy(np.ascontiguousarray(img)).to(dev), torch.from_numpy(np.ascontiguousarray(seg)).to(dev), onoff, 0, xf)
    d = eng.layers[0]
    oh = torch.full((m, 55, 55, 64), float("nan"), dtype=torch.float16, device=dev)
    ol = torch.full_like(oh, float("nan"))
    _lib.check(eng._h, eng._lib.mpx_conv_bn_act(eng._h, 0, None, None, None, None, ptr(oh), ptr(ol), None, m, eng._stream()), "conv")
    torch.cuda.synchronize()
    # the masked normalised images against the CPU staging of oracle.scorer, then the layer against F.conv2d(masked, w, b, 4, 2) + ReLU
    x = scorer.to_tensor_normalize(img)
    masked = alexnet_ref.masked_batch(x, seg, onoff.cpu().numpy())
    assert (xf.cpu().numpy().view(np.int32) == masked.numpy().view(np.int32)).all()       # K0 is bit-exact (tests/test_gpu_parity.py)
    staged = merge(*split(xf)).double()                 # what the staging holds: the masked normalised image rounded to hi + lo
    sd = synth.make_state_dict(ARCH)
    want = F.relu(F.conv2d(staged, sd["features.0.weight"].double().to(dev), sd["features.0.bias"].double().to(dev), 4, 2)).permute(0, 2, 3, 1)
    assert (want - _ref_layer(sd, d, staged).permute(0, 2, 3, 1)).abs().max().item() <= 1e-12      # the per-layer yardstick is that conv
    err = (merge(oh, ol).double() - want).abs().max().item()
    print("first layer from K0 (%s): max err %.3e, scale %.2f" % (seg_kind, err, want.abs().max().item()))
    assert err <= LAYER_TOL * max(want.abs().max().item(), 1.0), err


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
def test_alexnet_end_to_end(eng, dev, golden_dir):
    """Logits lens (tests/logits_lens.py): all 1000 logits of every row against fp64, bound 4 d_L with d_L = the fp32 CPU loop's distance.  Measured on one MI355X: alexnet d_L 1.62e-05, engine 3.28e-05 (2.02)."""
    lens = LogitsLens(ARCH)
    m = 64
    img, seg = _felz(golden_dir)
    sd = synth.make_state_dict(ARCH)
    x = scorer.to_tensor_normalize(img)
    label, prob = alexnet_ref.predict(sd, x)
    assert 0.05 < prob.max() < 0.99 and (prob > 1e-3).sum() >= 3          # non-degenerate softmax
    S = len(np.unique(seg))
    onoff = synth.random_onoff(m, S, seed=11)
    _o, score, pred, logits = eng.score_masks(img, seg, onoff, label, return_logits=True)
    ref_score, ref_pred, ref_logits = alexnet_ref.score_masks_reference_loop(sd, x, seg, onoff, label, return_logits=True)
    s64, logits64 = alexnet_ref.score_masks_fp64(sd, x, seg, onoff, label)
    lens.add("felz", logits, ref_logits, logits64)
    top2 = np.sort(logits64, axis=1)[:, -2:]
    gap = top2[:, 1] - top2[:, 0]
    err_engine = float(np.abs(score.astype(np.float64) - s64).max())
    err_cpu = float(np.abs(ref_score.astype(np.float64) - s64).max())
    err_both = float(np.abs(score.astype(np.float64) - ref_score.astype(np.float64)).max())
    print("alexnet: %d masks, S %d, label %d, scores %.4f..%.4f" % (m, S, label, ref_score.min(), ref_score.max()))
    print("alexnet: max|d| engine vs fp64 %.3e, fp32 CPU loop vs fp64 %.3e, engine vs fp32 CPU loop %.3e, smallest fp64 logit gap %.4f"
          % (err_engine, err_cpu, err_both, gap.min()))
    assert ref_score.max() - ref_score.min() > 0.05                        # the masks move the score
    assert err_both <= SCORE_TOL
    assert err_both <= SCORE_TOL_TIGHT and err_engine <= SCORE_TOL_TIGHT
    clear = gap > 1e-3
    assert (~clear).sum() <= m // 10
    assert (pred[clear] == logits64.argmax(1)[clear]).all()
    assert (pred == ref_pred)[clear].all()
    p_label, _ = eng.predict(img)
    assert p_label == label
    lens.check()


def test_a_mask_row_scores_the_same_bits_wherever_it_sits(eng, dev, golden_dir):
    check_position_independence(eng, *_felz(golden_dir),
                                (8, ((1, 0, (0,)), (37, 41, (0, 5, 36)), (300, 42, (1, 150, 299)), (512, 43, (0, 255, 511)), (700, 44, (3, 511, 512, 699)))))


# ------------------------------------------------------------------------------------------------
# API and errors
# ------------------------------------------------------------------------------------------------
def test_api_on_an_alexnet_engine(eng, dev, golden_dir):
    ref = Reference(alexnet_ref, synth.make_state_dict(ARCH))
    check_api(eng, ref, *_felz(golden_dir), rows=24, tol=SCORE_TOL_TIGHT, windows=(0, 3, 9), heatmaps=1, predict=False, table_step=7, validate=40)


def test_alexnet_error_paths(eng, mpx_lib, dev):
    with pytest.raises(ValueError):
        MaskedForwardEngine(ARCH, max_batch=2, device=0, stem="table")
    with pytest.raises(ValueError):
        eng.score_masks(synth.make_images(1)[0], synth.grid_segments(), synth.random_onoff(2, 196), 0, stem="table")
    with pytest.raises(ValueError):
        eng.stem_planes(1)
    z = torch.zeros(224, 224, dtype=torch.int32, device=dev)
    im = torch.zeros(224, 224, 3, dtype=torch.uint8, device=dev)
    on = torch.ones(1, 1, dtype=torch.uint8, device=dev)
    mean = (C.c_float * 3)(*scorer.MEAN)
    std = (C.c_float * 3)(*scorer.STD)
    assert eng._lib.mpx_stem_table_build(eng._h, ptr(im), None, ptr(z), 1, mean, std, None) == -2
    assert eng._lib.mpx_stem_table_apply(eng._h, ptr(on), 1, 1, 0, None) == -2
    assert eng._lib.mpx_stem_conv_maxpool(eng._h, ptr(z), ptr(z), 1, None) == -2
    hi, lo = C.c_void_p(1), C.c_void_p(1)
    assert eng._lib.mpx_stem_planes(eng._h, C.byref(hi), C.byref(lo)) == 0 and not hi.value and not lo.value
    for bad in (4001, 4099):
        h = C.c_void_p()
        assert mpx_lib.mpx_create(bad, 2, 0, C.byref(h)) == -1 and not h.value
    fresh = MaskedForwardEngine(ARCH, max_batch=2, device=0)
    try:
        with pytest.raises(KeyError):
            fresh.load_state_dict(synth.make_state_dict("resnet18"))
        with pytest.raises(ValueError):
            fresh.load_state_dict(synth.make_state_dict("vgg11"))       # features.0.weight is [64][3][3][3] there
    finally:
        fresh.close()
