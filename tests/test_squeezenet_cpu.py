"""SqueezeNet 1.1 without a GPU: the synthetic state_dict with torchvision's 52 keys in torchvision's order, the parameter and MAC counts,
the fp64 / fp32 CPU restatement (tests/squeezenet_ref.py) against an independent nn.Module build with ceil-mode pools, the floor-mode pools
giving the same maps, the arch ids, the C-ABI surface, and the statistics of the synthetic network on exactly the rows the GPU test scores."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import netref
import squeezenet_ref
from network_interpretation_imagenet_amd import _lib, engine, synth
from oracle import scorer

ARCH = "squeezenet1_1"
FIRES = ((3, 64, 16, 64), (4, 128, 16, 64), (6, 128, 32, 128), (7, 256, 32, 128), (9, 256, 48, 192), (10, 384, 48, 192),
         (11, 384, 64, 256), (12, 512, 64, 256))
PARAMS = 1235496            # torchvision's parameter count
MACS = 349151936            # the 26 convs
NEW_SYMBOLS = ("mpx_conv_out_slice", "mpx_global_avgpool_logits")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _expected_keys():
    """models.squeezenet1_1().state_dict(): key -> shape, in module order, written out from the Fire table."""
    out = [("features.0.weight", (64, 3, 3, 3)), ("features.0.bias", (64,))]
    for n, cin, s, e in FIRES:
        p = "features.%d." % n
        out += [(p + "squeeze.weight", (s, cin, 1, 1)), (p + "squeeze.bias", (s,)),
                (p + "expand1x1.weight", (e, s, 1, 1)), (p + "expand1x1.bias", (e,)),
                (p + "expand3x3.weight", (e, s, 3, 3)), (p + "expand3x3.bias", (e,))]
    return out + [("classifier.1.weight", (1000, 512, 1, 1)), ("classifier.1.bias", (1000,))]


def test_synth_squeezenet_state_dict_has_torchvisions_keys_order_and_shapes():
    sd = synth.make_state_dict(ARCH)
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == _expected_keys()
    assert len(sd) == 52 and list(sd) == list(synth.make_squeezenet_state_dict())
    assert all(v.dtype == torch.float32 for v in sd.values())
    assert sum(v.numel() for v in sd.values()) == PARAMS == squeezenet_ref.PARAMS
    assert tuple(synth.SQUEEZENET_FIRES) == FIRES == tuple(squeezenet_ref.FIRES)
    assert synth.SQUEEZENET_SEED_OFFSET + 7 == 79
    other = synth.make_squeezenet_state_dict(seed=8)
    assert not torch.equal(other["features.0.weight"], sd["features.0.weight"])


def test_macs_and_layer_counts_are_the_known_answers():
    """Counted here from the Fire table alone, then compared with the restatement's topology (which the GPU test compares with the engine's
    list and mpx_flops_per_forward = 2 x this)."""
    macs = 111 * 111 * 64 * 3 * 9
    assert macs == 21290688
    h, n_conv, prev = 111, 1, 64
    for n, cin, s, e in FIRES:
        if n in (3, 6, 9):
            assert (h - 3) % 2 == 0                       # ceil mode = floor mode, every window inside the map
            h = (h - 3) // 2 + 1
        assert cin == prev
        macs += h * h * (cin * s + s * e + 9 * s * e)
        n_conv += 3
        prev = 2 * e
    assert (h, prev) == (13, 512)
    macs += 13 * 13 * 512 * 1000
    assert 13 * 13 * 512 * 1000 == 86528000
    n_conv += 1
    assert macs == MACS == squeezenet_ref.MACS == squeezenet_ref.macs()
    convs = squeezenet_ref.topology()
    assert n_conv == 26 == len(convs) and convs[-1][0] == "classifier.1" and convs[-1][9] == 1
    assert len({c[0] for c in convs}) == 26
    # the distinct conv shapes: the stem, 8 squeeze, 4 + 4 expand, the classifier
    assert len({(c[2], c[3], c[4], c[7]) for c in convs}) == 18
    assert sorted({c[3] for c in convs if c[3] % 32 and c[0] != "classifier.1"}) == [16, 48]
    assert max(c[3] * c[8] * c[8] for c in convs) == 64 * 111 * 111            # the largest map of one conv: the stem's
    planes = [(c[0], p * c[8] * c[8]) for c, (p, _o) in zip(convs, squeezenet_ref.out_slices())]
    assert max(n for name, n in planes if "expand" in name) == 128 * 55 * 55                  # the largest concatenation
    assert max(n for _name, n in planes) == 64 * 111 * 111                                    # every output fits a buffer of the stem's size
    sl = squeezenet_ref.out_slices()
    assert sl[0] == (64, 0) and sl[1:4] == [(32, 0), (128, 0), (128, 64)] and sl[13:16] == [(64, 0), (384, 0), (384, 192)] and sl[-1] == (1000, 0)


def test_squeezenet_arch_ids():
    assert engine.ARCH_IDS[ARCH] == 7011
    ids = list(engine.ARCH_IDS.values())
    assert len(ids) == len(set(ids))
    assert "squeezenet1_0" not in engine.ARCH_IDS
    with pytest.raises(ValueError, match="AlexNet"):
        engine.MaskedForwardEngine("squeezenet1_0")


@pytest.mark.parametrize("arch_id", [7000, 7010, 7012, 7999])
def test_unknown_squeezenet_id_is_refused(mpx_lib, arch_id):
    """mpx_create rejects the id before it touches a device."""
    h = C.c_void_p()
    assert mpx_lib.mpx_create(arch_id, 4, 0, C.byref(h)) == -1 and not h.value


def test_new_c_abi_symbols_are_in_the_header_the_binding_and_the_library(mpx_lib):
    netref.assert_c_abi_symbols(mpx_lib, "MPX_ARCH_SQUEEZENET 7000", NEW_SYMBOLS)
    # every entry refuses a null engine before it touches a device
    a, b = C.c_int(), C.c_int()
    assert mpx_lib.mpx_conv_out_slice(None, 0, C.byref(a), C.byref(b)) == -1
    assert mpx_lib.mpx_global_avgpool_logits(None, None, None, None, 1, 169, 1000, 1000, None) == -1
    # mpx_conv_desc keeps its layout
    assert C.sizeof(_lib.ConvDesc) == 48 + 48 + 11 * 4


# ------------------------------------------------------------------------------------------------
# the restatement against an independent nn.Module build
# ------------------------------------------------------------------------------------------------
class _Fire(nn.Module):
    def __init__(self, inplanes, squeeze_planes, expand1x1_planes, expand3x3_planes):
        super().__init__()
        self.squeeze = nn.Conv2d(inplanes, squeeze_planes, kernel_size=1)
        self.expand1x1 = nn.Conv2d(squeeze_planes, expand1x1_planes, kernel_size=1)
        self.expand3x3 = nn.Conv2d(squeeze_planes, expand3x3_planes, kernel_size=3, padding=1)

    def forward(self, x):
        x = torch.relu(self.squeeze(x))
        return torch.cat([torch.relu(self.expand1x1(x)), torch.relu(self.expand3x3(x))], 1)


class _SqueezeNet11(nn.Module):
    """torchvision's module tree (same names, so load_state_dict(strict=True) is the check of the key set), written independently of
    squeezenet_ref: nn.Sequential with nn.MaxPool2d(ceil_mode=True), as torchvision builds it."""

    def __init__(self):
        super().__init__()
        self.features = nn.Sequential(
            nn.Conv2d(3, 64, kernel_size=3, stride=2), nn.ReLU(inplace=True),
            nn.MaxPool2d(kernel_size=3, stride=2, ceil_mode=True), _Fire(64, 16, 64, 64), _Fire(128, 16, 64, 64),
            nn.MaxPool2d(kernel_size=3, stride=2, ceil_mode=True), _Fire(128, 32, 128, 128), _Fire(256, 32, 128, 128),
            nn.MaxPool2d(kernel_size=3, stride=2, ceil_mode=True), _Fire(256, 48, 192, 192), _Fire(384, 48, 192, 192),
            _Fire(384, 64, 256, 256), _Fire(512, 64, 256, 256))
        self.classifier = nn.Sequential(nn.Dropout(p=0.5), nn.Conv2d(512, 1000, kernel_size=1), nn.ReLU(inplace=True),
                                        nn.AdaptiveAvgPool2d((1, 1)))

    def forward(self, x):
        return torch.flatten(self.classifier(self.features(x)), 1)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_restatement_matches_an_nn_module_build(dtype):
    sd = synth.make_state_dict(ARCH)
    model = _SqueezeNet11()
    model.load_state_dict(sd, strict=True)
    model.to(dtype).eval()
    g = torch.Generator().manual_seed(2)
    x = torch.cat([scorer.to_tensor_normalize(synth.make_images(2)[1])[None], torch.randn(1, 3, 224, 224, generator=g)]).to(dtype)
    sdt = squeezenet_ref.cast(sd, dtype)
    with torch.no_grad():
        want = model(x)
        trace, trace_floor = [], []
        got = squeezenet_ref.forward(sdt, x, trace)
        got_floor = squeezenet_ref.forward(sdt, x, trace_floor, ceil_mode=False)
    assert tuple(got.shape) == (2, 1000)
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    print("%s %s: max |d| %.3e of logit scale %.2f" % (ARCH, dtype, err, scale))
    assert scale > 1.0 and err <= 1e-5 * scale
    # the floor-mode pools give the same maps, bit for bit: 111 -> 55 -> 27 -> 13
    assert torch.equal(got, got_floor)
    assert [n for n, _t in trace] == ["features.%d" % k for k in (0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)]
    for (name, t), (_n, tf) in zip(trace, trace_floor):
        assert torch.equal(t, tf), name
    sides = dict((n, t.shape[-1]) for n, t in trace)
    assert [sides["features.%d" % k] for k in (0, 2, 5, 8, 12)] == [111, 55, 27, 13, 13]
    assert [t.shape[1] for n, t in trace if n in ("features.4", "features.7", "features.10", "features.12")] == [128, 256, 384, 512]


def _rows(golden_dir, kind):
    """(unmasked softmax row, fp64 scores, fp64 logits) of the rows of one end-to-end case."""
    sd = synth.make_state_dict(ARCH)
    m, seed = {k: (m, s) for k, m, s in squeezenet_ref.E2E_CASES}[kind]
    img, seg = squeezenet_ref.e2e_inputs(golden_dir, kind)
    x = scorer.to_tensor_normalize(img)
    trace = []
    with torch.no_grad():
        logits = squeezenet_ref.forward(squeezenet_ref.cast(sd, torch.float64), x[None].double(), trace)
    p = F.softmax(logits, 1)[0]
    onoff = synth.random_onoff(m, len(np.unique(seg)), seed=seed)
    s64, logits64 = squeezenet_ref.score_masks_fp64(sd, x, seg, onoff, int(p.argmax()))
    return p, s64, logits64, trace


@pytest.mark.parametrize("kind", [c[0] for c in squeezenet_ref.E2E_CASES])
def test_synthetic_squeezenet_statistics_on_the_rows_the_gpu_test_scores(golden_dir, kind):
    """The trunk neither dies nor blows up, the unmasked softmax is peaked but unsaturated (what the GPU test asserts before it scores), the
    masks move the score, and on EVERY mask row of squeezenet_ref.E2E_CASES the fp64 top-two logit margin is >= 1e-3: the GPU test then
    compares the argmax of every row, none excluded."""
    p, s64, logits64, trace = _rows(golden_dir, kind)
    rms = [t.pow(2).mean().sqrt().item() for _n, t in trace]
    print("%s %s: map rms %.3f .. %.3f, top softmax %.4f, %d classes over 1e-3" % (ARCH, kind, min(rms), max(rms), p.max().item(), int((p > 1e-3).sum())))
    assert min(rms) > 0.05 and max(rms) < 50.0, (min(rms), max(rms))
    assert 0.05 <= p.max().item() <= 0.95
    top2 = np.sort(logits64, axis=1)[:, -2:]
    gap = top2[:, 1] - top2[:, 0]
    print("%s %s: %d rows, scores %.4f .. %.4f, smallest fp64 top-two margin %.4f" % (ARCH, kind, len(s64), s64.min(), s64.max(), gap.min()))
    assert gap.min() >= 1e-3                                # every row, none excluded
    assert s64.max() - s64.min() > 0.01                     # the masks move the score


@pytest.mark.parametrize("kind", [c[0] for c in squeezenet_ref.E2E_CASES])
def test_weight_conditions_on_every_row_the_gpu_test_scores(golden_dir, kind):
    """On EVERY masked row the GPU test scores the softmax peak lies in [0.05, 0.95] and the fp64 top-two logit gap is >= 1e-3, with plain
    He-normal weights and N(0, 0.05) biases on every conv, classifier.1 included, at the default seed (torch generator seed synth.SQUEEZENET_SEED_OFFSET + 7 = 79).
    Figures (fp64, this file's rows): grid, 8 rows: peak 0.69 .. 0.77, smallest gap 1.45; felzenszwalb, 20 rows: peak 0.10 .. 0.64, smallest
    gap 0.76.  The felzenszwalb rows of the `blobs` picture are heavily masked and give much flatter logits than the unmasked picture (0.67),
    which is why the draw matters: at generator seed 7 their peaks are 0.013 .. 0.082 (the grid rows' 0.15 .. 0.23), and of generator seeds 0 .. 79 only 79 meets
    the condition on all 28 rows (synth.py has the survey)."""
    _p, _s64, logits64, _trace = _rows(golden_dir, kind)
    peak = F.softmax(torch.from_numpy(logits64), 1).max(1)[0].numpy()
    top2 = np.sort(logits64, axis=1)[:, -2:]
    gap = top2[:, 1] - top2[:, 0]
    print("%s %s: %d rows, softmax peak %.4f .. %.4f (%d rows under 0.05), smallest fp64 top-two gap %.4f"
          % (ARCH, kind, len(peak), peak.min(), peak.max(), int((peak < 0.05).sum()), gap.min()))
    assert gap.min() >= 1e-3
    assert 0.05 <= peak.min() and peak.max() <= 0.95
