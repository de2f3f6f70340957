"""AlexNet without a GPU: the synthetic state_dict with torchvision's keys, the two-run packing of the 11x11 first layer, classifier.1 as
a 6x6 conv, the C-ABI surface (mpx_maxpool3x3s2p0, arch ids), and the fp64 CPU restatement (tests/alexnet_ref.py) against an
independent nn.Sequential build."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import alexnet_ref
from network_interpretation_imagenet_amd import _lib, engine, synth
from oracle import scorer

# models.alexnet().state_dict(): key -> shape
ALEXNET_SHAPES = [
    ("features.0.weight", (64, 3, 11, 11)), ("features.0.bias", (64,)),
    ("features.3.weight", (192, 64, 5, 5)), ("features.3.bias", (192,)),
    ("features.6.weight", (384, 192, 3, 3)), ("features.6.bias", (384,)),
    ("features.8.weight", (256, 384, 3, 3)), ("features.8.bias", (256,)),
    ("features.10.weight", (256, 256, 3, 3)), ("features.10.bias", (256,)),
    ("classifier.1.weight", (4096, 9216)), ("classifier.1.bias", (4096,)),
    ("classifier.4.weight", (4096, 4096)), ("classifier.4.bias", (4096,)),
    ("classifier.6.weight", (1000, 4096)), ("classifier.6.bias", (1000,)),
]


def test_synth_alexnet_state_dict_has_torchvisions_keys_and_shapes():
    sd = synth.make_state_dict("alexnet")
    assert len(sd) == 16
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == ALEXNET_SHAPES
    assert all(v.dtype == torch.float32 for v in sd.values())


def test_alexnet_arch_id():
    assert engine.ARCH_IDS["alexnet"] == 4000
    assert sum(1 for v in engine.ARCH_IDS.values() if v == 4000) == 1


def test_unsupported_arch_text_names_alexnet():
    with pytest.raises(ValueError, match="AlexNet"):
        engine.MaskedForwardEngine("squeezenet1_0")


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _unpacked(planes_hi, planes_lo, rows, K):
    """[rows][K] f64 = hi + lo of the piece-major packed planes (include/mpx.h, mpx_pack_conv_weights)."""
    row = np.arange(rows)[:, None]
    k = np.arange(K)[None, :]
    r = row % 16
    at = ((((row // 16) * (K // 32) + k // 32) * 16 + r) * 4 + (((k // 8) % 4) ^ ((r // 8) * 2))) * 8 + k % 8
    return planes_hi.ravel()[at].view(np.float16).astype(np.float64) + planes_lo.ravel()[at].view(np.float16).astype(np.float64)


def test_pack_first_alexnet_layer_two_run_layout(mpx_lib):
    """cin == 3, ksize == 11, k_packed == 704: tap (ky, px, c) at K position ky*64 + px*4 + c, zero weights on px >= 11 and c == 3."""
    rng = np.random.default_rng(3)
    w = (rng.standard_normal((64, 3, 11, 11)) * 0.1).astype(np.float32)
    bias = rng.standard_normal(64).astype(np.float32)
    d = _lib.ConvDesc()
    d.cin, d.cout, d.ksize, d.stride, d.pad = 3, 64, 11, 4, 2
    d.k_packed = K = 704
    d.cout_pad = 128
    hi = np.zeros((128, K), dtype=np.uint16)
    lo = np.zeros_like(hi)
    sc = np.zeros(128, dtype=np.float32)
    sh = np.zeros(128, dtype=np.float32)
    assert mpx_lib.mpx_pack_conv_weights(C.byref(d), _p(w), None, None, _p(bias), None, None, 1e-5, _p(hi), _p(lo), _p(sc), _p(sh)) == 0
    planes = _unpacked(hi, lo, 128, K)
    got = planes[:64] * sc[:64, None].astype(np.float64)        # the exponent undone
    want = np.zeros((64, 11, 16, 4))
    want[:, :, :11, :3] = w.transpose(0, 2, 3, 1)               # [cout][ky][px][c]
    # a split-fp16 pair carries 22 bits of a weight scaled into [512, 1024): 2^-22 relative to the row's max |w| < 1
    np.testing.assert_allclose(got, want.reshape(64, K), rtol=0, atol=2.0 ** -21)
    g = got.reshape(64, 11, 16, 4)
    assert (g[:, :, 11:, :] == 0).all() and (g[..., 3] == 0).all()
    assert (planes[64:] == 0).all() and (sh[:64] == bias).all() and (sh[64:] == 0).all()
    # element ky*64 + px*4 + c, spelled out
    for co, c, ky, px in ((0, 0, 0, 0), (5, 2, 10, 10), (63, 1, 7, 8), (17, 0, 3, 7)):
        assert abs(got[co, ky * 64 + px * 4 + c] - float(w[co, c, ky, px])) <= 2.0 ** -21


def test_pack_refuses_other_k_for_the_11x11_three_channel_layer(mpx_lib):
    rng = np.random.default_rng(4)
    w = rng.standard_normal((16, 3, 11, 11)).astype(np.float32)
    b = np.zeros(16, dtype=np.float32)
    for K in (352, 11 * 11 * 4, 768):
        d = _lib.ConvDesc()
        d.cin, d.cout, d.ksize, d.k_packed, d.cout_pad = 3, 16, 11, K, 128
        hi = np.zeros((128, K), dtype=np.uint16)
        lo = np.zeros_like(hi)
        sc = np.zeros(128, dtype=np.float32)
        assert mpx_lib.mpx_pack_conv_weights(C.byref(d), _p(w), None, None, _p(b), None, None, 1e-5, _p(hi), _p(lo), _p(sc), _p(sc.copy())) == -1


# sha256 of w_hi | w_lo | scale | shift of the descriptors the existing packer tests use (tests/test_vgg_cpu.py: the ResNet stem, the CIFAR
# conv1, a 5-wide row-run layer, the VGG first layer), weights from default_rng(5), recorded on the commit before the 704 rule
EXISTING_PACKS = {
    (7, 224): "30cd0611a06b1a5259ba59682255b1f5dfdb06a1aea90319d645fc23e41aa888",
    (3, 288): "27628e966703971ba1d85f90585eeaca3c6004182180aa6f0669d2393038b908",
    (5, 160): "caf738ba0c63b93d46e73e0477a296881d75fa11f0eb214bcc099a0a118510e6",
    (3, 96): "16055684404cbf58dd69219547259ca752ea2d47769e3115ac1a2024ecbbc6d3",
}


def test_existing_three_channel_descriptors_pack_to_the_same_bytes(mpx_lib):
    for (k, K), want in EXISTING_PACKS.items():
        rng = np.random.default_rng(5)
        d = _lib.ConvDesc()
        d.cin, d.cout, d.ksize, d.k_packed, d.cout_pad = 3, 16, k, K, 128
        w = rng.standard_normal((16, 3, k, k)).astype(np.float32)
        b = rng.standard_normal(16).astype(np.float32)
        hi = np.zeros((128, K), dtype=np.uint16)
        lo = np.zeros_like(hi)
        sc = np.zeros(128, dtype=np.float32)
        sh = np.zeros(128, dtype=np.float32)
        assert mpx_lib.mpx_pack_conv_weights(C.byref(d), _p(w), None, None, _p(b), None, None, 1e-5, _p(hi), _p(lo), _p(sc), _p(sh)) == 0
        got = hashlib.sha256(hi.tobytes() + lo.tobytes() + sc.tobytes() + sh.tobytes()).hexdigest()
        assert got == want, (k, K, got)
    # ... and a 7x7 three-channel descriptor with any other K is still refused
    d = _lib.ConvDesc()
    d.cin, d.cout, d.ksize, d.k_packed, d.cout_pad = 3, 16, 7, 7 * 7 * 32, 128
    w = np.zeros((16, 3, 7, 7), dtype=np.float32)
    hi = np.zeros((128, d.k_packed), dtype=np.uint16)
    sc = np.zeros(128, dtype=np.float32)
    assert mpx_lib.mpx_pack_conv_weights(C.byref(d), _p(w), None, None, _p(sc.copy()), None, None, 1e-5, _p(hi), _p(hi.copy()), _p(sc), _p(sc.copy())) == -1


def test_classifier1_as_a_6x6_conv_is_linear_on_flatten():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 256, 6, 6, generator=g, dtype=torch.float64)
    w = torch.randn(64, 9216, generator=g, dtype=torch.float64)
    b = torch.randn(64, generator=g, dtype=torch.float64)
    lin = F.linear(torch.flatten(x, 1), w, b)
    conv = F.conv2d(x, w.view(64, 256, 6, 6), b).flatten(1)
    assert ((lin - conv).abs() <= 1e-12 * lin.abs().clamp(min=1.0)).all()


def test_c_abi_exports_maxpool3x3s2p0(mpx_lib):
    assert "mpx_maxpool3x3s2p0" in _lib.SIGNATURES
    assert mpx_lib.mpx_maxpool3x3s2p0(None, None, None, None, None, 1, 55, 64, None) == -1


@pytest.mark.parametrize("arch_id", [4001, 4099])
def test_unknown_alexnet_id_is_refused(mpx_lib, arch_id):
    """mpx_create rejects the id before it touches a device."""
    h = C.c_void_p()
    assert mpx_lib.mpx_create(arch_id, 4, 0, C.byref(h)) == -1 and not h.value


def _sequential(sd):
    """An nn.Sequential build of torchvision's AlexNet written independently of alexnet_ref (module by module, load_state_dict)."""
    model = nn.Module()
    model.features = nn.Sequential(
        nn.Conv2d(3, 64, kernel_size=11, stride=4, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
        nn.Conv2d(64, 192, kernel_size=5, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
        nn.Conv2d(192, 384, kernel_size=3, padding=1), nn.ReLU(inplace=True),
        nn.Conv2d(384, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True),
        nn.Conv2d(256, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2))
    model.avgpool = nn.AdaptiveAvgPool2d((6, 6))
    model.classifier = nn.Sequential(nn.Dropout(), nn.Linear(256 * 6 * 6, 4096), nn.ReLU(inplace=True), nn.Dropout(),
                                     nn.Linear(4096, 4096), nn.ReLU(inplace=True), nn.Linear(4096, 1000))
    model.load_state_dict(sd, strict=True)
    model.double().eval()

    def run(x):
        return model.classifier(torch.flatten(model.avgpool(model.features(x)), 1))
    return run


def test_fp64_restatement_matches_an_nn_sequential_build():
    sd = synth.make_state_dict("alexnet")
    x = scorer.to_tensor_normalize(synth.make_images(2)[1])[None].double()
    with torch.no_grad():
        want = _sequential(sd)(x)
        got = alexnet_ref.forward(alexnet_ref.cast(sd, torch.float64), x)
    assert tuple(got.shape) == (1, 1000)
    assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())


def test_restatement_trace_has_the_maps_the_engine_runs():
    sd = alexnet_ref.cast(synth.make_state_dict("alexnet"), torch.float64)
    trace = []
    with torch.no_grad():
        alexnet_ref.forward(sd, torch.zeros(1, 3, 224, 224, dtype=torch.float64), trace)
    assert [tuple(t.shape[1:]) for t in trace] == [(64, 55, 55), (192, 27, 27), (384, 13, 13), (256, 13, 13), (256, 13, 13), (4096,), (4096,)]


def test_synthetic_alexnet_keeps_activations_o1_and_the_softmax_peaked_but_unsaturated():
    """Without this a 1e-4 score check says nothing (synth docstring); fp16 hi saturates at 65504."""
    sd = alexnet_ref.cast(synth.make_state_dict("alexnet"), torch.float64)
    x = scorer.to_tensor_normalize(synth.make_images(1)[0])[None].double()
    trace = []
    with torch.no_grad():
        logits = alexnet_ref.forward(sd, x, trace)
    rms = [t.pow(2).mean().sqrt().item() for t in trace]
    assert min(rms) > 0.3 and max(rms) < 3.0, rms
    assert max(t.abs().max().item() for t in trace) < 65504 / 1000
    p = F.softmax(logits, 1)[0]
    assert 0.05 < p.max().item() < 0.99
    assert int((p > 1e-3).sum()) >= 3
