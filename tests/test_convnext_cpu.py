"""ConvNeXt-Tiny / -Small without a GPU: the synthetic state_dict with torchvision's keys in torchvision's order, the parameter, MAC and
layer counts computed two ways, the fp64 / fp32 CPU restatement (tests/convnext_ref.py) against an independent nn.Module build, the
conditions on exactly the rows the GPU test scores (the blocks, GELU and the per-pixel LayerNorm really move their scores), the C-ABI
surface and the static no-scratch guard on the new kernels.

Surveyed on the CPU in fp64 with the committed gains (synth.CONVNEXT_*; felzenszwalb / grid picture), convnext_tiny: trunk RMS 1.04 .. 1.38
over the 18 blocks, GELU pre-activations std 1.53 with 1 % / 99 % quantiles -3.5 / +3.6 (a quarter below -1, a quarter above +1), unmasked
softmax peak 0.14 / 0.087, rows' peaks 0.53 .. 0.61 / 0.55 .. 0.58, top-two fp64 margins >= 2.56 / 2.70; with the classifier gain at 3.0 its
rows' peaks reach 0.952, so tiny keeps 2.0.  convnext_small at 2.0: rows' peaks 0.18 .. 0.22 / 0.15 .. 0.25, but two rows move by under 2e-3
(0.0019 with ReLU for GELU, 0.0002 with the LayerNorm over the map); at 3.0: unmasked peak 0.54 / 0.73, rows' peaks 0.54 .. 0.62 / 0.43 .. 0.68,
margins >= 1.39 / 1.43, smallest moves 0.0107 / 0.0052: small gets 3.0 (synth.CONVNEXT_FC_GAIN)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import convnext_ref as ref
import netref
from network_interpretation_imagenet_amd import _lib, engine, synth
from oracle import scorer
from test_host_logic import _device_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {"convnext_tiny": 28589128, "convnext_small": 50223688}            # torchvision's published parameter counts
MACS = {"convnext_tiny": 4455531264, "convnext_small": 8683712256}
DEPTHS = {"convnext_tiny": (3, 3, 9, 3), "convnext_small": (3, 3, 27, 3)}
DIMS = (96, 192, 384, 768)
NEW_SYMBOLS = ("mpx_conv_epilogue_act", "mpx_dwconv_ln", "mpx_load_dwconv_ln", "mpx_num_lnorms", "mpx_lnorm_info", "mpx_load_lnorm",
               "mpx_lnorm_params", "mpx_dwconv7x7_ln", "mpx_layernorm_c", "mpx_global_avgpool_ln", "mpx_profile_collect_ln")
MOVE = 2e-3         # every scored row moves by more than this when a block, GELU or the per-pixel reduction is taken away


def _expected_keys(arch):
    """models.convnext_tiny() / convnext_small().state_dict(): key -> shape, in module order, written out from the table."""
    wb = lambda p, w, b: [(p + ".weight", w), (p + ".bias", b)]
    out = wb("features.0.0", (96, 3, 4, 4), (96,)) + wb("features.0.1", (96,), (96,))
    for s, (c, d) in enumerate(zip(DIMS, DEPTHS[arch])):
        if s:
            cp = DIMS[s - 1]
            out += wb("features.%d.0" % (2 * s), (cp,), (cp,)) + wb("features.%d.1" % (2 * s), (c, cp, 2, 2), (c,))
        for b in range(d):
            p = "features.%d.%d." % (2 * s + 1, b)
            out += [(p + "layer_scale", (c, 1, 1))] + wb(p + "block.0", (c, 1, 7, 7), (c,)) + wb(p + "block.2", (c,), (c,))
            out += wb(p + "block.3", (4 * c, c), (4 * c,)) + wb(p + "block.5", (c, 4 * c), (c,))
    return out + wb("classifier.0", (768,), (768,)) + wb("classifier.2", (1000, 768), (1000,))


@pytest.mark.parametrize("arch", ref.ARCHS)
def test_synth_convnext_state_dict_has_torchvisions_keys_order_and_shapes(arch):
    sd = synth.make_state_dict(arch)
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == _expected_keys(arch)
    assert list(sd) == list(synth.make_convnext_state_dict(arch)) and all(v.dtype == torch.float32 for v in sd.values())
    assert sum(v.numel() for v in sd.values()) == PARAMS[arch] == ref.PARAMS[arch]         # every entry is an nn.Parameter: no running statistics
    ls = torch.cat([v.flatten() for k, v in sd.items() if k.endswith("layer_scale")])
    assert 0.1 <= ls.min().item() and ls.max().item() <= 1.0 and 0.45 < ls.mean().item() < 0.65      # O(0.1 .. 1), not torchvision's 1e-6 init


@pytest.mark.parametrize("arch,n_conv,n_dw", [("convnext_tiny", 41, 18), ("convnext_small", 77, 36)])
def test_macs_and_layer_counts_are_the_known_answers(arch, n_conv, n_dw):
    """Counted here stage by stage in closed form, then compared with the restatement's topology (which the GPU test compares with the
    engine's lists and mpx_flops_per_forward = 2 x this)."""
    macs = 56 * 56 * 96 * 3 * 16
    for s, (c, d) in enumerate(zip(DIMS, DEPTHS[arch])):
        h = 56 >> s
        if s:
            macs += h * h * c * DIMS[s - 1] * 4
        macs += d * h * h * (49 * c + 2 * 4 * c * c)
    macs += 768 * 1000
    assert macs == MACS[arch] == ref.MACS[arch] == ref.macs(arch)
    convs, dws, lnorms = ref.topology(arch)
    assert (len(convs), len(dws), len(lnorms)) == (n_conv, n_dw, 5) and convs[-1][0] == "classifier.2" and convs[0][0] == "features.0.0"
    assert sum(c[9] for c in convs) == n_dw == sum(c[8] for c in convs)             # one GELU layer and one residual layer per block
    assert all(c[2] % 32 == 0 or c[2] == 3 for c in convs) and all(c[3] % 32 == 0 or c[3] == 1000 for c in convs)      # no padded pitches
    assert max(c[3] * c[7] * c[7] for c in convs) == 384 * 56 * 56                  # the largest map: block.3's output in stage 0
    assert len({c[0] for c in convs}) == n_conv and [n for n, _c, _h in lnorms] == ["features.0.1", "features.2.0", "features.4.0", "features.6.0", "classifier.0"]


def test_convnext_arch_ids_and_the_unserved_names():
    assert engine.ARCH_IDS["convnext_tiny"] == 12001 and engine.ARCH_IDS["convnext_small"] == 12002
    ids = list(engine.ARCH_IDS.values())
    assert len(ids) == len(set(ids))
    for name in ("convnext_base", "convnext_large"):
        assert name not in engine.ARCH_IDS
        with pytest.raises(ValueError, match="ConvNeXt-Tiny"):
            engine.MaskedForwardEngine(name)
    assert engine.default_bn_eps("convnext_tiny") == 1e-6 and engine.default_bn_eps("resnet50") == 1e-5


def test_new_c_abi_symbols_are_in_the_header_the_binding_and_the_library(mpx_lib):
    netref.assert_c_abi_symbols(mpx_lib, "MPX_ARCH_CONVNEXT 12000", NEW_SYMBOLS)
    # every entry refuses a null engine before it touches a device
    ld, p, a, f = _lib.LnormDesc(), C.c_void_p(), C.c_int(), C.c_float()
    assert mpx_lib.mpx_dwconv7x7_ln(None, None, None, None, None, None, None, 1e-6, None, None, 1, 7, 96, 7, 1, 0, None) == -1
    assert mpx_lib.mpx_layernorm_c(None, None, None, None, None, 1e-6, None, None, 1, 96, 0, None) == -1
    assert mpx_lib.mpx_global_avgpool_ln(None, None, None, None, None, 1e-6, None, None, 1, 49, 768, None) == -1
    assert mpx_lib.mpx_conv_epilogue_act(None, 0, C.byref(a)) == -1 and mpx_lib.mpx_dwconv_ln(None, 0, C.byref(a), C.byref(p), C.byref(f)) == -1
    assert mpx_lib.mpx_load_dwconv_ln(None, 0, None, None, None, None, 1e-6) == -1
    assert mpx_lib.mpx_num_lnorms(None) == -1 and mpx_lib.mpx_lnorm_info(None, 0, C.byref(ld)) == -1
    assert mpx_lib.mpx_load_lnorm(None, 0, None, None, 1e-6) == -1 and mpx_lib.mpx_lnorm_params(None, 0, C.byref(p), C.byref(p), C.byref(f)) == -1
    assert mpx_lib.mpx_profile_collect_ln(None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert [n for n, _t in _lib.LnormDesc._fields_] == ["name", "channels", "hw"] and C.sizeof(_lib.LnormDesc) == 64 + 2 * 4
    # the descriptors that must keep their layout
    assert [n for n, _t in _lib.DwConvDesc._fields_] == ["name", "bn_name", "channels", "pitch", "stride", "hin", "clamp_in"]
    assert C.sizeof(_lib.ConvDesc) == 96 + 11 * 4


@pytest.mark.parametrize("arch_id", [12000, 12003, 12999])
def test_unknown_convnext_id_is_refused(mpx_lib, arch_id):
    """mpx_create rejects the id before it touches a device."""
    h = C.c_void_p()
    assert mpx_lib.mpx_create(arch_id, 4, 0, C.byref(h)) == -1 and not h.value


def test_eps_zero_packs_the_layer_scale_exactly(mpx_lib):
    """block.5 through the host packer: conv_bias = bias, gamma = layer_scale, beta = 0, mean = 0, var = 1, eps = 0 gives scale = layer_scale
    * 2^-e and shift = bias * layer_scale, with no other rounding than the product's."""
    d = _lib.ConvDesc()
    d.cin, d.cout, d.ksize, d.stride, d.pad, d.hin, d.hout, d.relu, d.residual, d.k_packed, d.cout_pad = 384, 96, 1, 1, 0, 56, 56, 0, 1, 384, 128
    g = torch.Generator().manual_seed(3)
    w = torch.randn(96, 384, generator=g) * 0.05
    bias, ls = torch.randn(96, generator=g), 0.1 + 0.9 * torch.rand(96, generator=g)
    zero, one = torch.zeros(96), torch.ones(96)
    hi, lo = torch.zeros(128 * 384, dtype=torch.int16), torch.zeros(128 * 384, dtype=torch.int16)
    sc, sh = torch.zeros(128), torch.zeros(128)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = mpx_lib.mpx_pack_conv_weights(C.byref(d), ptr(w), ptr(bias), ptr(ls), ptr(zero), ptr(zero), ptr(one), 0.0, ptr(hi), ptr(lo), ptr(sc), ptr(sh))
    assert rc == 0
    e = 10 - torch.frexp(w.abs().max(1)[0])[1]
    assert torch.equal(sc[:96], torch.ldexp(ls.double(), -e).float()) and torch.equal(sh[:96], (bias.double() * ls.double()).float())
    assert (sc[96:] == 0).all() and (sh[96:] == 0).all()


def test_the_new_kernels_have_no_scratch(mpx_lib):
    """The static guard of tests/test_host_logic.py matches `_f16x3_kernel` names and allows the generic kernel 72 bytes; the new
    instantiations and the three LayerNorm kernels are held to none at all (read from the built library, no GPU)."""
    ks = _device_kernels(_lib.LIB_PATH)
    gelu = {n: k for n, k in ks.items() if "conv_f16x3_kernel" in n and "ConvGelu" in n}
    ln = {n: k for n, k in ks.items() if any(t in n for t in ("dwconv7x7_ln_kernel", "layernorm_c_kernel", "global_avgpool_ln_kernel"))}
    assert len(gelu) == 5 and len(ln) == 3, sorted(ks)
    for n, k in list(gelu.items()) + list(ln.items()):
        assert int(k["private_segment_fixed_size"]) == 0 and int(k.get("vgpr_spill_count", 0)) == 0, (n, k)
    plain = [n for n in ks if "conv_f16x3_kernel" in n and "ConvGelu" not in n]
    assert len(plain) == 13             # every instantiation the parent had, under its own name


# ------------------------------------------------------------------------------------------------
# the restatement against an independent nn.Module build
# ------------------------------------------------------------------------------------------------
class _LayerNorm2d(nn.LayerNorm):
    def forward(self, x):
        return F.layer_norm(x.permute(0, 2, 3, 1), self.normalized_shape, self.weight, self.bias, self.eps).permute(0, 3, 1, 2)


class _Permute(nn.Module):
    def __init__(self, dims):
        super().__init__()
        self.dims = dims

    def forward(self, x):
        return x.permute(*self.dims)


class _CNBlock(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.block = nn.Sequential(nn.Conv2d(dim, dim, 7, padding=3, groups=dim), _Permute([0, 2, 3, 1]), nn.LayerNorm(dim, eps=1e-6),
                                   nn.Linear(dim, 4 * dim), nn.GELU(), nn.Linear(4 * dim, dim), _Permute([0, 3, 1, 2]))
        self.layer_scale = nn.Parameter(torch.ones(dim, 1, 1) * 1e-6)

    def forward(self, x):
        return x + self.layer_scale * self.block(x)


class _ConvNeXt(nn.Module):
    """torchvision's module tree (same names, so load_state_dict(strict=True) is the check of the key set), built with nn modules."""

    def __init__(self, depths):
        super().__init__()
        layers = [nn.Sequential(nn.Conv2d(3, 96, 4, 4), _LayerNorm2d(96, eps=1e-6))]
        for s, (c, d) in enumerate(zip(DIMS, depths)):
            if s:
                layers.append(nn.Sequential(_LayerNorm2d(DIMS[s - 1], eps=1e-6), nn.Conv2d(DIMS[s - 1], c, 2, 2)))
            layers.append(nn.Sequential(*[_CNBlock(c) for _ in range(d)]))
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(_LayerNorm2d(768, eps=1e-6), nn.Flatten(1), nn.Linear(768, 1000))

    def forward(self, x):
        return self.classifier(self.avgpool(self.features(x)))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_restatement_matches_an_nn_module_build(dtype):
    arch = "convnext_tiny"
    sd = synth.make_state_dict(arch)
    model = _ConvNeXt(DEPTHS[arch])
    model.load_state_dict(sd, strict=True)
    model.to(dtype).eval()
    x = scorer.to_tensor_normalize(synth.make_images(2)[1])[None].to(dtype)
    trace = []
    with torch.no_grad():
        want = model(x)
        got = ref.forward(ref.cast(sd, dtype), x, trace)
    assert tuple(got.shape) == (1, 1000) and len(trace) == 1 + 3 + 3 * 18
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    print("%s %s: max |d| %.3e of logit scale %.2f" % (arch, dtype, err, scale))
    assert scale > 1.0 and err <= 1e-5 * scale


_ROWS = {}


def _rows(golden_dir, arch):
    """The fp64 yardstick of the scored rows, computed once per network: per case (unmasked softmax, trace, scores, logits, and the scores
    under each of the three switches)."""
    if arch not in _ROWS:
        sd = synth.make_state_dict(arch)
        sd64 = ref.cast(sd, torch.float64)
        out = {}
        for kind, m, seed in ref.E2E_CASES:
            img, seg = ref.e2e_inputs(golden_dir, kind)
            x = scorer.to_tensor_normalize(img)
            trace = []
            with torch.no_grad():
                logits = ref.forward(sd64, x[None].double(), trace)
            p = F.softmax(logits, 1)[0]
            label = int(p.argmax())
            onoff = synth.random_onoff(m, len(np.unique(seg)), seed=seed)
            s64, logits64 = ref.score_masks_fp64(sd, x, seg, onoff, label)
            moved = {name: ref.score_masks_fp64(sd, x, seg, onoff, label, **sw)[0]
                     for name, sw in (("layer_scale=1e-6", dict(layer_scale=1e-6)), ("gelu=False", dict(gelu=False)), ("ln_map=True", dict(ln_map=True)))}
            out[kind] = (p, trace, s64, logits64, moved)
        _ROWS[arch] = out
    return _ROWS[arch]


@pytest.mark.parametrize("arch", ref.ARCHS)
def test_synthetic_convnext_statistics_and_switches_on_the_rows_the_gpu_test_scores(golden_dir, arch):
    """The trunk neither grows nor dies, the GELU pre-activations spread over about +-3, the fp64 softmax is peaked but unsaturated on the
    unmasked picture and on EVERY scored row, every row's fp64 top-two margin is >= 1e-3, and every row moves by more than 2e-3 with the
    layer scales at 1e-6 (the blocks matter), with ReLU for GELU (the activation is visible) and with each block LayerNorm's statistics
    taken over the whole map (the per-pixel reduction is visible)."""
    for kind, m, _seed in ref.E2E_CASES:
        p, trace, s64, logits64, moved = _rows(golden_dir, arch)[kind]
        trunk = [t.pow(2).mean().sqrt().item() for name, t in trace if re.fullmatch(r"features\.\d\.\d+", name)]
        pre = torch.cat([t.flatten()[::97] for name, t in trace if name.endswith(".pre")])
        assert len(trunk) == sum(DEPTHS[arch]) and min(trunk) > 0.5 and max(trunk) < 3.0, (min(trunk), max(trunk))
        q01, q99 = pre.quantile(0.01).item(), pre.quantile(0.99).item()
        assert -5.0 < q01 < -2.5 and 2.5 < q99 < 5.0 and (pre < -1).double().mean().item() > 0.1 and (pre > 1).double().mean().item() > 0.1
        top2 = np.sort(logits64, axis=1)[:, -2:]
        gap = top2[:, 1] - top2[:, 0]
        peaks = F.softmax(torch.from_numpy(logits64), 1).max(1)[0].numpy()
        print("%s %s: trunk rms %.3f .. %.3f, pre-activation quantiles %.2f / %.2f, top softmax %.4f, %d rows, scores %.4f .. %.4f, peaks %.3f .. %.3f, "
              "smallest fp64 top-two margin %.4f" % (arch, kind, min(trunk), max(trunk), q01, q99, p.max().item(), m, s64.min(), s64.max(), peaks.min(), peaks.max(), gap.min()))
        assert 0.05 <= p.max().item() <= 0.95
        assert len(peaks) == m and peaks.min() >= 0.05 and peaks.max() <= 0.95       # every row the GPU test scores, none excluded
        assert gap.min() >= 1e-3
        for name, s in moved.items():
            d = np.abs(s - s64)
            print("%s %s %s: rows move by %.4f .. %.4f" % (arch, kind, name, d.min(), d.max()))
            assert d.min() > MOVE, (arch, kind, name, d)
