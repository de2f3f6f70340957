"""ViT-B/16 / ViT-B/32 without a GPU: the synthetic state_dict with torchvision's keys in torchvision's order, the parameter and MAC counts
computed two ways, the fp64 / fp32 CPU restatement (tests/vit_ref.py) against an independent nn.Module build, the conditions on exactly the
rows the GPU test scores (attention, the position embedding and the class token really move their scores), the ids, the descriptor-name
mapping, the bias-only packing, the C-ABI surface and the static no-scratch guard on the new kernels.

Surveyed on the CPU in fp64 with the committed gains (synth.VIT_*; felzenszwalb / grid picture).  vit_b_16: token RMS 0.93 / 1.05, trunk RMS
1.18 .. 3.25 / 1.28 .. 3.34 over the 12 layers (additive growth: 24 updates of about 0.6), attention logits' standard deviation per row 2.14
falling to 1.29 in the last layer, mean softmax peak per row 0.18 falling to 0.07 (uniform: 0.005), GELU pre-activations' 1 % / 99 %
quantiles -3.5 / +3.5, unmasked softmax peak 0.14 / 0.22, the rows' peaks 0.15 .. 0.25 / 0.16 .. 0.27, fp64 top-two margins >= 0.22 / 0.83;
the rows move by >= 0.0096 with uniform attention weights, >= 0.009 without the position embedding, >= 0.0101 with a zero class token.
vit_b_32 (heads.head gain 2.5; at 3.0 the unmasked grid picture peaks at 0.952): logits' standard deviation 2.2 falling to 1.4, mean peak 0.34
falling to 0.16 (uniform: 0.02), unmasked peak 0.34 / 0.88, rows' peaks 0.12 .. 0.23 / 0.58 .. 0.71, margins >= 0.29 / 1.8, smallest moves 0.013 /
0.026.  With seeds 11 / 5 for the rows (ConvNeXt's) one vit_b_16 row moved by 0.0010 without the position embedding and one by 0.0017 with a
zero class token: the rows are seeds 8 / 1 (tests/vit_ref.E2E_CASES)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import netref
import vit_ref as ref
from network_interpretation_imagenet_amd import _lib, engine, synth
from oracle import scorer
from test_host_logic import _device_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {"vit_b_16": 86567656, "vit_b_32": 88224232}            # torchvision's published parameter counts
NEW_SYMBOLS = ("mpx_conv_rows", "mpx_num_attn", "mpx_attn_info", "mpx_load_tokens", "mpx_token_params", "mpx_attention", "mpx_tokens_assemble",
               "mpx_layernorm_rows", "mpx_profile_collect_attn")
MOVE = 2e-3         # every scored row moves by more than this when the attention weights, the position embedding or the class token are taken away


def _expected_keys(arch):
    """models.vit_b_16() / vit_b_32().state_dict(): key -> shape, in module order, written out from the table."""
    p, t = ref.PATCH[arch], ref.TOKENS[arch]
    wb = lambda q, w, b: [(q + ".weight", w), (q + ".bias", b)]
    out = [("class_token", (1, 1, 768))] + wb("conv_proj", (768, 3, p, p), (768,)) + [("encoder.pos_embedding", (1, t, 768))]
    for i in range(12):
        q = "encoder.layers.encoder_layer_%d." % i
        out += wb(q + "ln_1", (768,), (768,))
        out += [(q + "self_attention.in_proj_weight", (2304, 768)), (q + "self_attention.in_proj_bias", (2304,))]
        out += wb(q + "self_attention.out_proj", (768, 768), (768,)) + wb(q + "ln_2", (768,), (768,))
        out += wb(q + "mlp.0", (3072, 768), (3072,)) + wb(q + "mlp.3", (768, 3072), (768,))
    return out + wb("encoder.ln", (768,), (768,)) + wb("heads.head", (1000, 768), (1000,))


@pytest.mark.parametrize("arch", ref.ARCHS)
def test_synth_vit_state_dict_has_torchvisions_keys_order_and_shapes(arch):
    sd = synth.make_state_dict(arch)
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == _expected_keys(arch)
    assert list(sd) == list(synth.make_vit_state_dict(arch)) and all(v.dtype == torch.float32 for v in sd.values())
    assert sum(v.numel() for v in sd.values()) == PARAMS[arch] == ref.PARAMS[arch]         # every entry is an nn.Parameter
    # neither torchvision's zero head nor its 0.02 position embedding, which would switch both off
    assert sd["heads.head.weight"].std().item() > 0.05 and 0.4 < sd["encoder.pos_embedding"].std().item() < 0.6


@pytest.mark.parametrize("arch,macs", [("vit_b_16", 17563828224), ("vit_b_32", 4409186304)])
def test_macs_and_launch_counts_are_the_known_answers(arch, macs):
    """Counted here in closed form, then compared with the restatement's topology (which the GPU test compares with the engine's lists and
    mpx_flops_per_forward = 2 x this).  The attention products count: 2 * T^2 * 64 * 12 per layer."""
    p, t = ref.PATCH[arch], ref.TOKENS[arch]
    linear = 768 * 2304 + 768 * 768 + 2 * 768 * 3072
    want = (t - 1) * 768 * 3 * p * p + 12 * (t * linear + 2 * t * t * 64 * 12) + 768 * 1000
    assert want == macs == ref.MACS[arch] == ref.macs(arch)
    convs, lnorms, attns = ref.topology(arch)
    assert (len(convs), len(lnorms), len(attns)) == (50, 25, 12) and convs[0][0] == "conv_proj" and convs[-1][0] == "heads.head"
    assert sum(c[7] for c in convs) == 12 and sum(c[6] for c in convs) == 24              # one GELU layer and two residual layers per block
    assert sum(c[5] for c in convs) == 48 and all(c[4] == t for c in convs if c[5])       # the token layers run on T rows per image
    assert len(convs) + len(lnorms) + len(attns) + 1 + 1 == 89                             # + the token assembly and the head: the launches of a forward
    assert max(len(c[0]) for c in convs) == len("encoder_layer_11.self_attention.out_proj") == 40 < 48


def test_vit_arch_ids_and_the_unserved_names():
    assert engine.ARCH_IDS["vit_b_16"] == 13016 and engine.ARCH_IDS["vit_b_32"] == 13032
    ids = list(engine.ARCH_IDS.values())
    assert len(ids) == len(set(ids))
    for name in ("vit_l_16", "vit_l_32", "vit_h_14", "swin_t", "swin_b"):
        assert name not in engine.ARCH_IDS
        with pytest.raises(ValueError, match="ViT-B/16"):
            engine.MaskedForwardEngine(name)
    assert engine.default_bn_eps("vit_b_16") == 1e-6 and engine.default_bn_eps("resnet50") == 1e-5


def test_descriptor_names_map_back_to_torchvisions():
    """name[48] cannot hold torchvision's longest prefix, so descriptor names drop "encoder.layers."; the loader puts it back, and every key it
    then asks for exists in the state_dict -- in_proj's with an underscore."""
    assert len("encoder.layers.encoder_layer_11.self_attention.out_proj") > 47
    sd = synth.make_state_dict("vit_b_16")
    convs, lnorms, _attns = ref.topology("vit_b_16")
    for c in convs:
        full = engine.state_dict_name(c[0])
        keys = (full + "_weight", full + "_bias") if c[0].endswith(".in_proj") else (full + ".weight", full + ".bias")
        assert all(k in sd for k in keys), keys
        assert len(c[0]) < 48
    for n in lnorms:
        assert engine.state_dict_name(n) + ".weight" in sd and len(n) < 64
    assert engine.state_dict_name("encoder_layer_11.mlp.3") == "encoder.layers.encoder_layer_11.mlp.3"
    assert engine.state_dict_name("conv_proj") == "conv_proj" and engine.state_dict_name("heads.head") == "heads.head" and engine.state_dict_name("layer1.0.conv1") == "layer1.0.conv1"
    used = {engine.state_dict_name(c[0]) + s for c in convs for s in ((("_weight", "_bias") if c[0].endswith(".in_proj") else (".weight", ".bias")))}
    used |= {engine.state_dict_name(n) + s for n in lnorms for s in (".weight", ".bias")} | {"class_token", "encoder.pos_embedding"}
    assert used == set(sd)                                   # and nothing in the state_dict is left unread


def test_new_c_abi_symbols_are_in_the_header_the_binding_and_the_library(mpx_lib):
    netref.assert_c_abi_symbols(mpx_lib, "MPX_ARCH_VIT 13000", NEW_SYMBOLS)
    # every entry refuses a null engine before it touches a device
    ad, p, a = _lib.AttnDesc(), C.c_void_p(), C.c_int()
    assert mpx_lib.mpx_attention(None, None, None, None, None, 1, 197, 12, 0, None) == -1
    assert mpx_lib.mpx_tokens_assemble(None, None, None, None, None, None, None, 1, 197, 768, 0, None) == -1
    assert mpx_lib.mpx_layernorm_rows(None, None, None, None, None, 1e-6, None, None, 1, 197, 768, 0, None) == -1
    assert mpx_lib.mpx_conv_rows(None, 0, C.byref(a)) == -1 and mpx_lib.mpx_num_attn(None) == -1 and mpx_lib.mpx_attn_info(None, 0, C.byref(ad)) == -1
    assert mpx_lib.mpx_load_tokens(None, None, None) == -1 and mpx_lib.mpx_token_params(None, C.byref(p), C.byref(p), C.byref(a), C.byref(a)) == -1
    assert mpx_lib.mpx_profile_collect_attn(None, None, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert [n for n, _t in _lib.AttnDesc._fields_] == ["name", "tokens", "heads", "head_dim"] and C.sizeof(_lib.AttnDesc) == 48 + 3 * 4
    assert C.sizeof(_lib.ConvDesc) == 96 + 11 * 4              # mpx_conv_desc keeps its layout


@pytest.mark.parametrize("arch_id", [13000, 13014, 13017, 13033, 13999])
def test_unknown_vit_id_is_refused(mpx_lib, arch_id):
    """mpx_create rejects the id before it touches a device."""
    h = C.c_void_p()
    assert mpx_lib.mpx_create(arch_id, 4, 0, C.byref(h)) == -1 and not h.value


def test_eps_zero_packs_a_bias_only_layer_exactly(mpx_lib):
    """A bias-only Linear through the host packer: conv_bias = bias, gamma = 1, beta = 0, mean = 0, var = 1, eps = 0 gives scale = 2^-e and
    shift = bias bit for bit -- and the same planes, scale and shift as the packer's no-BatchNorm form (gamma = NULL, the bias as beta)."""
    d = _lib.ConvDesc()
    d.cin, d.cout, d.ksize, d.stride, d.pad, d.hin, d.hout, d.relu, d.residual, d.k_packed, d.cout_pad = 768, 96, 1, 1, 0, 0, 0, 0, 1, 768, 128
    g = torch.Generator().manual_seed(3)
    w = torch.randn(96, 768, generator=g) * 0.05
    bias = torch.randn(96, generator=g)
    zero, one = torch.zeros(96), torch.ones(96)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    out = []
    for args in ((ptr(bias), ptr(one), ptr(zero), ptr(zero), ptr(one)), (None, None, ptr(bias), None, None)):
        hi, lo = torch.zeros(128 * 768, dtype=torch.int16), torch.zeros(128 * 768, dtype=torch.int16)
        sc, sh = torch.zeros(128), torch.zeros(128)
        assert mpx_lib.mpx_pack_conv_weights(C.byref(d), ptr(w), *args, 0.0, ptr(hi), ptr(lo), ptr(sc), ptr(sh)) == 0
        out.append((hi, lo, sc, sh))
    e = 10 - torch.frexp(w.abs().max(1)[0])[1]
    hi, lo, sc, sh = out[0]
    assert torch.equal(sc[:96], torch.ldexp(torch.ones(96, dtype=torch.float64), -e).float()) and torch.equal(sh[:96], bias)
    assert (sc[96:] == 0).all() and (sh[96:] == 0).all()
    assert all(torch.equal(a, b) for a, b in zip(out[0], out[1]))


def test_pack_conv_weights_keeps_its_meaning_for_the_patch_stems_descriptors(mpx_lib):
    """mpx_pack_conv_weights sees the descriptor alone, and cin = 3, k = 16, K = 1024 is also a generic layout (256 taps of cin_pad = 4): the
    public packer keeps that meaning; only mpx_set_conv_weights, which knows the layer is a stem, asks for the row-run layout."""
    d = _lib.ConvDesc()
    d.cin, d.cout, d.ksize, d.stride, d.pad, d.hin, d.hout, d.relu, d.residual, d.k_packed, d.cout_pad = 3, 16, 16, 16, 0, 224, 14, 0, 0, 1024, 16
    g = torch.Generator().manual_seed(5)
    w = torch.randn(16, 3, 16, 16, generator=g)
    hi, lo = torch.zeros(16 * 1024, dtype=torch.int16), torch.zeros(16 * 1024, dtype=torch.int16)
    sc, sh = torch.zeros(16), torch.zeros(16)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert mpx_lib.mpx_pack_conv_weights(C.byref(d), ptr(w), None, None, None, None, None, 0.0, ptr(hi), ptr(lo), ptr(sc), ptr(sh)) == 0
    # generic layout: k index (ky * 16 + kx) * 4 + c; row 0 sits in the first 16-row piece: element (k >> 5) * 512 + chunk * 8 + (k & 7)
    e = 10 - int(torch.frexp(w[0].abs().max())[1])
    k = (5 * 16 + 7) * 4 + 2
    at = (k >> 5) * 512 + (((k >> 3) & 3) ^ 0) * 8 + (k & 7)
    want = torch.ldexp(w[0, 2, 5, 7].double(), torch.tensor(e)).to(torch.float16)
    assert hi.view(torch.float16)[at] == want


def test_the_new_kernels_have_no_scratch(mpx_lib):
    """Read from the built library, no GPU: the attention and token assembly kernels and the LayerNorm kernel (mpx_cnext.h's
    layernorm_c_kernel, which takes the input row stride of encoder.ln: there is no strided copy of it) use no scratch and spill nothing,
    and every conv kernel the parent had is still there under its own name."""
    ks = _device_kernels(_lib.LIB_PATH)
    new = {n: k for n, k in ks.items() if any(t in n for t in ("attention_f16x3_kernel", "tokens_assemble_kernel", "layernorm_c_kernel"))}
    assert len(new) == 3, sorted(ks)
    assert not any("layernorm_rows_kernel" in n for n in ks)
    for n, k in new.items():
        assert int(k["private_segment_fixed_size"]) == 0 and int(k.get("vgpr_spill_count", 0)) == 0, (n, k)
    assert len([n for n in ks if "conv_f16x3_kernel" in n and "ConvGelu" not in n]) == 13 and len([n for n in ks if "ConvGelu" in n]) == 5
    assert sum("layernorm_c_kernel" in n for n in ks) == 1


# ------------------------------------------------------------------------------------------------
# the restatement against an independent nn.Module build
# ------------------------------------------------------------------------------------------------
class _Block(nn.Module):
    def __init__(self):
        super().__init__()
        self.ln_1 = nn.LayerNorm(768, eps=1e-6)
        self.self_attention = nn.MultiheadAttention(768, 12, dropout=0.0, batch_first=True)
        self.ln_2 = nn.LayerNorm(768, eps=1e-6)
        self.mlp = nn.Sequential(nn.Linear(768, 3072), nn.GELU(), nn.Dropout(0.0), nn.Linear(3072, 768), nn.Dropout(0.0))

    def forward(self, x):
        y = self.ln_1(x)
        y, _ = self.self_attention(y, y, y, need_weights=False)
        x = x + y
        return x + self.mlp(self.ln_2(x))


class _Encoder(nn.Module):
    def __init__(self, t):
        super().__init__()
        self.pos_embedding = nn.Parameter(torch.zeros(1, t, 768))
        self.layers = nn.Sequential()
        for i in range(12):
            self.layers.add_module("encoder_layer_%d" % i, _Block())
        self.ln = nn.LayerNorm(768, eps=1e-6)

    def forward(self, x):
        return self.ln(self.layers(x + self.pos_embedding))


class _ViT(nn.Module):
    """torchvision's module tree (same names, so load_state_dict(strict=True) is the check of the key set), built with nn modules."""

    def __init__(self, patch):
        super().__init__()
        self.class_token = nn.Parameter(torch.zeros(1, 1, 768))
        self.conv_proj = nn.Conv2d(3, 768, patch, patch)
        self.encoder = _Encoder((224 // patch) ** 2 + 1)
        self.heads = nn.Sequential()
        self.heads.add_module("head", nn.Linear(768, 1000))

    def forward(self, x):
        x = self.conv_proj(x).flatten(2).permute(0, 2, 1)
        x = torch.cat([self.class_token.expand(x.shape[0], -1, -1), x], 1)
        return self.heads(self.encoder(x)[:, 0])


@pytest.mark.parametrize("arch,dtype", [("vit_b_32", torch.float64), ("vit_b_32", torch.float32), ("vit_b_16", torch.float64)])
def test_restatement_matches_an_nn_module_build(arch, dtype):
    sd = synth.make_state_dict(arch)
    model = _ViT(ref.PATCH[arch])
    model.load_state_dict(sd, strict=True)
    model.to(dtype).eval()
    x = scorer.to_tensor_normalize(synth.make_images(2)[1])[None].to(dtype)
    trace = []
    with torch.no_grad():
        want = model(x)
        got = ref.forward(ref.cast(sd, dtype), x, trace)
    assert tuple(got.shape) == (1, 1000) and len(trace) == 1 + 4 * 12
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    print("%s %s: max |d| %.3e of logit scale %.2f" % (arch, dtype, err, scale))
    assert scale > 1.0 and err <= 1e-5 * scale


@pytest.mark.parametrize("arch", ref.ARCHS)
def test_synthetic_vit_statistics_and_switches_on_the_rows_the_gpu_test_scores(golden_dir, arch):
    """The residual stream neither dies nor explodes, the attention logits spread so that rows lie between uniform and a few dominant keys,
    the GELU pre-activations spread over about +-3.5, the fp64 softmax is peaked but unsaturated on the unmasked picture and on EVERY scored
    row, every row's fp64 top-two margin is >= 1e-3, and every row moves by more than 2e-3 under each of the three switches."""
    t = ref.TOKENS[arch]
    for kind, m, _seed in ref.E2E_CASES:
        r = ref.e2e_rows(golden_dir, arch)[kind]
        trace = dict(r["trace"])
        trunk = [trace[ref.PREFIX + "encoder_layer_%d" % i].pow(2).mean().sqrt().item() for i in range(12)]
        assert 0.5 < trace["tokens"].pow(2).mean().sqrt().item() < 2.0 and min(trunk) > 0.8 and max(trunk) < 5.0, trunk
        spread, peak = [], []
        for i in range(12):
            q, k = (z.reshape(1, t, 12, 64).permute(0, 2, 1, 3) for z in trace[ref.PREFIX + "encoder_layer_%d.qkv" % i].split(768, -1)[:2])
            s = q @ k.transpose(-1, -2) / 8
            spread.append(s.std(-1).mean().item())
            peak.append(F.softmax(s, -1).max(-1)[0].mean().item())
        assert 1.0 < min(spread) and max(spread) < 3.0 and 3.0 / t < min(peak) and max(peak) < 0.5, (spread, peak)
        pre = torch.cat([v.flatten()[::97] for name, v in r["trace"] if name.endswith(".pre")])
        q01, q99 = pre.quantile(0.01).item(), pre.quantile(0.99).item()
        assert -5.0 < q01 < -2.5 and 2.5 < q99 < 5.0
        top2 = np.sort(r["logits64"], axis=1)[:, -2:]
        gap = top2[:, 1] - top2[:, 0]
        peaks = F.softmax(torch.from_numpy(r["logits64"]), 1).max(1)[0].numpy()
        print("%s %s: trunk rms %.2f .. %.2f, logit spread %.2f .. %.2f, mean row peak %.3f .. %.3f, pre-activation quantiles %.2f / %.2f, top softmax %.4f, "
              "%d rows, scores %.4f .. %.4f, peaks %.3f .. %.3f, smallest fp64 top-two margin %.4f"
              % (arch, kind, min(trunk), max(trunk), min(spread), max(spread), min(peak), max(peak), q01, q99, r["p"].max().item(), m, r["s64"].min(),
                 r["s64"].max(), peaks.min(), peaks.max(), gap.min()))
        assert 0.05 <= r["p"].max().item() <= 0.95
        assert len(peaks) == m and peaks.min() >= 0.05 and peaks.max() <= 0.95       # every row the GPU test scores, none excluded
        assert gap.min() >= 1e-3
        for name, s in r["moved"].items():
            d = np.abs(s - r["s64"])
            print("%s %s %s: rows move by %.4f .. %.4f" % (arch, kind, name, d.min(), d.max()))
            assert d.min() > MOVE, (arch, kind, name, d)
