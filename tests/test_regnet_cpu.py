"""RegNetX-400MF .. -8GF without a GPU: the table of the five networks held twice over (from torchvision's BlockParams rule and from the
restatement's topology: widths, depths, groups, parameters, MACs), the synthetic state_dict with torchvision's keys, order and shapes, the
arch ids, the ids that stay refused, the header / binding / library, and the conditions on exactly the rows the GPU test scores
(tests/regnet_ref.py E2E_CASES): the fp64 top-two margin, the softmax peak, and that grouping is live on every one of them.

Surveyed with the gains of synth.REGNET_ARCHS (fp64, rows of E2E_CASES; smallest top-two margin, softmax peak, smallest move of a score when
group g reads the channels of group g + 1):
  regnet_x_400mf (f.c gain 0.4)  felz 8 rows: margin 0.0045, peak 0.122 .. 0.733, move 0.094;  grid 4 rows: margin 1.87, peak 0.725 .. 0.796, move 0.724
  regnet_x_800mf (0.3)           felz 4 rows: margin 0.687,  peak 0.057 .. 0.509, move 0.021;  grid 2 rows: margin 1.35, peak 0.567 .. 0.613, move 0.233
  regnet_x_1_6gf (0.4)           felz 4 rows: margin 0.143,  peak 0.204 .. 0.450, move 0.197;  grid 2 rows: margin 0.97, peak 0.652 .. 0.732, move 0.651
  regnet_x_3_2gf (0.3)           felz 4 rows: margin 0.768,  peak 0.126 .. 0.621, move 0.068;  grid 2 rows: margin 1.46, peak 0.732 .. 0.784, move 0.700
  regnet_x_8gf   (0.4)           felz 3 rows: margin 1.31,   peak 0.415 .. 0.720, move 0.414
With a gain of 0.3 on all five, 400MF's and 1.6GF's felz peaks fall to 0.037 / 0.029 and an 8GF row moves by 4e-4 only; with 0.5 the 8GF peak saturates (0.986 .. 1).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import netref
import regnet_ref as ref
from network_interpretation_imagenet_amd import _lib, engine, synth
from oracle import scorer

ARCHS = ref.ARCHS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _expected_keys(arch):
    """models.<arch>().state_dict() without num_batches_tracked: key -> shape, written out from the table."""
    _id, widths, depths, gw, groups, _p, _m, _n = ref.TABLE[arch]
    out = [("stem.0.weight", (32, 3, 3, 3))] + netref.bn_keys("stem.1", 32, tracked=False)
    cin = 32
    for s in range(4):
        w = widths[s]
        for j in range(depths[s]):
            p = "trunk_output.block%d.block%d-%d." % (s + 1, s + 1, j)
            if j == 0:
                out += [(p + "proj.0.weight", (w, cin, 1, 1))] + netref.bn_keys(p + "proj.1", w, tracked=False)
            out += [(p + "f.a.0.weight", (w, cin, 1, 1))] + netref.bn_keys(p + "f.a.1", w, tracked=False)
            out += [(p + "f.b.0.weight", (w, w // groups[s], 3, 3))] + netref.bn_keys(p + "f.b.1", w, tracked=False)
            out += [(p + "f.c.0.weight", (w, w, 1, 1))] + netref.bn_keys(p + "f.c.1", w, tracked=False)
            cin = w
    return out + [("fc.weight", (1000, cin)), ("fc.bias", (1000,))]


@pytest.mark.parametrize("arch", ARCHS)
def test_the_table_follows_from_torchvisions_rule_and_from_the_topology(arch):
    """Widths, depths and groups from BlockParams.from_init_params; parameters and MACs from the conv list, from the synthetic state_dict and
    from the tensors the restatement's conv calls see on a real forward."""
    arch_id, widths, depths, gw, groups, n_params, n_macs, n_convs = ref.TABLE[arch]
    r_widths, r_depths, r_gws = ref.block_params(arch)
    assert (r_widths, r_depths) == (widths, depths)
    assert r_gws == tuple(min(gw, w) for w in widths) and tuple(w // g for w, g in zip(widths, r_gws)) == groups
    assert all(w % 8 == 0 for w in widths) and sum(depths) == ref.INIT[arch][0]
    convs = ref.topology(arch)
    assert len(convs) == n_convs == 1 + 3 * sum(depths) + 4 + 1 and convs[-1][0] == "fc" and len({c[0] for c in convs}) == len(convs)
    assert all(len(c[0]) < 48 and len(c[1]) < 48 for c in convs)
    fb = [c for c in convs if c[0].endswith(".f.b.0")]
    assert [c[11] for c in fb] == [g for g, d in zip(groups, depths) for _ in range(d)]
    assert [c[5] for c in fb] == [2 if j == 0 else 1 for d in depths for j in range(d)]
    assert ref.params(arch) == n_params and ref.macs(arch) == n_macs
    sd = synth.make_state_dict(arch)
    assert sum(v.numel() for k, v in sd.items() if k.endswith((".weight", ".bias"))) == n_params
    count = [0]
    with torch.no_grad():
        ref.forward(sd, torch.zeros(1, 3, 224, 224), arch, count=count)
    by_hand = 112 * 112 * 32 * 27 + widths[3] * 1000
    cin, h = 32, 112
    for s in range(4):
        w = widths[s]
        for j in range(depths[s]):
            ho = h // 2 if j == 0 else h
            by_hand += h * h * cin * w + ho * ho * w * (w // groups[s]) * 9 + ho * ho * w * w + (ho * ho * cin * w if j == 0 else 0)
            cin, h = w, ho
    print("%s: %d MACs per forward, %d parameters, %d convs" % (arch, count[0], n_params, len(convs)))
    assert count[0] == by_hand == n_macs
    assert engine.ARCH_IDS[arch] == arch_id == 14000 + {"400mf": 4, "800mf": 8, "1_6gf": 16, "3_2gf": 32, "8gf": 80}[arch[len("regnet_x_"):]]


def test_the_group_counts_and_pitches_are_the_ones_the_kernel_was_written_for():
    groups = {g for a in ARCHS for g in ref.TABLE[a][4]}
    assert {7, 17, 25, 38, 42, 21, 9} <= groups and min(groups) == 1 and max(groups) == 42
    assert ref.TABLE["regnet_x_8gf"][4][0] == 1 and ref.block_params("regnet_x_8gf")[2][0] == 80        # one group of 80 channels: a dense 3x3
    odd = sorted({w for a in ARCHS for w in ref.TABLE[a][1] if w % 32})
    assert odd == [72, 80, 168, 240, 400, 408, 432, 720, 912, 1008]          # (160 = 5 * 32 keeps its width)
    assert [ref.pitch(w) for w in (72, 400, 720, 1008, 64)] == [96, 416, 736, 1024, 64]
    assert {c[2] // c[11] for a in ARCHS for c in ref.topology(a) if c[11] > 1} == {16, 24, 48, 120}


@pytest.mark.parametrize("arch", ARCHS)
def test_synth_regnet_state_dict_has_torchvisions_keys_order_shapes_and_parameter_count(arch):
    sd = synth.make_state_dict(arch)
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == _expected_keys(arch)
    assert list(sd) == list(synth.make_regnet_state_dict(arch))
    assert all(v.dtype == torch.float32 for v in sd.values())
    assert not any(k.endswith(".bias") and sd[k[:-4] + "weight"].dim() == 4 for k in sd)    # no conv has a bias
    assert synth.REGNET_ARCHS[arch][:3] == ref.TABLE[arch][1:4]
    w = sd["trunk_output.block3.block3-1.f.b.0.weight"]                                     # the conv gain comes from the fan-in: 9 cg
    assert abs(w.std().item() / (2.0 / (9 * w.shape[1])) ** 0.5 - 1) < 0.05


def test_regnet_arch_ids_are_unique_and_the_error_text_keeps_its_words():
    ids = list(engine.ARCH_IDS.values())
    assert len(ids) == len(set(ids))
    assert sorted(v for v in ids if 14000 <= v < 15000) == [14004, 14008, 14016, 14032, 14080]
    with pytest.raises(ValueError, match="AlexNet") as e:
        engine.MaskedForwardEngine("no_such_network")
    assert "RegNetX" in str(e.value)
    assert all(engine.default_bn_eps(a) == 1e-5 for a in ARCHS)


@pytest.mark.parametrize("arch_id", [14000, 14001, 14005, 14040, 14160, 14320, 14999])
def test_unknown_regnet_id_is_refused(mpx_lib, arch_id):
    """mpx_create rejects the id before it touches a device."""
    h = C.c_void_p()
    assert mpx_lib.mpx_create(arch_id, 4, 0, C.byref(h)) == -1 and not h.value


def test_the_id_the_tile_and_the_kernel_are_in_the_header_the_binding_and_the_library(mpx_lib):
    with open(os.path.join(ROOT, "include", "mpx.h")) as fh:
        header = fh.read()
    assert "#define MPX_ARCH_REGNET 14000" in header
    assert re.search(r"^ \*  18 = the grouped 3x3 kernel for any group count", header, re.M)
    for name in ARCHS:
        assert name[len("regnet_x"):] in header
    assert "mpx_conv_groups" in _lib.SIGNATURES and getattr(mpx_lib, "mpx_conv_groups") is not None
    with open(os.path.join(ROOT, "network_interpretation_imagenet_amd", "libmpx.so"), "rb") as fh:
        blob = fh.read()
    for cg in (16, 24, 48, 120):        # the four group widths of the kernel (Itanium mangling: the first template argument as Li<cg>E)
        assert ("gconvw3x3_f16x3_kernelILi%dELi" % cg).encode() in blob, cg
    # the descriptor keeps its layout
    assert C.sizeof(_lib.ConvDesc) == 96 + 11 * 4


def test_restatement_is_torch_conv2d_with_groups_and_the_shift_switch_rolls_the_groups():
    """F.conv2d(groups=G) against a dense conv of the zero-extended weight; shift_groups is a roll of the input by one group width."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 72, 9, 9, generator=g, dtype=torch.float64)
    w = torch.randn(72, 24, 3, 3, generator=g, dtype=torch.float64)
    for stride in (1, 2):
        zero_ext = torch.zeros(72, 72, 3, 3, dtype=torch.float64)
        for co in range(72):
            zero_ext[co, co // 24 * 24:co // 24 * 24 + 24] = w[co]
        want = F.conv2d(x, zero_ext, None, stride, 1)
        assert (F.conv2d(x, w, None, stride, 1, 1, 3) - want).abs().max() <= 1e-12 * want.abs().max()
        shifted = torch.zeros_like(zero_ext)
        for co in range(72):
            gi = (co // 24 + 1) % 3
            shifted[co, gi * 24:gi * 24 + 24] = w[co]
        want = F.conv2d(x, shifted, None, stride, 1)
        assert (F.conv2d(x.roll(-24, 1), w, None, stride, 1, 1, 3) - want).abs().max() <= 1e-12 * want.abs().max()


@pytest.mark.parametrize("arch", ARCHS)
def test_preconditions_on_the_rows_the_gpu_test_scores(golden_dir, arch):
    """EVERY row of regnet_ref.E2E_CASES: fp64 top-two logit margin >= 1e-3 and fp64 softmax peak inside [0.05, 0.95] -- the GPU test then
    compares the argmax of every row, none excluded -- and with group g reading the input channels of group (g + 1) mod G EVERY row moves
    by at least 2e-3: a kernel that read the wrong group's channels could not pass."""
    sd = synth.make_state_dict(arch)
    total = 0
    for kind, (img, seg, onoff, label, s64, logits64) in ref.e2e_rows(golden_dir, arch).items():
        top2 = np.sort(logits64, axis=1)[:, -2:]
        gap = top2[:, 1] - top2[:, 0]
        peaks = F.softmax(torch.from_numpy(logits64), 1).max(1)[0].numpy()
        s_shift, _l = ref.score_masks_fp64(sd, arch, scorer.to_tensor_normalize(img), seg, onoff, label, shift_groups=True)
        moved = np.abs(s_shift - s64)
        print("%s %s: %d rows, label %d, scores %.4f .. %.4f, smallest fp64 top-two margin %.4f, softmax peak %.4f .. %.4f; shifted groups: smallest move %.4f (median %.4f)"
              % (arch, kind, len(s64), label, s64.min(), s64.max(), gap.min(), peaks.min(), peaks.max(), moved.min(), np.median(moved)))
        assert gap.min() >= 1e-3
        assert peaks.min() >= 0.05 and peaks.max() <= 0.95
        assert moved.min() >= 2e-3, np.sort(moved)
        assert np.isfinite(logits64).all() and np.abs(logits64).max() < 1e3
        total += len(s64)
    assert total == {"regnet_x_400mf": 12, "regnet_x_800mf": 6, "regnet_x_1_6gf": 6, "regnet_x_3_2gf": 6, "regnet_x_8gf": 3}[arch]
