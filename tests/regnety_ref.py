"""CPU restatement of torchvision's RegNetY forward, regnet_y_800mf .. regnet_y_8gf (test infrastructure only), on top of tests/regnet_ref.py:
the width rule (BlockParams.from_init_params), the stem, the bottleneck and the scoring loops are RegNetX's.  Written from torchvision's
published module structure (regnet.py, ops/misc.py), which is not installed here.

The one addition, in every block between f.b (grouped 3x3 + BN + ReLU) and f.c (1x1 + BN): f.se = SqueezeExcitation(w, q) with
q = int(round(0.25 * w_in)) of the BLOCK's input width (32 in block1-0, the previous stage's width in the other stage openers) --
adaptive_avg_pool2d(1), fc1 (1x1 conv with bias), ReLU, fc2 (1x1 conv with bias), sigmoid, x * gate.  One switch shows that the gates are live
on the rows the tests score: `gate_half=True` replaces every gate by 0.5.
"""
import math

import torch
import torch.nn.functional as F

import netref
import regnet_ref as xref
from regnet_ref import EPS, STEM, bn, cast, e2e_inputs, masked_batch, pitch  # noqa: F401  (re-exported: the tests use them through this module)

# arch -> (depth, w_0, w_a, w_m, group width) of torchvision's regnet_y_* builders
INIT = {
    "regnet_y_800mf": (14, 56, 38.84, 2.4, 16),
    "regnet_y_1_6gf": (27, 48, 20.71, 2.65, 24),
    "regnet_y_3_2gf": (21, 80, 42.63, 2.66, 24),
    "regnet_y_8gf": (17, 192, 76.82, 2.19, 56),
}
ARCHS = tuple(INIT)
# arch -> (engine id, stage widths, depths, group width, groups per stage, parameters, conv entries with the fc, SE layers)
TABLE = {
    "regnet_y_800mf": (15008, (64, 144, 320, 784), (1, 3, 8, 2), 16, (4, 9, 20, 49), 6432512, 48, 14),
    "regnet_y_1_6gf": (15016, (48, 120, 336, 888), (2, 6, 17, 2), 24, (2, 5, 14, 37), 11202430, 87, 27),
    "regnet_y_3_2gf": (15032, (72, 216, 576, 1512), (2, 5, 13, 1), 24, (3, 9, 24, 63), 19436338, 69, 21),
    "regnet_y_8gf": (15080, (224, 448, 896, 2016), (2, 4, 10, 1), 56, (4, 8, 16, 36), 39381472, 57, 17),
}

# The rows the end-to-end checks score: arch -> ((label map, number of mask rows, seed of synth.random_onoff), ...)
E2E_CASES = {
    "regnet_y_800mf": (("felz", 4, 11), ("grid", 2, 5)),
    "regnet_y_1_6gf": (("felz", 4, 11), ("grid", 2, 5)),
    "regnet_y_3_2gf": (("felz", 4, 11), ("grid", 2, 5)),
    "regnet_y_8gf": (("felz", 3, 11),),
}


def block_params(arch):
    """BlockParams.from_init_params with bottleneck multiplier 1 (regnet_ref.block_params on this family's generating parameters):
    -> (stage widths, stage depths, group width per stage)."""
    depth, w_0, w_a, w_m, group_width = INIT[arch]
    quant = 8
    widths_cont = torch.arange(depth) * w_a + w_0
    capacity = torch.round(torch.log(widths_cont / w_0) / math.log(w_m))
    block_widths = (torch.round(torch.divide(w_0 * torch.pow(w_m, capacity), quant)) * quant).int().tolist()
    split = [(w != wp) for w, wp in zip(block_widths + [0], [0] + block_widths)]
    stage_widths = [w for w, t in zip(block_widths, split[:-1]) if t]
    starts = [d for d, t in enumerate(split) if t]
    stage_depths = [b - a for a, b in zip(starts[:-1], starts[1:])]
    gws = [min(group_width, w) for w in stage_widths]
    stage_widths = [xref._make_divisible(w, g) for w, g in zip(stage_widths, gws)]
    return tuple(stage_widths), tuple(stage_depths), tuple(gws)


def blocks(arch):
    """(prefix "trunk_output.blockS.blockS-J.", w_in, w, group width, stride, side of the input map, side of the output map, has proj, q) per
    block, from the rule (block_params), not from the table."""
    widths, depths, gws = block_params(arch)
    out, cin, h = [], STEM, 112
    for s, (w, d, gw) in enumerate(zip(widths, depths, gws)):
        for j in range(d):
            stride = 2 if j == 0 else 1
            ho = (h - 1) // stride + 1
            out.append(("trunk_output.block%d.block%d-%d." % (s + 1, s + 1, j), cin, w, gw, stride, h, ho, j == 0, int(round(0.25 * cin))))
            cin, h = w, ho
    return out


def topology(arch):
    """The conv list in the engine's order: (name, bn name, cin, cout, ksize, stride, pad, hin, hout, relu, residual, groups)."""
    convs = [("stem.0", "stem.1", 3, STEM, 3, 2, 1, 224, 112, 1, 0, 1)]
    cin = STEM
    for p, cin, w, gw, stride, h, ho, proj, _q in blocks(arch):
        if proj:
            convs.append((p + "proj.0", p + "proj.1", cin, w, 1, 2, 0, h, ho, 0, 0, 1))
        convs.append((p + "f.a.0", p + "f.a.1", cin, w, 1, 1, 0, h, h, 1, 0, 1))
        convs.append((p + "f.b.0", p + "f.b.1", w, w, 3, stride, 1, h, ho, 1, 0, w // gw))
        convs.append((p + "f.c.0", p + "f.c.1", w, w, 1, 1, 0, ho, ho, 1, 1, 1))
        cin = w
    convs.append(("fc", "", cin, 1000, 1, 1, 0, 1, 1, 0, 0, 1))
    return convs


def se_layers(arch):
    """The SE list in the engine's order: (name, channels, pitch, q, side of the map it pools)."""
    return [(p + "f.se", w, pitch(w), q, ho) for p, _cin, w, _gw, _stride, _h, ho, _proj, q in blocks(arch)]


def macs(arch):
    """Multiply-accumulates of one forward: the conv list's, plus fc1 and fc2 of every SE layer."""
    return sum(c[8] * c[8] * c[3] * (c[2] // c[11]) * c[4] * c[4] for c in topology(arch)) + sum(2 * w * q for _n, w, _p, q, _h in se_layers(arch))


def params(arch):
    """Parameters: conv weights, two per BatchNorm channel, the fc's bias, and fc1 / fc2 weight and bias of every SE layer."""
    convs = sum(c[3] * (c[2] // c[11]) * c[4] * c[4] + (2 * c[3] if c[1] else c[3]) for c in topology(arch))
    return convs + sum(2 * w * q + q + w for _n, w, _p, q, _h in se_layers(arch))


def se_gate(sd, p, t):
    """The gate [N][w][1][1] of block prefix p for f.b's output t, and fc1's pre-activation [N][q][1][1]."""
    z1 = F.conv2d(F.adaptive_avg_pool2d(t, 1), sd[p + "f.se.fc1.weight"], sd[p + "f.se.fc1.bias"])
    return torch.sigmoid(F.conv2d(F.relu(z1), sd[p + "f.se.fc2.weight"], sd[p + "f.se.fc2.bias"])), z1


def forward(sd, x, arch, trace=None, gate_half=False, gates=None):
    """logits [N, 1000] for the normalised NCHW batch x.  `trace` (a list) receives (name, tensor) of every block output; `gates` (a list)
    every block's gate tensor; gate_half replaces every gate by 0.5."""
    x = F.relu(bn(sd, "stem.1", F.conv2d(x, sd["stem.0.weight"], None, 2, 1)))
    for p, _cin, w, gw, stride, _h, _ho, proj, _q in blocks(arch):
        t = F.relu(bn(sd, p + "f.a.1", F.conv2d(x, sd[p + "f.a.0.weight"])))
        t = F.relu(bn(sd, p + "f.b.1", F.conv2d(t, sd[p + "f.b.0.weight"], None, stride, 1, 1, w // gw)))
        gate, _z1 = se_gate(sd, p, t)
        if gates is not None:
            gates.append(gate)
        t = t * (torch.full_like(gate, 0.5) if gate_half else gate)
        t = bn(sd, p + "f.c.1", F.conv2d(t, sd[p + "f.c.0.weight"]))
        idn = bn(sd, p + "proj.1", F.conv2d(x, sd[p + "proj.0.weight"], None, 2)) if proj else x
        x = F.relu(t + idn)
        if trace is not None:
            trace.append((p[:-1], x))
    x = torch.flatten(F.adaptive_avg_pool2d(x, 1), 1)
    return F.linear(x, sd["fc.weight"], sd["fc.bias"])


def bound(arch):
    """The forward of `arch` as the forward(sd, x, **switches) that netref and the test drivers take."""
    return netref.bound(forward, arch)


def score_masks_reference_loop(sd, arch, x_chw, segments, onoff, label, return_logits=False):
    """netref.score_masks_reference_loop with the RegNetY forward of `arch`."""
    return netref.score_masks_reference_loop(bound(arch), sd, x_chw, segments, onoff, label, return_logits)


def score_masks_fp64(sd, arch, x_chw, segments, onoff, label, gate_half=False):
    """netref.score_masks_fp64 with the RegNetY forward of `arch`, 4 rows at a time."""
    return netref.score_masks_fp64(bound(arch), sd, x_chw, segments, onoff, label, chunk=4, gate_half=gate_half)


_E2E = {}


def e2e_rows(golden_dir, arch):
    """Per case of E2E_CASES[arch], computed once per process and shared: dict kind -> (img, seg, onoff, label, s64, logits64).  The label is
    the fp64 argmax of the unmasked picture."""
    if arch not in _E2E:
        _E2E[arch] = netref.e2e_rows(forward, E2E_CASES[arch], golden_dir, arch, chunk=4)
    return _E2E[arch]
