"""CPU restatement of torchvision's RegNetX forward, regnet_x_400mf .. regnet_x_8gf (test infrastructure only; oracle/ stays ResNet-only).
Written from torchvision's published module structure (regnet.py), which is not installed here.

BlockParams.from_init_params(depth, w_0, w_a, w_m, group_width): the continuous widths w_0 + w_a * i are snapped to w_0 * w_m^k and quantised
to 8; runs of equal widths are the stages; a stage's group width is min(group_width, width) and its width is made divisible by that
(_make_divisible).  The network: stem.0 (3 -> 32, 3x3 stride 2 pad 1) + stem.1 (BatchNorm) + ReLU, no max pool; per stage s = 1 .. 4 blocks
trunk_output.block{s}.block{s}-{j} = ResBottleneckBlock with bottleneck ratio 1 -- f.a 1x1 (w_in -> w) + BN + ReLU, f.b 3x3 pad 1 GROUPED
(w / gw groups, stride 2 in block 0 of every stage) + BN + ReLU, f.c 1x1 (w -> w) + BN, plus proj (1x1 stride 2 + BN) in block 0 or the
identity, ReLU --; adaptive_avg_pool2d(1), fc.  BatchNorm eps 1e-5.  Written with torch.nn.functional (the grouped layer is
F.conv2d(groups=...)) on the state_dict, in whatever dtype the tensors have (fp64 for yardsticks), plus the reference-style batch-1 fp32
scoring loop of oracle.scorer with this forward in place of the ResNet one.  One switch shows that grouping is live on the rows the tests
score: `shift_groups=True` lets group g of every grouped layer read the input channels of group (g + 1) mod G.
"""
import math

import torch
import torch.nn.functional as F

import netref
from netref import cast, e2e_inputs, masked_batch  # noqa: F401  (re-exported: the tests use them through this module)

# arch -> (depth, w_0, w_a, w_m, group width) of torchvision's regnet_x_* builders
INIT = {
    "regnet_x_400mf": (22, 24, 24.48, 2.54, 16),
    "regnet_x_800mf": (16, 56, 35.73, 2.28, 16),
    "regnet_x_1_6gf": (18, 80, 34.01, 2.25, 24),
    "regnet_x_3_2gf": (25, 88, 26.31, 2.25, 48),
    "regnet_x_8gf": (23, 80, 49.56, 2.88, 120),
}
ARCHS = tuple(INIT)
# arch -> (engine id, stage widths, depths, group width, groups per stage, parameters, MAC per forward, conv entries with the fc)
TABLE = {
    "regnet_x_400mf": (14004, (32, 64, 160, 400), (1, 2, 7, 12), 16, (2, 4, 10, 25), 5495976, 413812608, 72),
    "regnet_x_800mf": (14008, (64, 128, 288, 672), (1, 3, 7, 5), 16, (4, 8, 18, 42), 7259656, 799699712, 54),
    "regnet_x_1_6gf": (14016, (72, 168, 408, 912), (2, 4, 10, 2), 24, (3, 7, 17, 38), 9190136, 1602849792, 60),
    "regnet_x_3_2gf": (14032, (96, 192, 432, 1008), (2, 6, 15, 2), 48, (2, 4, 9, 21), 15296552, 3176621952, 81),
    "regnet_x_8gf": (14080, (80, 240, 720, 1920), (2, 5, 15, 1), 120, (1, 2, 6, 16), 39572648, 7995132416, 75),
}
STEM = 32
EPS = 1e-5

# The rows the end-to-end checks score: arch -> ((label map, number of mask rows, seed of synth.random_onoff), ...)
E2E_CASES = {
    "regnet_x_400mf": (("felz", 8, 11), ("grid", 4, 5)),
    "regnet_x_800mf": (("felz", 4, 11), ("grid", 2, 5)),
    "regnet_x_1_6gf": (("felz", 4, 11), ("grid", 2, 5)),
    "regnet_x_3_2gf": (("felz", 4, 11), ("grid", 2, 5)),
    "regnet_x_8gf": (("felz", 3, 11),),
}


def _make_divisible(v, divisor):
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def block_params(arch):
    """BlockParams.from_init_params with bottleneck multiplier 1: -> (stage widths, stage depths, group width per stage)."""
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
    stage_widths = [_make_divisible(w, g) for w, g in zip(stage_widths, gws)]
    return tuple(stage_widths), tuple(stage_depths), tuple(gws)


def bn(sd, prefix, x):
    return netref.bn(sd, prefix, x, EPS)


def blocks(arch):
    """(prefix "trunk_output.blockS.blockS-J.", w_in, w, group width, stride, side of the input map, side of the output map, has proj) per block,
    from the rule (block_params), not from the table."""
    widths, depths, gws = block_params(arch)
    out, cin, h = [], STEM, 112
    for s, (w, d, gw) in enumerate(zip(widths, depths, gws)):
        for j in range(d):
            stride = 2 if j == 0 else 1
            ho = (h - 1) // stride + 1
            out.append(("trunk_output.block%d.block%d-%d." % (s + 1, s + 1, j), cin, w, gw, stride, h, ho, j == 0))
            cin, h = w, ho
    return out


def topology(arch):
    """The conv list in the engine's order: (name, bn name, cin, cout, ksize, stride, pad, hin, hout, relu, residual, groups)."""
    convs = [("stem.0", "stem.1", 3, STEM, 3, 2, 1, 224, 112, 1, 0, 1)]
    cin = STEM
    for p, cin, w, gw, stride, h, ho, proj in blocks(arch):
        if proj:
            convs.append((p + "proj.0", p + "proj.1", cin, w, 1, 2, 0, h, ho, 0, 0, 1))
        convs.append((p + "f.a.0", p + "f.a.1", cin, w, 1, 1, 0, h, h, 1, 0, 1))
        convs.append((p + "f.b.0", p + "f.b.1", w, w, 3, stride, 1, h, ho, 1, 0, w // gw))
        convs.append((p + "f.c.0", p + "f.c.1", w, w, 1, 1, 0, ho, ho, 1, 1, 1))
        cin = w
    convs.append(("fc", "", cin, 1000, 1, 1, 0, 1, 1, 0, 0, 1))
    return convs


def macs(arch):
    """Multiply-accumulates of one forward, from the conv list: a grouped layer reads cin / groups channels per output channel."""
    return sum(c[8] * c[8] * c[3] * (c[2] // c[11]) * c[4] * c[4] for c in topology(arch))


def params(arch):
    """Parameters from the conv list: weights, two per BatchNorm channel, the fc's bias."""
    return sum(c[3] * (c[2] // c[11]) * c[4] * c[4] + (2 * c[3] if c[1] else c[3]) for c in topology(arch))


def pitch(c):
    return -(-c // 32) * 32


def forward(sd, x, arch, trace=None, shift_groups=False, count=None):
    """logits [N, 1000] for the normalised NCHW batch x.  `trace` (a list) receives (name, tensor) of every block output; `count` (a
    one-element list) receives the multiply-accumulates per image, counted from the tensors each conv call actually sees."""

    def conv(x, w, stride=1, pad=0, groups=1):
        y = F.conv2d(x, w, None, stride, pad, 1, groups)
        if count is not None:
            count[0] += y.shape[1] * y.shape[2] * y.shape[3] * w.shape[1] * w.shape[2] * w.shape[3]
        return y

    x = F.relu(bn(sd, "stem.1", conv(x, sd["stem.0.weight"], 2, 1)))
    for p, _cin, w, gw, stride, _h, _ho, proj in blocks(arch):
        t = F.relu(bn(sd, p + "f.a.1", conv(x, sd[p + "f.a.0.weight"])))
        if shift_groups and w // gw > 1:
            t = t.roll(-gw, 1)              # group g reads the channels of group (g + 1) mod G
        t = F.relu(bn(sd, p + "f.b.1", conv(t, sd[p + "f.b.0.weight"], stride, 1, w // gw)))
        t = bn(sd, p + "f.c.1", conv(t, sd[p + "f.c.0.weight"]))
        idn = bn(sd, p + "proj.1", conv(x, sd[p + "proj.0.weight"], 2)) if proj else x
        x = F.relu(t + idn)
        if trace is not None:
            trace.append((p[:-1], x))
    x = torch.flatten(F.adaptive_avg_pool2d(x, 1), 1)
    if count is not None:
        count[0] += sd["fc.weight"].shape[0] * sd["fc.weight"].shape[1]
    return F.linear(x, sd["fc.weight"], sd["fc.bias"])


def bound(arch):
    """The forward of `arch` as the forward(sd, x, **switches) that netref and the test drivers take."""
    return netref.bound(forward, arch)


def score_masks_reference_loop(sd, arch, x_chw, segments, onoff, label, return_logits=False):
    """netref.score_masks_reference_loop with the RegNetX forward of `arch`."""
    return netref.score_masks_reference_loop(bound(arch), sd, x_chw, segments, onoff, label, return_logits)


def score_masks_fp64(sd, arch, x_chw, segments, onoff, label, shift_groups=False):
    """netref.score_masks_fp64 with the RegNetX forward of `arch`, 4 rows at a time."""
    return netref.score_masks_fp64(bound(arch), sd, x_chw, segments, onoff, label, chunk=4, shift_groups=shift_groups)


_E2E = {}


def e2e_rows(golden_dir, arch):
    """Per case of E2E_CASES[arch], computed once per process and shared: dict kind -> (img, seg, onoff, label, s64, logits64).  The label is
    the fp64 argmax of the unmasked picture."""
    if arch not in _E2E:
        _E2E[arch] = netref.e2e_rows(forward, E2E_CASES[arch], golden_dir, arch, chunk=4)
    return _E2E[arch]
