"""CPU restatement of torchvision's ShuffleNetV2 forward (test infrastructure only; oracle/ stays ResNet-only).

torchvision shufflenetv2.py: conv1 = Conv2d(3, 24, 3, stride 2, pad 1, no bias) + BatchNorm + ReLU; MaxPool2d(3, 2, 1); stage2 / stage3 /
stage4 of 4 / 8 / 4 InvertedResidual blocks (block 0 of a stage has stride 2); conv5 = Conv2d(., 1024 or 2048, 1) + BatchNorm + ReLU; the
mean over the 7x7 map; fc = Linear(., 1000).  A block with bf = oup / 2:
    stride 1: x1, x2 = x.chunk(2, dim=1); out = cat(x1, branch2(x2))          stride 2: out = cat(branch1(x), branch2(x))
    branch2 = 1x1 conv + BN + ReLU, depthwise 3x3 (pad 1, the block's stride) + BN, 1x1 conv + BN + ReLU
    branch1 = depthwise 3x3 stride 2 + BN, 1x1 conv + BN + ReLU
    out = channel_shuffle(out, 2)
Eval mode: every BatchNorm uses its running statistics.  Written with torch.nn.functional on the state_dict, in whatever dtype the tensors
have (fp64 for yardsticks), with torchvision's literal shuffle `view(B, 2, C / 2, H, W).transpose(1, 2)`, plus the reference-style batch-1
fp32 scoring loop of oracle.scorer with this forward in place of the ResNet one.
"""
import numpy as np
import torch
import torch.nn.functional as F

import netref
from netref import cast, e2e_inputs, masked_batch  # noqa: F401  (re-exported: the tests use them through this module)

ARCHS = ("shufflenet_v2_x0_5", "shufflenet_v2_x1_0", "shufflenet_v2_x1_5", "shufflenet_v2_x2_0")
WIDTHS = {"shufflenet_v2_x0_5": (24, 48, 96, 192, 1024), "shufflenet_v2_x1_0": (24, 116, 232, 464, 1024),
          "shufflenet_v2_x1_5": (24, 176, 352, 704, 1024), "shufflenet_v2_x2_0": (24, 244, 488, 976, 2048)}
REPEATS = (4, 8, 4)
EPS = 1e-5
PARAMS = {"shufflenet_v2_x0_5": 1366792, "shufflenet_v2_x1_0": 2278604, "shufflenet_v2_x1_5": 3503624, "shufflenet_v2_x2_0": 7393996}
MACS = {"shufflenet_v2_x0_5": 40476448, "shufflenet_v2_x1_0": 144907992, "shufflenet_v2_x1_5": 295759392, "shufflenet_v2_x2_0": 583253464}
# (bf, hp) of stage2 / stage3 / stage4: half a stage's width and that rounded up to 32
HALVES = {"shufflenet_v2_x0_5": ((24, 32), (48, 64), (96, 96)), "shufflenet_v2_x1_0": ((58, 64), (116, 128), (232, 256)),
          "shufflenet_v2_x1_5": ((88, 96), (176, 192), (352, 352)), "shufflenet_v2_x2_0": ((122, 128), (244, 256), (488, 512))}

# The rows the end-to-end checks score: (label map, number of mask rows, seed of synth.random_onoff).  tests/test_shufflenet_cpu.py asserts on
# exactly these rows that the softmax peak lies in [0.05, 0.95] and the fp64 top-two logit margin is >= 1e-3.
E2E_CASES = (("felz", 20, 11), ("grid", 8, 5))
E2E_ARCHS = ("shufflenet_v2_x1_0", "shufflenet_v2_x0_5")


def bn(sd, prefix, x):
    return netref.bn(sd, prefix, x, EPS)


def channel_shuffle(x, groups=2):
    """torchvision's: view(B, groups, C / groups, H, W), transpose(1, 2), flatten back."""
    b, c, h, w = x.shape
    return x.view(b, groups, c // groups, h, w).transpose(1, 2).contiguous().view(b, c, h, w)


def halves(arch):
    return tuple((oup // 2, -(-(oup // 2) // 32) * 32) for oup in WIDTHS[arch][1:4])


def two_half_index(bf, hp):
    """Physical channel of every logical channel l of a two-half map: l < bf at l, l >= bf at hp + (l - bf).  i64[2 bf]."""
    l = np.arange(2 * bf)
    return np.where(l < bf, l, hp + l - bf)


def shuffle_source(bf, hp):
    """The engine's shuffle as an index map: for every physical output channel q of a two-half map (pitch 2 hp), (which, index) of the source
    element -- which = 0: a, 1: b, -1: a pad channel (zero) -- with h = q // hp, j = q % hp, l = h * bf + j."""
    q = np.arange(2 * hp)
    h, j = q // hp, q % hp
    l = h * bf + j
    which = np.where(j >= bf, -1, l & 1)
    return which, np.where(j >= bf, 0, l >> 1)


def blocks(arch):
    """(stage N, block k, inp, oup, stride, side of the input map) per block."""
    w = WIDTHS[arch]
    out, inp, h = [], w[0], 56
    for s, (oup, reps) in enumerate(zip(w[1:4], REPEATS)):
        for b in range(reps):
            stride = 2 if b == 0 else 1
            out.append((s + 2, b, inp, oup, stride, h))
            inp, h = oup, (h - 1) // stride + 1
    return out


def topology(arch):
    """The network's layers in forward order.  convs: (name, bn name, cin, cout, ksize, stride, pad, hin, hout, relu, residual) for conv1,
    every 1x1 conv, conv5 and fc; depthwise: (name, bn name, channels, stride, hin)."""
    w = WIDTHS[arch]
    convs = [("conv1.0", "conv1.1", 3, w[0], 3, 2, 1, 224, 112, 1, 0)]
    dws = []
    for n, k, inp, oup, stride, h in blocks(arch):
        p = "stage%d.%d." % (n, k)
        bf, ho = oup // 2, (h - 1) // stride + 1
        if stride == 2:
            dws.append((p + "branch1.0", p + "branch1.1", inp, 2, h))
            convs.append((p + "branch1.2", p + "branch1.3", inp, bf, 1, 1, 0, ho, ho, 1, 0))
        convs.append((p + "branch2.0", p + "branch2.1", inp if stride == 2 else bf, bf, 1, 1, 0, h, h, 1, 0))
        dws.append((p + "branch2.3", p + "branch2.4", bf, stride, h))
        convs.append((p + "branch2.5", p + "branch2.6", bf, bf, 1, 1, 0, ho, ho, 1, 0))
    convs.append(("conv5.0", "conv5.1", w[3], w[4], 1, 1, 0, 7, 7, 1, 0))
    convs.append(("fc", "", w[4], 1000, 1, 1, 0, 1, 1, 0, 0))
    return convs, dws


def macs(arch):
    """Multiply-accumulates of one forward: convs, depthwise convs and fc."""
    convs, dws = topology(arch)
    m = sum(hout * hout * cout * cin * k * k for _n, _b, cin, cout, k, _s, _p, _hin, hout, _r, _res in convs)
    return m + sum(((hin - 1) // s + 1) ** 2 * c * 9 for _n, _b, c, s, hin in dws)


def branch2(sd, p, x, stride):
    c = sd[p + "branch2.3.weight"].shape[0]
    t = F.relu(bn(sd, p + "branch2.1", F.conv2d(x, sd[p + "branch2.0.weight"])))
    t = bn(sd, p + "branch2.4", F.conv2d(t, sd[p + "branch2.3.weight"], None, stride, 1, 1, c))
    return F.relu(bn(sd, p + "branch2.6", F.conv2d(t, sd[p + "branch2.5.weight"])))


def branch1(sd, p, x):
    c = sd[p + "branch1.0.weight"].shape[0]
    t = bn(sd, p + "branch1.1", F.conv2d(x, sd[p + "branch1.0.weight"], None, 2, 1, 1, c))
    return F.relu(bn(sd, p + "branch1.3", F.conv2d(t, sd[p + "branch1.2.weight"])))


def features(sd, arch, x, trace=None):
    """The trunk up to relu(bn(conv5(.))); `trace` (a list) receives (name, tensor) of conv1, the pool, every block output and conv5."""
    def note(name, t):
        if trace is not None:
            trace.append((name, t))
        return t

    x = note("conv1", F.relu(bn(sd, "conv1.1", F.conv2d(x, sd["conv1.0.weight"], None, 2, 1))))
    x = note("maxpool", F.max_pool2d(x, 3, 2, 1))
    for n, k, _inp, _oup, stride, _h in blocks(arch):
        p = "stage%d.%d." % (n, k)
        if stride == 1:
            x1, x2 = x.chunk(2, dim=1)
            out = torch.cat((x1, branch2(sd, p, x2, 1)), dim=1)
        else:
            out = torch.cat((branch1(sd, p, x), branch2(sd, p, x, 2)), dim=1)
        x = note("stage%d.%d" % (n, k), channel_shuffle(out, 2))
    return note("conv5", F.relu(bn(sd, "conv5.1", F.conv2d(x, sd["conv5.0.weight"]))))


def forward(sd, arch, x, trace=None):
    """logits [N, 1000] of torchvision's shufflenet_v2_* for the normalised NCHW batch x."""
    x = features(sd, arch, x, trace).mean([2, 3])
    return F.linear(x, sd["fc.weight"], sd["fc.bias"])


def bound(arch):
    """The forward of `arch` as the forward(sd, x) that netref and the test drivers take."""
    return lambda sd, x: forward(sd, arch, x)


def score_masks_reference_loop(sd, arch, x_chw, segments, onoff, label, return_logits=False):
    """netref.score_masks_reference_loop with the ShuffleNetV2 forward of `arch`."""
    return netref.score_masks_reference_loop(bound(arch), sd, x_chw, segments, onoff, label, return_logits)


def score_masks_fp64(sd, arch, x_chw, segments, onoff, label):
    """netref.score_masks_fp64 with the ShuffleNetV2 forward of `arch`, 8 rows at a time."""
    return netref.score_masks_fp64(bound(arch), sd, x_chw, segments, onoff, label, chunk=8)


def predict(sd, arch, x_chw):
    return netref.predict(bound(arch), sd, x_chw)
