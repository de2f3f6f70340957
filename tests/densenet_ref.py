"""CPU restatement of torchvision's DenseNet forward (test infrastructure only; oracle/ stays ResNet-only).

torchvision densenet.py with growth rate 32, bn_size 4 and 64 initial features: `features` = conv0 (3 -> 64, 7x7 stride 2 pad 3, no bias),
norm0, ReLU, MaxPool2d(3, 2, 1); then per block b its dense layers -- norm1 -> ReLU -> conv1 (1x1, C -> 128) -> norm2 -> ReLU -> conv2
(3x3 pad 1, 128 -> 32), the output concatenated behind the C input channels -- and, behind blocks 1 to 3, transition b = norm -> ReLU ->
conv (1x1, C -> C / 2) -> AvgPool2d(2, 2); then norm5, F.relu, adaptive_avg_pool2d((1, 1)), flatten, classifier.  Eval mode: every
BatchNorm uses its running statistics.  Written with torch.nn.functional on the state_dict, in whatever dtype the tensors have (fp64 for
yardsticks), plus the reference-style batch-1 fp32 scoring loop of oracle.scorer with this forward in place of the ResNet one.
"""
import torch
import torch.nn.functional as F

import netref
from netref import cast, e2e_inputs, masked_batch  # noqa: F401  (re-exported: the tests use them through this module)

BLOCKS = {"densenet121": (6, 12, 24, 16), "densenet169": (6, 12, 32, 32), "densenet201": (6, 12, 48, 32)}
GROWTH, MID, INIT = 32, 128, 64
EPS = 1e-5

# The rows the end-to-end checks score, per architecture: (label map, number of mask rows, seed of synth.random_onoff).  tests/test_densenet_cpu.py
# asserts on exactly these rows that the fp64 top-two logit margin is >= 1e-3, so tests/test_gpu_densenet.py compares the argmax of every row.
E2E_CASES = (("felz", 20, 11), ("grid", 8, 5))


def bn(sd, prefix, x):
    return netref.bn(sd, prefix, x, EPS)


def topology(arch):
    """Every conv in forward order as (name, cin, cout, ksize, stride, pad, hin, hout, relu) and every stand-alone BatchNorm as
    (name, channels, side of its map), generated from the block tuple."""
    convs = [("features.conv0", 3, INIT, 7, 2, 3, 224, 112, 1)]
    norms = []
    c, h = INIT, 56
    blocks = BLOCKS[arch]
    for b, n in enumerate(blocks):
        for j in range(n):
            p = "features.denseblock%d.denselayer%d." % (b + 1, j + 1)
            norms.append((p + "norm1", c, h))
            convs.append((p + "conv1", c, MID, 1, 1, 0, h, h, 1))
            convs.append((p + "conv2", MID, GROWTH, 3, 1, 1, h, h, 0))
            c += GROWTH
        if b + 1 < len(blocks):
            p = "features.transition%d." % (b + 1)
            norms.append((p + "norm", c, h))
            convs.append((p + "conv", c, c // 2, 1, 1, 0, h, h, 0))
            c //= 2
            h //= 2
    norms.append(("features.norm5", c, h))
    convs.append(("classifier", c, 1000, 1, 1, 0, 1, 1, 0))
    return convs, norms


def macs(arch):
    """Multiply-accumulates of the convs and the classifier of one forward, in torchvision's order (a transition's conv runs before its pool)."""
    return sum(hout * hout * cout * cin * k * k for _n, cin, cout, k, _s, _p, _hin, hout, _r in topology(arch)[0])


def features(sd, arch, x, trace=None):
    """The trunk up to relu(norm5(.)); `trace` (a list) receives every post-ReLU map a conv reads and the final one."""
    x = F.conv2d(x, sd["features.conv0.weight"], None, 2, 3)
    x = F.max_pool2d(F.relu(bn(sd, "features.norm0", x)), 3, 2, 1)
    blocks = BLOCKS[arch]
    for b, n in enumerate(blocks):
        for j in range(n):
            p = "features.denseblock%d.denselayer%d." % (b + 1, j + 1)
            t = F.relu(bn(sd, p + "norm1", x))
            if trace is not None:
                trace.append(t)
            t = F.relu(bn(sd, p + "norm2", F.conv2d(t, sd[p + "conv1.weight"])))
            if trace is not None:
                trace.append(t)
            x = torch.cat([x, F.conv2d(t, sd[p + "conv2.weight"], None, 1, 1)], 1)
        if b + 1 < len(blocks):
            p = "features.transition%d." % (b + 1)
            t = F.relu(bn(sd, p + "norm", x))
            if trace is not None:
                trace.append(t)
            x = F.avg_pool2d(F.conv2d(t, sd[p + "conv.weight"]), 2, 2)
    x = F.relu(bn(sd, "features.norm5", x))
    if trace is not None:
        trace.append(x)
    return x


def forward(sd, arch, x, trace=None):
    """logits [N, 1000] of torchvision's DenseNet `arch` for the normalised NCHW batch x."""
    x = features(sd, arch, x, trace)
    x = torch.flatten(F.adaptive_avg_pool2d(x, (1, 1)), 1)
    return F.linear(x, sd["classifier.weight"], sd["classifier.bias"])


def bound(arch):
    """The forward of `arch` as the forward(sd, x) that netref and the test drivers take."""
    return lambda sd, x: forward(sd, arch, x)


def score_masks_reference_loop(sd, arch, x_chw, segments, onoff, label, return_logits=False):
    """netref.score_masks_reference_loop with the DenseNet forward of `arch`."""
    return netref.score_masks_reference_loop(bound(arch), sd, x_chw, segments, onoff, label, return_logits)


def score_masks_fp64(sd, arch, x_chw, segments, onoff, label):
    """netref.score_masks_fp64 with the DenseNet forward of `arch`, 8 rows at a time."""
    return netref.score_masks_fp64(bound(arch), sd, x_chw, segments, onoff, label, chunk=8)


def predict(sd, arch, x_chw):
    return netref.predict(bound(arch), sd, x_chw)
