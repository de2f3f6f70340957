"""CPU restatement of torchvision's MobileNetV2 forward (test infrastructure only; oracle/ stays ResNet-only).

torchvision mobilenetv2.py, width 1.0: features.0 = Conv2d(3, 32, 3, stride 2, pad 1, no bias) + BatchNorm + ReLU6; 17 InvertedResidual
blocks (t, c, n, s) = (1,16,1,1) (6,24,2,2) (6,32,3,2) (6,64,4,2) (6,96,3,1) (6,160,3,2) (6,320,1,1), each 1x1 expand + BN + ReLU6 (absent
when t = 1), depthwise 3x3 (pad 1, groups = hidden) + BN + ReLU6, 1x1 project + BN without activation, plus the block input when stride
is 1 and cin == cout; features.18 = Conv2d(320, 1280, 1) + BN + ReLU6; adaptive_avg_pool2d((1, 1)), flatten, classifier.1 =
Linear(1280, 1000) (classifier.0 is Dropout: nothing in eval mode).  Eval mode: every BatchNorm uses its running statistics.  Written
with torch.nn.functional on the state_dict, in whatever dtype the tensors have (fp64 for yardsticks), plus the reference-style batch-1
fp32 scoring loop of oracle.scorer with this forward in place of the ResNet one.  `act6=False` replaces every ReLU6 by ReLU (what the
tests use to show that the clamp is active on their inputs).
"""
import torch
import torch.nn.functional as F

import netref
from netref import cast, e2e_inputs, masked_batch  # noqa: F401  (re-exported: the tests use them through this module)

ARCH = "mobilenet_v2"
CFG = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))
EPS = 1e-5
PARAMS = 3504872
MACS = 300774272

# The rows the end-to-end checks score: (label map, number of mask rows, seed of synth.random_onoff).  tests/test_mobilenet_cpu.py asserts on
# exactly these rows that the fp64 top-two logit margin is >= 1e-3, so tests/test_gpu_mobilenet.py compares the argmax of every row.
E2E_CASES = (("felz", 20, 11), ("grid", 8, 5))


def bn(sd, prefix, x):
    return netref.bn(sd, prefix, x, EPS)


def blocks():
    """(index k of features.k, cin, hidden, cout, stride, side of the input map, has an expand conv, adds its input) per block."""
    out = []
    cin, h, k = 32, 112, 1
    for t, c, n, s in CFG:
        for b in range(n):
            stride = s if b == 0 else 1
            out.append((k, cin, cin * t, c, stride, h, t != 1, stride == 1 and cin == c))
            cin, h, k = c, (h - 1) // stride + 1, k + 1
    return out


def topology():
    """The network's layers in forward order.  convs: (name, bn name, cin, cout, ksize, stride, pad, hin, hout, relu, residual) for the stem,
    every expand / project conv, features.18 and the classifier -- relu = 1 where torchvision has ReLU6 behind the BatchNorm (the MFMA conv
    applies ReLU, its consumer the clamp); depthwise: (name, bn name, channels, stride, hin)."""
    convs = [("features.0.0", "features.0.1", 3, 32, 3, 2, 1, 224, 112, 1, 0)]
    dws = []
    for k, cin, hidden, cout, stride, h, expand, res in blocks():
        p = "features.%d.conv." % k
        ho = (h - 1) // stride + 1
        if expand:
            convs.append((p + "0.0", p + "0.1", cin, hidden, 1, 1, 0, h, h, 1, 0))
            dws.append((p + "1.0", p + "1.1", hidden, stride, h))
            convs.append((p + "2", p + "3", hidden, cout, 1, 1, 0, ho, ho, 0, int(res)))
        else:
            dws.append((p + "0.0", p + "0.1", hidden, stride, h))
            convs.append((p + "1", p + "2", hidden, cout, 1, 1, 0, ho, ho, 0, int(res)))
    convs.append(("features.18.0", "features.18.1", 320, 1280, 1, 1, 0, 7, 7, 1, 0))
    convs.append(("classifier.1", "", 1280, 1000, 1, 1, 0, 1, 1, 0, 0))
    return convs, dws


def macs():
    """Multiply-accumulates of one forward: convs, depthwise convs and the classifier."""
    convs, dws = topology()
    m = sum(hout * hout * cout * cin * k * k for _n, _b, cin, cout, k, _s, _p, _hin, hout, _r, _res in convs)
    return m + sum(((hin - 1) // s + 1) ** 2 * c * 9 for _n, _b, c, s, hin in dws)


def features(sd, x, trace=None, act6=True):
    """The trunk up to relu6(bn(features.18(.))); `trace` (a list) receives (name, tensor) of every post-activation map and every block output."""
    act = F.relu6 if act6 else F.relu

    def note(name, t):
        if trace is not None:
            trace.append((name, t))
        return t

    x = note("features.0", act(bn(sd, "features.0.1", F.conv2d(x, sd["features.0.0.weight"], None, 2, 1))))
    for k, _cin, hidden, _cout, stride, _h, expand, res in blocks():
        p = "features.%d.conv." % k
        t, j = x, 0
        if expand:
            t = note(p + "0", act(bn(sd, p + "0.1", F.conv2d(t, sd[p + "0.0.weight"]))))
            j = 1
        t = note(p + "%d" % j, act(bn(sd, p + "%d.1" % j, F.conv2d(t, sd[p + "%d.0.weight" % j], None, stride, 1, 1, hidden))))
        t = bn(sd, p + "%d" % (j + 2), F.conv2d(t, sd[p + "%d.weight" % (j + 1)]))
        x = note("features.%d" % k, x + t if res else t)
    return note("features.18", act(bn(sd, "features.18.1", F.conv2d(x, sd["features.18.0.weight"]))))


def forward(sd, x, trace=None, act6=True):
    """logits [N, 1000] of torchvision's mobilenet_v2 for the normalised NCHW batch x."""
    x = features(sd, x, trace, act6)
    x = torch.flatten(F.adaptive_avg_pool2d(x, (1, 1)), 1)
    return F.linear(x, sd["classifier.1.weight"], sd["classifier.1.bias"])


def score_masks_reference_loop(sd, x_chw, segments, onoff, label, return_logits=False):
    """netref.score_masks_reference_loop with the MobileNetV2 forward."""
    return netref.score_masks_reference_loop(forward, sd, x_chw, segments, onoff, label, return_logits)


def score_masks_fp64(sd, x_chw, segments, onoff, label, act6=True):
    """netref.score_masks_fp64 with the MobileNetV2 forward, 8 rows at a time."""
    return netref.score_masks_fp64(forward, sd, x_chw, segments, onoff, label, chunk=8, act6=act6)


def predict(sd, x_chw):
    return netref.predict(forward, sd, x_chw)
