"""CPU restatement of torchvision's EfficientNet-B0 forward (test infrastructure only; oracle/ stays ResNet-only).

torchvision efficientnet.py, efficientnet_b0 in eval mode: features.0 = Conv2d(3, 32, 3, stride 2, pad 1, no bias) + BatchNorm + SiLU; 16
MBConv blocks features.S.B over the seven stages of CFG, each `block` = 1x1 expand + BN + SiLU (absent when the expand ratio is 1),
depthwise k x k (pad (k - 1) / 2, groups = expanded width) + BN + SiLU, SqueezeExcitation(expanded, max(1, cin // 4)) -- gate =
sigmoid(fc2(silu(fc1(avgpool(x))))), fc1 / fc2 1x1 convs with bias, output gate * x --, 1x1 project + BN without activation, plus the block
input when stride is 1 and cin == cout; features.8 = Conv2d(320, 1280, 1) + BN + SiLU; adaptive_avg_pool2d(1), flatten, classifier.1 =
Linear(1280, 1000) (classifier.0 is Dropout and StochasticDepth sits behind every block: nothing in eval mode).  BatchNorm eps 1e-5, running
statistics.  Written with torch.nn.functional on the state_dict, in whatever dtype the tensors have (fp64 for yardsticks), plus the
reference-style batch-1 fp32 scoring loop of oracle.scorer with this forward in place of the ResNet one.  Two switches show that the new
arithmetic is live on the rows the tests score: `silu=False` replaces every SiLU by the identity, `gate=0.5` (any float) replaces every SE
gate by that constant.
"""
import torch
import torch.nn.functional as F

import netref
from netref import cast, e2e_inputs, masked_batch  # noqa: F401  (re-exported: the tests use them through this module)

ARCH = "efficientnet_b0"
# (expand ratio t, kernel k, stride of the first block s, input channels, output channels, blocks n) of stages 1 .. 7
CFG = ((1, 3, 1, 32, 16, 1), (6, 3, 2, 16, 24, 2), (6, 5, 2, 24, 40, 2), (6, 3, 2, 40, 80, 3), (6, 5, 1, 80, 112, 3), (6, 5, 2, 112, 192, 4),
       (6, 3, 1, 192, 320, 1))
EPS = 1e-5
PARAMS = 5288548
MACS = 385814752

# The rows the end-to-end checks score: (label map, number of mask rows, seed of synth.random_onoff) -- mobilenet_ref.E2E_CASES.
E2E_CASES = (("felz", 20, 11), ("grid", 8, 5))


def bn(sd, prefix, x):
    return netref.bn(sd, prefix, x, EPS)


def blocks():
    """(stage S, block B, cin, expanded width e, cout, kernel, stride, side of the input map, side of the output map, squeeze width q, adds its
    input) per block."""
    out = []
    h = 112
    for s, (t, k, st, cin, cout, n) in enumerate(CFG):
        for b in range(n):
            stride = st if b == 0 else 1
            ho = (h - 1) // stride + 1
            out.append((s + 1, b, cin, cin * t, cout, k, stride, h, ho, max(1, cin // 4), stride == 1 and cin == cout))
            cin, h = cout, ho
    return out


def topology():
    """The network's layers in forward order.  convs: (name, bn name, cin, cout, ksize, stride, pad, hin, hout, relu, residual, consumer act)
    for the stem, every expand / project conv, features.8 and the classifier -- relu is 0 everywhere, consumer act is 1 where torchvision has
    SiLU behind the BatchNorm (the MFMA conv stores the pre-activation, its consumer takes the SiLU); depthwise: (name, bn name, channels,
    kernel, stride, hin); se: (name, channels, q, side of the map)."""
    convs = [("features.0.0", "features.0.1", 3, 32, 3, 2, 1, 224, 112, 0, 0, 1)]
    dws, ses = [], []
    for s, b, cin, e, cout, k, stride, h, ho, q, res in blocks():
        p = "features.%d.%d.block." % (s, b)
        j = 0
        if e != cin:
            convs.append((p + "0.0", p + "0.1", cin, e, 1, 1, 0, h, h, 0, 0, 1))
            j = 1
        dws.append((p + "%d.0" % j, p + "%d.1" % j, e, k, stride, h))
        ses.append((p + "%d" % (j + 1), e, q, ho))
        convs.append((p + "%d.0" % (j + 2), p + "%d.1" % (j + 2), e, cout, 1, 1, 0, ho, ho, 0, int(res), 0))
    convs.append(("features.8.0", "features.8.1", 320, 1280, 1, 1, 0, 7, 7, 0, 0, 1))
    convs.append(("classifier.1", "", 1280, 1000, 1, 1, 0, 1, 1, 0, 0, 0))
    return convs, dws, ses


def macs():
    """Multiply-accumulates of one forward: convs, depthwise convs, the SE layers' two FCs (2 e q each) and the classifier."""
    convs, dws, ses = topology()
    m = sum(c[8] * c[8] * c[3] * c[2] * c[4] * c[4] for c in convs)
    m += sum(((hin - 1) // s + 1) ** 2 * c * k * k for _n, _b, c, k, s, hin in dws)
    return m + sum(2 * e * q for _n, e, q, _h in ses)


def features(sd, x, trace=None, silu=True, gate=None):
    """The trunk up to silu(bn(features.8(.))); `trace` (a list) receives (name, tensor) of every post-activation map, every SE gate
    ("<se name>.gate") and every block output."""
    act = F.silu if silu else (lambda t: t)

    def note(name, t):
        if trace is not None:
            trace.append((name, t))
        return t

    x = note("features.0", act(bn(sd, "features.0.1", F.conv2d(x, sd["features.0.0.weight"], None, 2, 1))))
    for s, b, cin, e, _cout, k, stride, _h, _ho, _q, res in blocks():
        p = "features.%d.%d.block." % (s, b)
        t, j = x, 0
        if e != cin:
            t = note(p + "0", act(bn(sd, p + "0.1", F.conv2d(t, sd[p + "0.0.weight"]))))
            j = 1
        t = note(p + "%d" % j, act(bn(sd, p + "%d.1" % j, F.conv2d(t, sd[p + "%d.0.weight" % j], None, stride, (k - 1) // 2, 1, e))))
        se = p + "%d" % (j + 1)
        if gate is None:
            z = F.conv2d(F.adaptive_avg_pool2d(t, 1), sd[se + ".fc1.weight"], sd[se + ".fc1.bias"])
            g = torch.sigmoid(F.conv2d(act(z), sd[se + ".fc2.weight"], sd[se + ".fc2.bias"]))
        else:
            g = torch.full((t.shape[0], e, 1, 1), float(gate), dtype=t.dtype)
        note(se + ".gate", g)
        t = g * t
        t = bn(sd, p + "%d.1" % (j + 2), F.conv2d(t, sd[p + "%d.0.weight" % (j + 2)]))
        x = note("features.%d.%d" % (s, b), x + t if res else t)
    return note("features.8", act(bn(sd, "features.8.1", F.conv2d(x, sd["features.8.0.weight"]))))


def forward(sd, x, trace=None, silu=True, gate=None):
    """logits [N, 1000] of torchvision's efficientnet_b0 for the normalised NCHW batch x."""
    x = features(sd, x, trace, silu, gate)
    x = torch.flatten(F.adaptive_avg_pool2d(x, 1), 1)
    return F.linear(x, sd["classifier.1.weight"], sd["classifier.1.bias"])


def score_masks_reference_loop(sd, x_chw, segments, onoff, label, return_logits=False):
    """netref.score_masks_reference_loop with the EfficientNet-B0 forward."""
    return netref.score_masks_reference_loop(forward, sd, x_chw, segments, onoff, label, return_logits)


def score_masks_fp64(sd, x_chw, segments, onoff, label, silu=True, gate=None):
    """netref.score_masks_fp64 with the EfficientNet-B0 forward, 8 rows at a time."""
    return netref.score_masks_fp64(forward, sd, x_chw, segments, onoff, label, chunk=8, silu=silu, gate=gate)


def predict(sd, x_chw):
    return netref.predict(forward, sd, x_chw)
