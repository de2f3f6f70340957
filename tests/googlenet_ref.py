"""CPU restatement of torchvision's GoogLeNet forward (test infrastructure only; oracle/ stays ResNet-only).

torchvision googlenet.py with aux_logits off, in eval mode, transform_input off: conv1 = BasicConv2d(3, 64, 7, stride 2, pad 3) | maxpool1 =
MaxPool2d(3, 2, ceil_mode=True) | conv2 = BasicConv2d(64, 64, 1) | conv3 = BasicConv2d(64, 192, 3, pad 1) | maxpool2 (3, 2, ceil) |
inception3a, 3b | maxpool3 (3, 2, ceil) | inception4a .. 4e | maxpool4 = MaxPool2d(2, 2, ceil_mode=True) | inception5a, 5b |
AdaptiveAvgPool2d((1, 1)) | flatten | Dropout (nothing in eval mode) | fc = Linear(1024, 1000).
BasicConv2d = Conv2d(bias=False) + BatchNorm2d(eps=0.001) + ReLU.
Inception(in, c1, r3, c3, r5, c5, pp) = cat(branch1: 1x1 in -> c1 | branch2: 1x1 in -> r3, 3x3 pad 1 r3 -> c3 | branch3: 1x1 in -> r5, 3x3 pad 1
r5 -> c5 (torchvision's 3x3 where the paper has 5x5) | branch4: MaxPool2d(3, 1, 1, ceil_mode=True), 1x1 in -> pp) along the channels.

The three stride-2 pools run on 112, 56 and 28: hin - 3 is odd, so ceil mode gives 56 / 28 / 14 where floor mode gives 55 / 27 / 13, and
the last window hangs over the edge.  Written with torch.nn.functional on the state_dict, in whatever dtype the tensors have (fp64 for
yardsticks), plus the reference-style batch-1 fp32 scoring loop of oracle.scorer with this forward in place of the ResNet one.
"""
import torch
import torch.nn.functional as F

import netref
from netref import cast, e2e_inputs, masked_batch  # noqa: F401  (re-exported: the tests use them through this module)

ARCH = "googlenet"
BN_EPS = 1e-3
# (name, in, c1, r3, c3, r5, c5, pp, side of the map the module runs on)
MODULES = (("inception3a", 192, 64, 96, 128, 16, 32, 32, 28), ("inception3b", 256, 128, 128, 192, 32, 96, 64, 28),
           ("inception4a", 480, 192, 96, 208, 16, 48, 64, 14), ("inception4b", 512, 160, 112, 224, 24, 64, 64, 14),
           ("inception4c", 512, 128, 128, 256, 24, 64, 64, 14), ("inception4d", 512, 112, 144, 288, 32, 64, 64, 14),
           ("inception4e", 528, 256, 160, 320, 32, 128, 128, 14), ("inception5a", 832, 256, 160, 320, 32, 128, 128, 7),
           ("inception5b", 832, 384, 192, 384, 48, 128, 128, 7))
BRANCHES = ("branch1", "branch2.0", "branch2.1", "branch3.0", "branch3.1", "branch4.1")
PARAMS = 6624904            # torchvision's published figure
MACS = 1498376192           # the 57 convs and fc

# The rows the end-to-end checks score: (label map, number of mask rows, seed of synth.random_onoff), as tests/squeezenet_ref.py.
# tests/test_googlenet_cpu.py asserts on exactly these rows that the fp64 top-two logit margin is >= 1e-3.
E2E_CASES = (("felz", 20, 11), ("grid", 8, 5))


def pad32(c):
    return -(-c // 32) * 32


def pool_side(hin, k, stride, pad, ceil_mode=True):
    """PyTorch's pooling_output_shape."""
    span = hin + 2 * pad - k
    ho = (-(-span // stride) if ceil_mode else span // stride) + 1
    if ceil_mode and (ho - 1) * stride >= hin + pad:
        ho -= 1
    return ho


def topology():
    """The 58 entries of the conv list in forward order: (name, bn name, cin, cout, ksize, stride, pad, hin, hout, relu, residual)."""
    convs = [("conv1.conv", "conv1.bn", 3, 64, 7, 2, 3, 224, 112, 1, 0), ("conv2.conv", "conv2.bn", 64, 64, 1, 1, 0, 56, 56, 1, 0),
             ("conv3.conv", "conv3.bn", 64, 192, 3, 1, 1, 56, 56, 1, 0)]
    for name, cin, c1, r3, c3, r5, c5, pp, h in MODULES:
        for br, ci, co, k in (("branch1", cin, c1, 1), ("branch2.0", cin, r3, 1), ("branch2.1", r3, c3, 3), ("branch3.0", cin, r5, 1),
                              ("branch3.1", r5, c5, 3), ("branch4.1", cin, pp, 1)):
            convs.append(("%s.%s.conv" % (name, br), "%s.%s.bn" % (name, br), ci, co, k, 1, k // 2, h, h, 1, 0))
    convs.append(("fc", "", 1024, 1000, 1, 1, 0, 1, 1, 0, 0))
    return convs


def out_slices():
    """(row pitch, channel offset, stored channels) of every conv's output planes.  The last conv of each branch writes its range of the
    module's concatenation, whose pitch is the concatenation's width rounded up to 32 (544 for inception4d's 528) and whose last slice
    (branch4.1) also stores the pad channels, as zeros; every other layer fills whole rows of its own planes (widths rounded up to 32: 16, 24,
    48, 112, 144 -> 32, 32, 64, 128, 160)."""
    out = [(64, 0, 64), (64, 0, 64), (192, 0, 192)]
    for _name, _cin, c1, r3, c3, r5, c5, pp, _h in MODULES:
        width = c1 + c3 + c5 + pp
        p = pad32(width)
        out += [(p, 0, c1), (pad32(r3), 0, pad32(r3)), (p, c1, c3), (pad32(r5), 0, pad32(r5)), (p, c1 + c3, c5),
                (p, c1 + c3 + c5, pp + p - width)]
    return out + [(1000, 0, 1000)]


def clip_pools():
    """(hin, stride, pad, pitch) of the twelve clipped 3x3 max pools in forward order."""
    out = [(112, 2, 0, 64), (56, 2, 0, 192)]
    for name, cin, *_rest, h in MODULES:
        if name == "inception4a":
            out.append((28, 2, 0, pad32(cin)))
        out.append((h, 1, 1, pad32(cin)))
    return out


def macs():
    return sum(hout * hout * cout * cin * k * k for _n, _b, cin, cout, k, _s, _p, _hin, hout, _r, _res in topology())


def basic(sd, name, x, stride=1, pad=0, eps=BN_EPS):
    x = F.conv2d(x, sd[name + ".conv.weight"], None, stride, pad)
    b = name + ".bn."
    return F.relu(F.batch_norm(x, sd[b + "running_mean"], sd[b + "running_var"], sd[b + "weight"], sd[b + "bias"], False, 0.0, eps))


def inception(sd, p, x, ceil_mode=True):
    b1 = basic(sd, p + ".branch1", x)
    b2 = basic(sd, p + ".branch2.1", basic(sd, p + ".branch2.0", x), 1, 1)
    b3 = basic(sd, p + ".branch3.1", basic(sd, p + ".branch3.0", x), 1, 1)
    b4 = basic(sd, p + ".branch4.1", F.max_pool2d(x, 3, 1, 1, 1, ceil_mode))
    return torch.cat([b1, b2, b3, b4], 1)


def features(sd, x, trace=None, ceil_mode=True):
    """The trunk up to inception5b; `trace` (a list) receives (name, tensor) of the three convs, every pool and every module output."""

    def note(name, t):
        if trace is not None:
            trace.append((name, t))
        return t

    x = note("conv1", basic(sd, "conv1", x, 2, 3))
    x = note("maxpool1", F.max_pool2d(x, 3, 2, 0, 1, ceil_mode))
    x = note("conv2", basic(sd, "conv2", x))
    x = note("conv3", basic(sd, "conv3", x, 1, 1))
    x = note("maxpool2", F.max_pool2d(x, 3, 2, 0, 1, ceil_mode))
    for name, *_rest in MODULES:
        if name == "inception4a":
            x = note("maxpool3", F.max_pool2d(x, 3, 2, 0, 1, ceil_mode))
        if name == "inception5a":
            x = note("maxpool4", F.max_pool2d(x, 2, 2, 0, 1, ceil_mode))
        x = note(name, inception(sd, name, x, ceil_mode))
    return x


def forward(sd, x, trace=None, ceil_mode=True):
    """logits [N, 1000] of torchvision's googlenet (aux_logits off, transform_input off, eval) for the normalised NCHW batch x."""
    x = features(sd, x, trace, ceil_mode)
    x = torch.flatten(F.adaptive_avg_pool2d(x, (1, 1)), 1)
    return F.linear(x, sd["fc.weight"], sd["fc.bias"])


def score_masks_reference_loop(sd, x_chw, segments, onoff, label, return_logits=False):
    """netref.score_masks_reference_loop with the GoogLeNet forward."""
    return netref.score_masks_reference_loop(forward, sd, x_chw, segments, onoff, label, return_logits)


def score_masks_fp64(sd, x_chw, segments, onoff, label):
    """netref.score_masks_fp64 with the GoogLeNet forward, 8 rows at a time."""
    return netref.score_masks_fp64(forward, sd, x_chw, segments, onoff, label, chunk=8)


def predict(sd, x_chw):
    return netref.predict(forward, sd, x_chw)
