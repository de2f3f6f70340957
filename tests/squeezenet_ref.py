"""CPU restatement of torchvision's SqueezeNet 1.1 forward (test infrastructure only; oracle/ stays ResNet-only).

torchvision squeezenet.py, version "1_1": features.0 = Conv2d(3, 64, 3, stride 2) (no padding: 224 -> 111) + ReLU; MaxPool2d(3, 2,
ceil_mode=True) at features.2 / .5 / .8 (111 -> 55 -> 27 -> 13); eight Fire modules features.N = Fire(cin, s, e, e) for (N, cin, s, e) =
(3,64,16,64) (4,128,16,64) (6,128,32,128) (7,256,32,128) (9,256,48,192) (10,384,48,192) (11,384,64,256) (12,512,64,256), each
relu(squeeze 1x1) -> cat(relu(expand1x1), relu(expand3x3 pad 1)) along the channels; classifier = Dropout (nothing in eval mode),
classifier.1 = Conv2d(512, 1000, 1), ReLU, AdaptiveAvgPool2d((1, 1)); flatten.  Every conv has a bias; there is no BatchNorm.

In all three pools hin - 3 is even (108, 52, 24), so the ceil-mode output size equals the floor-mode one and every window lies inside the
map: `ceil_mode=False` gives the same maps (tests/test_squeezenet_cpu.py asserts it), which is why the engine runs its unpadded floor-mode
3x3 stride-2 pool.  Written with torch.nn.functional on the state_dict, in whatever dtype the tensors have (fp64 for yardsticks), plus the
reference-style batch-1 fp32 scoring loop of oracle.scorer with this forward in place of the ResNet one.
"""
import torch
import torch.nn.functional as F

import netref
from netref import cast, e2e_inputs, masked_batch  # noqa: F401  (re-exported: the tests use them through this module)

ARCH = "squeezenet1_1"
FIRES = ((3, 64, 16, 64), (4, 128, 16, 64), (6, 128, 32, 128), (7, 256, 32, 128), (9, 256, 48, 192), (10, 384, 48, 192),
         (11, 384, 64, 256), (12, 512, 64, 256))
POOLS_BEFORE = (3, 6, 9)        # a max pool (features.2 / .5 / .8) sits in front of these Fire modules
PARAMS = 1235496
MACS = 349151936

# The rows the end-to-end checks score: (label map, number of mask rows, seed of synth.random_onoff), as tests/mobilenet_ref.py.
# tests/test_squeezenet_cpu.py asserts on exactly these rows that the fp64 top-two logit margin is >= 1e-3.
E2E_CASES = (("felz", 20, 11), ("grid", 8, 5))


def fire_sides():
    """(N, cin, s, e, side of the map the module runs on) per Fire module."""
    out, h = [], 111
    for n, cin, s, e in FIRES:
        if n in POOLS_BEFORE:
            h = (h - 3) // 2 + 1
        out.append((n, cin, s, e, h))
    return out


def topology():
    """The 26 convs in forward order: (name, bn name, cin, cout, ksize, stride, pad, hin, hout, relu, residual)."""
    convs = [("features.0", "", 3, 64, 3, 2, 0, 224, 111, 1, 0)]
    for n, cin, s, e, h in fire_sides():
        p = "features.%d." % n
        convs.append((p + "squeeze", "", cin, s, 1, 1, 0, h, h, 1, 0))
        convs.append((p + "expand1x1", "", s, e, 1, 1, 0, h, h, 1, 0))
        convs.append((p + "expand3x3", "", s, e, 3, 1, 1, h, h, 1, 0))
    convs.append(("classifier.1", "", 512, 1000, 1, 1, 0, 13, 13, 1, 0))
    return convs


def out_slices():
    """(row pitch, channel offset) of every conv's output planes: an expand conv writes its half of the Fire concatenation (pitch 2e, offset
    0 or e); every other layer a whole row of its own planes (squeeze widths 16 and 48 stored with pitch 32 and 64)."""
    out = []
    for name, _bn, _cin, cout, *_rest in topology():
        if name.endswith("expand1x1"):
            out.append((2 * cout, 0))
        elif name.endswith("expand3x3"):
            out.append((2 * cout, cout))
        else:
            out.append((cout if name == "classifier.1" else -(-cout // 32) * 32, 0))
    return out


def macs():
    return sum(hout * hout * cout * cin * k * k for _n, _b, cin, cout, k, _s, _p, _hin, hout, _r, _res in topology())


def fire(sd, p, x):
    s = F.relu(F.conv2d(x, sd[p + "squeeze.weight"], sd[p + "squeeze.bias"]))
    return torch.cat([F.relu(F.conv2d(s, sd[p + "expand1x1.weight"], sd[p + "expand1x1.bias"])),
                      F.relu(F.conv2d(s, sd[p + "expand3x3.weight"], sd[p + "expand3x3.bias"], 1, 1))], 1)


def features(sd, x, trace=None, ceil_mode=True):
    """The trunk up to features.12; `trace` (a list) receives (name, tensor) of the stem, every pool and every Fire output."""

    def note(name, t):
        if trace is not None:
            trace.append((name, t))
        return t

    x = note("features.0", F.relu(F.conv2d(x, sd["features.0.weight"], sd["features.0.bias"], 2)))
    for n, _cin, _s, _e in FIRES:
        if n in POOLS_BEFORE:
            x = note("features.%d" % (n - 1), F.max_pool2d(x, 3, 2, 0, 1, ceil_mode))
        x = note("features.%d" % n, fire(sd, "features.%d." % n, x))
    return x


def forward(sd, x, trace=None, ceil_mode=True):
    """logits [N, 1000] of torchvision's squeezenet1_1 for the normalised NCHW batch x."""
    x = features(sd, x, trace, ceil_mode)
    x = F.relu(F.conv2d(x, sd["classifier.1.weight"], sd["classifier.1.bias"]))
    return torch.flatten(F.adaptive_avg_pool2d(x, (1, 1)), 1)


def score_masks_reference_loop(sd, x_chw, segments, onoff, label, return_logits=False):
    """netref.score_masks_reference_loop with the SqueezeNet forward."""
    return netref.score_masks_reference_loop(forward, sd, x_chw, segments, onoff, label, return_logits)


def score_masks_fp64(sd, x_chw, segments, onoff, label):
    """netref.score_masks_fp64 with the SqueezeNet forward, 8 rows at a time."""
    return netref.score_masks_fp64(forward, sd, x_chw, segments, onoff, label, chunk=8)


def predict(sd, x_chw):
    return netref.predict(forward, sd, x_chw)
