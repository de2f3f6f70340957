"""CPU restatement of torchvision's VGG forward (test infrastructure only; oracle/ stays ResNet-only).

torchvision vgg.py: `features` = make_layers(cfg, batch_norm) -- Conv2d(3x3, padding 1, bias) [+ BatchNorm2d] + ReLU per number,
MaxPool2d(2, 2) per "M" -- then AdaptiveAvgPool2d((7, 7)), torch.flatten(x, 1) and `classifier` = Linear(25088, 4096), ReLU, Dropout,
Linear(4096, 4096), ReLU, Dropout, Linear(4096, num_classes).  Eval mode: BatchNorm uses its running statistics, Dropout is the identity.
Written with torch.nn.functional on the state_dict, in whatever dtype the tensors have (fp64 for yardsticks), plus the reference-style
batch-1 fp32 scoring loop of oracle.scorer with this forward in place of the ResNet one.
"""
import torch
import torch.nn.functional as F

from network_interpretation_imagenet_amd import synth
import netref
from netref import cast  # noqa: F401  (re-exported: the tests use it through this module)

BN_EPS = 1e-5


def features(sd, x, arch, trace=None):
    """The trunk; `trace` (a list) receives every post-ReLU map."""
    depth, bn = synth.vgg_arch(arch)
    idx = 0
    for v in synth.VGG_CFGS[depth]:
        if v == "M":
            x = F.max_pool2d(x, 2, 2)
            idx += 1
            continue
        p = "features.%d" % idx
        x = F.conv2d(x, sd[p + ".weight"], sd[p + ".bias"], 1, 1)
        if bn:
            q = "features.%d" % (idx + 1)
            x = F.batch_norm(x, sd[q + ".running_mean"], sd[q + ".running_var"], sd[q + ".weight"], sd[q + ".bias"], False, 0.0, BN_EPS)
        x = F.relu(x)
        if trace is not None:
            trace.append(x)
        idx += 3 if bn else 2
    return x


def forward(sd, x, arch, trace=None):
    """logits [N, 1000] of torchvision's VGG `arch` for the normalised NCHW batch x."""
    x = features(sd, x, arch, trace)
    x = F.adaptive_avg_pool2d(x, (7, 7))
    x = torch.flatten(x, 1)
    x = F.relu(F.linear(x, sd["classifier.0.weight"], sd["classifier.0.bias"]))
    if trace is not None:
        trace.append(x)
    x = F.relu(F.linear(x, sd["classifier.3.weight"], sd["classifier.3.bias"]))
    if trace is not None:
        trace.append(x)
    return F.linear(x, sd["classifier.6.weight"], sd["classifier.6.bias"])


def bound(arch):
    """The forward of `arch` as the forward(sd, x, **switches) that netref and the test drivers take."""
    return netref.bound(forward, arch)


def score_masks_reference_loop(sd, arch, x_chw, segments, onoff, label, return_logits=False):
    """netref.score_masks_reference_loop with the VGG forward of `arch`."""
    return netref.score_masks_reference_loop(bound(arch), sd, x_chw, segments, onoff, label, return_logits)


def score_masks_fp64(sd, arch, x_chw, segments, onoff, label):
    """netref.score_masks_fp64 with the VGG forward of `arch`, 4 rows at a time."""
    return netref.score_masks_fp64(bound(arch), sd, x_chw, segments, onoff, label, chunk=4)


def predict(sd, arch, x_chw):
    return netref.predict(bound(arch), sd, x_chw)
