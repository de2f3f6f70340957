"""CPU restatement of torchvision's AlexNet forward (test infrastructure only; oracle/ stays ResNet-only).

torchvision alexnet.py: `features` = Conv2d(3, 64, 11, stride 4, padding 2), ReLU, MaxPool2d(3, 2), Conv2d(64, 192, 5, padding 2), ReLU,
MaxPool2d(3, 2), Conv2d(192, 384, 3, padding 1), ReLU, Conv2d(384, 256, 3, padding 1), ReLU, Conv2d(256, 256, 3, padding 1), ReLU,
MaxPool2d(3, 2); then AdaptiveAvgPool2d((6, 6)), torch.flatten(x, 1) and `classifier` = Dropout, Linear(9216, 4096), ReLU, Dropout,
Linear(4096, 4096), ReLU, Linear(4096, num_classes).  Eval mode: Dropout is the identity.  Written with torch.nn.functional on the
state_dict, in whatever dtype the tensors have (fp64 for yardsticks), plus the reference-style batch-1 fp32 scoring loop of oracle.scorer
with this forward in place of the ResNet one.
"""
import torch
import torch.nn.functional as F

import netref
from netref import cast, masked_batch  # noqa: F401  (re-exported: the tests use them through this module)

# (state_dict prefix, stride, padding, max pool behind the ReLU) of the five convs of `features`
FEATURES = (("features.0", 4, 2, True), ("features.3", 1, 2, True), ("features.6", 1, 1, False), ("features.8", 1, 1, False),
            ("features.10", 1, 1, True))


def features(sd, x, trace=None):
    """The trunk; `trace` (a list) receives every post-ReLU map (before its pool)."""
    for p, stride, pad, pool in FEATURES:
        x = F.relu(F.conv2d(x, sd[p + ".weight"], sd[p + ".bias"], stride, pad))
        if trace is not None:
            trace.append(x)
        if pool:
            x = F.max_pool2d(x, 3, 2)
    return x


def forward(sd, x, trace=None):
    """logits [N, 1000] of torchvision's AlexNet for the normalised NCHW batch x."""
    x = features(sd, x, trace)
    x = F.adaptive_avg_pool2d(x, (6, 6))
    x = torch.flatten(x, 1)
    x = F.relu(F.linear(x, sd["classifier.1.weight"], sd["classifier.1.bias"]))
    if trace is not None:
        trace.append(x)
    x = F.relu(F.linear(x, sd["classifier.4.weight"], sd["classifier.4.bias"]))
    if trace is not None:
        trace.append(x)
    return F.linear(x, sd["classifier.6.weight"], sd["classifier.6.bias"])


def score_masks_reference_loop(sd, x_chw, segments, onoff, label, return_logits=False):
    """netref.score_masks_reference_loop with the AlexNet forward."""
    return netref.score_masks_reference_loop(forward, sd, x_chw, segments, onoff, label, return_logits)


def score_masks_fp64(sd, x_chw, segments, onoff, label):
    """netref.score_masks_fp64 with the AlexNet forward, 16 rows at a time."""
    return netref.score_masks_fp64(forward, sd, x_chw, segments, onoff, label, chunk=16)


def predict(sd, x_chw):
    return netref.predict(forward, sd, x_chw)
