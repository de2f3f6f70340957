"""CPU restatement of torchvision's VGG forward (test infrastructure only; oracle/ stays ResNet-only).

torchvision vgg.py: `features` = make_layers(cfg, batch_norm) -- Conv2d(3x3, padding 1, bias) [+ BatchNorm2d] + ReLU per number,
MaxPool2d(2, 2) per "M" -- then AdaptiveAvgPool2d((7, 7)), torch.flatten(x, 1) and `classifier` = Linear(25088, 4096), ReLU, Dropout,
Linear(4096, 4096), ReLU, Dropout, Linear(4096, num_classes).  Eval mode: BatchNorm uses its running statistics, Dropout is the identity.
Written with torch.nn.functional on the state_dict, in whatever dtype the tensors have (fp64 for yardsticks), plus the reference-style
batch-1 fp32 scoring loop of oracle.scorer with this forward in place of the ResNet one.
"""
import numpy as np
import torch
import torch.nn.functional as F

from network_interpretation_imagenet_amd import synth
from oracle.scorer import apply_mask, onoff_mask_u8

BN_EPS = 1e-5


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


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


def score_masks_reference_loop(sd, arch, x_chw, segments, onoff, label, return_logits=False):
    """oracle.scorer.score_masks_reference_loop with the VGG forward: one batch-1 fp32 forward per mask-vector.
    returns (score f32[M], pred i64[M]), and the fp32 logits f32[M, 1000] behind them when return_logits is set."""
    sd = cast(sd, torch.float32)
    m = onoff.shape[0]
    score = np.zeros(m, dtype=np.float32)
    pred = np.zeros(m, dtype=np.int64)
    rows = []
    for i in range(m):
        masked = apply_mask(x_chw, onoff_mask_u8(segments, onoff[i]))
        with torch.no_grad():
            logits = forward(sd, torch.from_numpy(masked[None]), arch)
            prob = F.softmax(logits, dim=1)
        score[i], pred[i] = prob.numpy()[0][label], int(logits.max(1, keepdim=True)[1][0, 0])
        rows.append(logits.numpy()[0])
    return (score, pred, np.stack(rows)) if return_logits else (score, pred)


def score_masks_fp64(sd, arch, x_chw, segments, onoff, label):
    """The yardstick: the same masks through the fp64 forward.  returns (score f64[M], logits f64[M, 1000])."""
    sd = cast(sd, torch.float64)
    with torch.no_grad():
        logits = torch.cat([forward(sd, torch.from_numpy(np.stack([apply_mask(x_chw, onoff_mask_u8(segments, row)) for row in onoff[i:i + 4]])).double(), arch)
                            for i in range(0, onoff.shape[0], 4)])
        prob = F.softmax(logits, dim=1)
    return prob[:, label].numpy(), logits.numpy()


def predict(sd, arch, x_chw):
    """Unmasked fp32 forward: (argmax, softmax row as f64 numpy)."""
    with torch.no_grad():
        logits = forward(cast(sd, torch.float32), x_chw[None], arch)
    return int(logits.argmax(1)[0]), F.softmax(logits.double(), dim=1)[0].numpy()
