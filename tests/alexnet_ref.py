"""CPU restatement of torchvision's AlexNet forward (test infrastructure only; oracle/ stays ResNet-only).

torchvision alexnet.py: `features` = Conv2d(3, 64, 11, stride 4, padding 2), ReLU, MaxPool2d(3, 2), Conv2d(64, 192, 5, padding 2), ReLU,
MaxPool2d(3, 2), Conv2d(192, 384, 3, padding 1), ReLU, Conv2d(384, 256, 3, padding 1), ReLU, Conv2d(256, 256, 3, padding 1), ReLU,
MaxPool2d(3, 2); then AdaptiveAvgPool2d((6, 6)), torch.flatten(x, 1) and `classifier` = Dropout, Linear(9216, 4096), ReLU, Dropout,
Linear(4096, 4096), ReLU, Linear(4096, num_classes).  Eval mode: Dropout is the identity.  Written with torch.nn.functional on the
state_dict, in whatever dtype the tensors have (fp64 for yardsticks), plus the reference-style batch-1 fp32 scoring loop of oracle.scorer
with this forward in place of the ResNet one.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.scorer import apply_mask, onoff_mask_u8

# (state_dict prefix, stride, padding, max pool behind the ReLU) of the five convs of `features`
FEATURES = (("features.0", 4, 2, True), ("features.3", 1, 2, True), ("features.6", 1, 1, False), ("features.8", 1, 1, False),
            ("features.10", 1, 1, True))


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


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


def masked_batch(x_chw, segments, onoff):
    """f32[M, 3, 224, 224]: the masked images of the rows of `onoff`, as oracle.scorer stages them."""
    return torch.from_numpy(np.stack([apply_mask(x_chw, onoff_mask_u8(segments, row)) for row in onoff]))


def score_masks_reference_loop(sd, x_chw, segments, onoff, label, return_logits=False):
    """oracle.scorer.score_masks_reference_loop with the AlexNet forward: one batch-1 fp32 forward per mask-vector.
    returns (score f32[M], pred i64[M]), and the fp32 logits f32[M, 1000] behind them when return_logits is set."""
    sd = cast(sd, torch.float32)
    m = onoff.shape[0]
    score = np.zeros(m, dtype=np.float32)
    pred = np.zeros(m, dtype=np.int64)
    rows = []
    for i in range(m):
        masked = apply_mask(x_chw, onoff_mask_u8(segments, onoff[i]))
        with torch.no_grad():
            logits = forward(sd, torch.from_numpy(masked[None]))
            prob = F.softmax(logits, dim=1)
        score[i], pred[i] = prob.numpy()[0][label], int(logits.max(1, keepdim=True)[1][0, 0])
        rows.append(logits.numpy()[0])
    return (score, pred, np.stack(rows)) if return_logits else (score, pred)


def score_masks_fp64(sd, x_chw, segments, onoff, label):
    """The yardstick: the same masks through the fp64 forward.  returns (score f64[M], logits f64[M, 1000])."""
    sd = cast(sd, torch.float64)
    with torch.no_grad():
        logits = torch.cat([forward(sd, masked_batch(x_chw, segments, onoff[i:i + 16]).double()) for i in range(0, onoff.shape[0], 16)])
        prob = F.softmax(logits, dim=1)
    return prob[:, label].numpy(), logits.numpy()


def predict(sd, x_chw):
    """Unmasked fp32 forward: (argmax, softmax row as f64 numpy)."""
    with torch.no_grad():
        logits = forward(cast(sd, torch.float32), x_chw[None])
    return int(logits.argmax(1)[0]), F.softmax(logits.double(), dim=1)[0].numpy()
