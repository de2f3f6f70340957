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
import numpy as np
import torch
import torch.nn.functional as F

from oracle.scorer import apply_mask, onoff_mask_u8

ARCH = "squeezenet1_1"
FIRES = ((3, 64, 16, 64), (4, 128, 16, 64), (6, 128, 32, 128), (7, 256, 32, 128), (9, 256, 48, 192), (10, 384, 48, 192),
         (11, 384, 64, 256), (12, 512, 64, 256))
POOLS_BEFORE = (3, 6, 9)        # a max pool (features.2 / .5 / .8) sits in front of these Fire modules
PARAMS = 1235496
MACS = 349151936

# The rows the end-to-end checks score: (label map, number of mask rows, seed of synth.random_onoff), as tests/mobilenet_ref.py.
# tests/test_squeezenet_cpu.py asserts on exactly these rows that the fp64 top-two logit margin is >= 1e-3.
E2E_CASES = (("felz", 20, 11), ("grid", 8, 5))


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


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


def masked_batch(x_chw, segments, onoff):
    """f32[M, 3, 224, 224]: the masked images of the rows of `onoff`, as oracle.scorer stages them."""
    return torch.from_numpy(np.stack([apply_mask(x_chw, onoff_mask_u8(segments, row)) for row in onoff]))


def score_masks_reference_loop(sd, x_chw, segments, onoff, label, return_logits=False):
    """oracle.scorer.score_masks_reference_loop with the SqueezeNet forward: one batch-1 fp32 forward per mask-vector.
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
        logits = torch.cat([forward(sd, masked_batch(x_chw, segments, onoff[i:i + 8]).double()) for i in range(0, onoff.shape[0], 8)])
        prob = F.softmax(logits, dim=1)
    return prob[:, label].numpy(), logits.numpy()


def predict(sd, x_chw):
    """Unmasked fp32 forward: (argmax, softmax row as f64 numpy)."""
    with torch.no_grad():
        logits = forward(cast(sd, torch.float32), x_chw[None])
    return int(logits.argmax(1)[0]), F.softmax(logits.double(), dim=1)[0].numpy()


def e2e_inputs(golden_dir, kind):
    """(image u8[224,224,3], label map) of an end-to-end case: the felzenszwalb fixture on the `blobs` image, or the 16-pixel grid."""
    import os
    from network_interpretation_imagenet_amd import synth
    if kind == "felz":
        g = np.load(os.path.join(golden_dir, "felzenszwalb_skimage0183.npz"))
        return g["blobs224/image"], g["blobs224/labels"].astype(np.int64)
    return synth.make_images(1)[0], synth.grid_segments().astype(np.int64)
