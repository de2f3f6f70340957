"""CPU restatement of torchvision's ResNeXt-50 32x4d / ResNeXt-101 32x8d forward (test infrastructure only; oracle/ stays ResNet-only).

torchvision resnet.py with Bottleneck, groups = 32, width_per_group = 4 / 8, eval mode: conv1 (7x7 stride 2 pad 3) + bn1 + ReLU +
MaxPool2d(3, 2, 1); four stages of Bottlenecks with planes 64, 128, 256, 512 and inner width = planes * width_per_group / 64 * 32 --
conv1 1x1 (-> width) + BN + ReLU, conv2 3x3 pad 1 GROUPED (32 groups, stride 2 in the first block of layer2 / 3 / 4) + BN + ReLU, conv3 1x1
(-> 4 * planes) + BN, plus the identity or downsample (1x1 conv with the block's stride + BN), ReLU --; adaptive_avg_pool2d(1), fc.  Written
with torch.nn.functional (F.conv2d(groups=32)) on the state_dict, in whatever dtype the tensors have (fp64 for yardsticks), plus the
reference-style batch-1 fp32 scoring loop of oracle.scorer with this forward in place of the ResNet one.  One switch shows that grouping is
live on the rows the tests score: `dense=True` treats conv2 as a DENSE conv whose weight is the grouped one zero-extended to [width][width]
[3][3] with every off-block entry then set non-zero -- to the group's own weights, tiled over all 32 input groups: w_dense[co][g' * cg + ci] =
w[co][ci].  That dense conv equals conv2d(sum over the 32 groups of x, w) exactly, which is how it is computed.
"""
import torch
import torch.nn.functional as F

import netref
from netref import cast, e2e_inputs, masked_batch  # noqa: F401  (re-exported: the tests use them through this module)

GROUPS = 32
# arch -> (block depths, width_per_group, published parameter count)
ARCHS = {"resnext50_32x4d": ((3, 4, 6, 3), 4, 25028904), "resnext101_32x8d": ((3, 4, 23, 3), 8, 88791336)}
PLANES = (64, 128, 256, 512)
EPS = 1e-5

# The rows the end-to-end checks score: arch -> ((label map, number of mask rows, seed of synth.random_onoff), ...)
E2E_CASES = {"resnext50_32x4d": (("felz", 8, 11), ("grid", 4, 5)), "resnext101_32x8d": (("felz", 4, 11),)}


def bn(sd, prefix, x):
    return netref.bn(sd, prefix, x, EPS)


def blocks(arch):
    """(prefix "layerS.B.", cin, width, cout, stride, side of the input map, side of the output map, has a downsample branch) per block."""
    depths, wpg, _params = ARCHS[arch]
    out, cin, h = [], 64, 56
    for s, (pl, d) in enumerate(zip(PLANES, depths)):
        w = pl * wpg // 64 * GROUPS
        for b in range(d):
            stride = 2 if (b == 0 and s > 0) else 1
            out.append(("layer%d.%d." % (s + 1, b), cin, w, pl * 4, stride, h, h // stride, b == 0))
            cin, h = pl * 4, h // stride
    return out


def topology(arch):
    """The conv list in the engine's order: (name, bn name, cin, cout, ksize, stride, pad, hin, hout, relu, residual, groups)."""
    convs = [("conv1", "bn1", 3, 64, 7, 2, 3, 224, 112, 1, 0, 1)]
    for p, cin, w, cout, stride, h, ho, ds in blocks(arch):
        convs.append((p + "conv1", p + "bn1", cin, w, 1, 1, 0, h, h, 1, 0, 1))
        convs.append((p + "conv2", p + "bn2", w, w, 3, stride, 1, h, ho, 1, 0, GROUPS))
        if ds:
            convs.append((p + "downsample.0", p + "downsample.1", cin, cout, 1, stride, 0, h, ho, 0, 0, 1))
        convs.append((p + "conv3", p + "bn3", w, cout, 1, 1, 0, ho, ho, 1, 1, 1))
    convs.append(("fc", "", 2048, 1000, 1, 1, 0, 1, 1, 0, 0, 1))
    return convs


def macs(arch):
    """Multiply-accumulates of one forward, from the conv list: a grouped layer reads cin / groups channels per output channel."""
    return sum(c[8] * c[8] * c[3] * (c[2] // c[11]) * c[4] * c[4] for c in topology(arch))


def conv2(x, w, stride, dense=False):
    if dense:       # the grouped weight tiled over all 32 input groups (module docstring)
        n, c, hh, ww = x.shape
        return F.conv2d(x.reshape(n, GROUPS, c // GROUPS, hh, ww).sum(1), w, None, stride, 1)
    return F.conv2d(x, w, None, stride, 1, 1, GROUPS)


def forward(sd, x, arch, trace=None, dense=False, count=None):
    """logits [N, 1000] for the normalised NCHW batch x.  `trace` (a list) receives (name, tensor) of every block output; `count` (a
    one-element list) receives the multiply-accumulates per image, counted from the tensors each conv call actually sees."""

    def conv(x, w, stride=1, pad=0, groups=1):
        y = F.conv2d(x, w, None, stride, pad, 1, groups)
        if count is not None:
            count[0] += y.shape[1] * y.shape[2] * y.shape[3] * w.shape[1] * w.shape[2] * w.shape[3]
        return y

    x = F.relu(bn(sd, "bn1", conv(x, sd["conv1.weight"], 2, 3)))
    x = F.max_pool2d(x, 3, 2, 1)
    for p, _cin, _w, _cout, stride, _h, _ho, ds in blocks(arch):
        t = F.relu(bn(sd, p + "bn1", conv(x, sd[p + "conv1.weight"])))
        t = conv2(t, sd[p + "conv2.weight"], stride, True) if dense else conv(t, sd[p + "conv2.weight"], stride, 1, GROUPS)
        t = F.relu(bn(sd, p + "bn2", t))
        t = bn(sd, p + "bn3", conv(t, sd[p + "conv3.weight"]))
        idn = bn(sd, p + "downsample.1", conv(x, sd[p + "downsample.0.weight"], stride)) if ds else x
        x = F.relu(t + idn)
        if trace is not None:
            trace.append((p[:-1], x))
    x = torch.flatten(F.adaptive_avg_pool2d(x, 1), 1)
    if count is not None:
        count[0] += sd["fc.weight"].shape[0] * sd["fc.weight"].shape[1]
    return F.linear(x, sd["fc.weight"], sd["fc.bias"])


def bound(arch):
    """The forward of `arch` as the forward(sd, x, **switches) that netref and the test drivers take."""
    return netref.bound(forward, arch)


def score_masks_reference_loop(sd, arch, x_chw, segments, onoff, label, return_logits=False):
    """netref.score_masks_reference_loop with the ResNeXt forward of `arch`."""
    return netref.score_masks_reference_loop(bound(arch), sd, x_chw, segments, onoff, label, return_logits)


def score_masks_fp64(sd, arch, x_chw, segments, onoff, label, dense=False):
    """netref.score_masks_fp64 with the ResNeXt forward of `arch`, 4 rows at a time."""
    return netref.score_masks_fp64(bound(arch), sd, x_chw, segments, onoff, label, chunk=4, dense=dense)


def predict(sd, arch, x_chw):
    return netref.predict(bound(arch), sd, x_chw)


_E2E = {}


def e2e_rows(golden_dir, arch):
    """Per case of E2E_CASES[arch], computed once per process and shared: dict kind -> (img, seg, onoff, label, s64, logits64).  The label is
    the fp64 argmax of the unmasked picture."""
    if arch not in _E2E:
        _E2E[arch] = netref.e2e_rows(forward, E2E_CASES[arch], golden_dir, arch, chunk=4)
    return _E2E[arch]
