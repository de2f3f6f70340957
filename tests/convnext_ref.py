"""CPU restatement of torchvision's ConvNeXt-Tiny / -Small forward (test infrastructure only; oracle/ stays ResNet-only).

torchvision convnext.py in eval mode: features.0 = Conv2d(3, 96, 4, stride 4, bias) + LayerNorm2d(96); four stages features.1 / .3 / .5 / .7 of
DEPTHS[arch] CNBlocks of width 96, 192, 384, 768 on 56 / 28 / 14 / 7 maps; features.2 / .4 / .6 = LayerNorm2d(C_prev) + Conv2d(C_prev, C, 2,
stride 2, bias); adaptive_avg_pool2d(1), classifier.0 = LayerNorm2d(768), flatten, classifier.2 = Linear(768, 1000).  A CNBlock is block.0 =
Conv2d(C, C, 7, pad 3, groups C, bias), a permute to NHWC, block.2 = LayerNorm(C), block.3 = Linear(C, 4C), GELU (exact, erf form), block.5 =
Linear(4C, C), the permute back, and output = input + layer_scale * block(input); StochasticDepth is the identity in eval.  Every LayerNorm
has eps 1e-6.  Written with torch.nn.functional on the state_dict, in whatever dtype the tensors have (fp64 for yardsticks), plus the
reference-style batch-1 fp32 scoring loop of oracle.scorer with this forward in place of the ResNet one.  Three switches show that the new
arithmetic is live on the rows the tests score: `layer_scale=1e-6` (any float) replaces every layer scale by that constant, `gelu=False`
replaces every GELU by ReLU, `ln_map=True` takes each block LayerNorm's statistics over the whole map instead of per pixel.
"""
import torch
import torch.nn.functional as F

import netref
from netref import cast, e2e_inputs, masked_batch  # noqa: F401  (re-exported: the tests use them through this module)

ARCHS = ("convnext_tiny", "convnext_small")
DEPTHS = {"convnext_tiny": (3, 3, 9, 3), "convnext_small": (3, 3, 27, 3)}
DIMS = (96, 192, 384, 768)
EPS = 1e-6
PARAMS = {"convnext_tiny": 28589128, "convnext_small": 50223688}
MACS = {"convnext_tiny": 4455531264, "convnext_small": 8683712256}

# The rows the end-to-end checks score: (label map, number of mask rows, seed of synth.random_onoff)
E2E_CASES = (("felz", 3, 11), ("grid", 2, 5))


def arch_of(sd):
    return "convnext_small" if "features.5.26.layer_scale" in sd else "convnext_tiny"


def topology(arch):
    """The network's layers in forward order.  convs: (name, bn name, cin, cout, ksize, stride, hin, hout, residual, epilogue act) of the
    stem, every block.3 / block.5, the three downsample convs and classifier.2 -- relu is 0 and pad is 0 everywhere, block.5's bn name is the
    block's layer_scale; depthwise: (name, LayerNorm name, channels, hin); lnorms: (name, channels, side of the map; 1 for classifier.0)."""
    convs = [("features.0.0", "", 3, 96, 4, 4, 224, 56, 0, 0)]
    lnorms = [("features.0.1", 96, 56)]
    dws = []
    h = 56
    for s, (c, d) in enumerate(zip(DIMS, DEPTHS[arch])):
        if s:
            lnorms.append(("features.%d.0" % (2 * s), DIMS[s - 1], h))
            convs.append(("features.%d.1" % (2 * s), "", DIMS[s - 1], c, 2, 2, h, h // 2, 0, 0))
            h //= 2
        for b in range(d):
            p = "features.%d.%d." % (2 * s + 1, b)
            dws.append((p + "block.0", p + "block.2", c, h))
            convs.append((p + "block.3", "", c, 4 * c, 1, 1, h, h, 0, 1))
            convs.append((p + "block.5", p + "layer_scale", 4 * c, c, 1, 1, h, h, 1, 0))
    lnorms.append(("classifier.0", 768, 1))
    convs.append(("classifier.2", "", 768, 1000, 1, 1, 1, 1, 0, 0))
    return convs, dws, lnorms


def macs(arch):
    """Multiply-accumulates of one forward: the convs and Linears (as 1x1 convs) and the depthwise convs; LayerNorm, GELU and the layer
    scale are not MACs."""
    convs, dws, _ln = topology(arch)
    return sum(c[7] * c[7] * c[3] * c[2] * c[4] * c[4] for c in convs) + sum(h * h * c * 49 for _n, _l, c, h in dws)


def ln2d(sd, prefix, x):
    """LayerNorm2d: the LayerNorm over the channels of each pixel of an NCHW map."""
    return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), sd[prefix + ".weight"], sd[prefix + ".bias"], EPS).permute(0, 3, 1, 2)


def features(sd, x, trace=None, layer_scale=None, gelu=True, ln_map=False):
    """The trunk up to the last block's output; `trace` (a list) receives (name, tensor): the stem's LayerNorm output, per block the
    depthwise + LayerNorm map ("<block>.ln", NHWC), the GELU pre-activation ("<block>.pre", NHWC) and the block output, and every downsample
    output."""
    def note(name, t):
        if trace is not None:
            trace.append((name, t))
        return t

    arch = arch_of(sd)
    x = note("features.0", ln2d(sd, "features.0.1", F.conv2d(x, sd["features.0.0.weight"], sd["features.0.0.bias"], 4)))
    for s, (c, d) in enumerate(zip(DIMS, DEPTHS[arch])):
        if s:
            p = "features.%d." % (2 * s)
            x = note(p[:-1], F.conv2d(ln2d(sd, p + "0", x), sd[p + "1.weight"], sd[p + "1.bias"], 2))
        for b in range(d):
            p = "features.%d.%d." % (2 * s + 1, b)
            t = F.conv2d(x, sd[p + "block.0.weight"], sd[p + "block.0.bias"], 1, 3, 1, c).permute(0, 2, 3, 1)
            if ln_map:      # the wrong reduction: statistics over the whole map of an image instead of per pixel
                mu = t.mean((1, 2, 3), keepdim=True)
                var = (t - mu).pow(2).mean((1, 2, 3), keepdim=True)
                t = (t - mu) / torch.sqrt(var + EPS) * sd[p + "block.2.weight"] + sd[p + "block.2.bias"]
            else:
                t = F.layer_norm(t, (c,), sd[p + "block.2.weight"], sd[p + "block.2.bias"], EPS)
            note(p + "ln", t)
            t = note(p + "pre", F.linear(t, sd[p + "block.3.weight"], sd[p + "block.3.bias"]))
            t = F.gelu(t) if gelu else F.relu(t)
            t = F.linear(t, sd[p + "block.5.weight"], sd[p + "block.5.bias"]).permute(0, 3, 1, 2)
            ls = sd[p + "layer_scale"] if layer_scale is None else torch.full_like(sd[p + "layer_scale"], float(layer_scale))
            x = note(p[:-1], x + ls * t)
    return x


def forward(sd, x, trace=None, layer_scale=None, gelu=True, ln_map=False):
    """logits [N, 1000] of torchvision's convnext_tiny / convnext_small for the normalised NCHW batch x."""
    x = features(sd, x, trace, layer_scale, gelu, ln_map)
    x = torch.flatten(ln2d(sd, "classifier.0", F.adaptive_avg_pool2d(x, 1)), 1)
    return F.linear(x, sd["classifier.2.weight"], sd["classifier.2.bias"])


def score_masks_reference_loop(sd, x_chw, segments, onoff, label, return_logits=False):
    """netref.score_masks_reference_loop with the ConvNeXt forward."""
    return netref.score_masks_reference_loop(forward, sd, x_chw, segments, onoff, label, return_logits)


def score_masks_fp64(sd, x_chw, segments, onoff, label, **switches):
    """netref.score_masks_fp64 with the ConvNeXt forward, 5 rows at a time."""
    return netref.score_masks_fp64(forward, sd, x_chw, segments, onoff, label, chunk=5, **switches)
