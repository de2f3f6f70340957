"""The draws and the bound of the grouped 3x3 kernel's tests (csrc/mpx_gconv.h, tile 16), in one place, by tests/conv_edge_draws.py's rule:
tests/test_gpu_resnext.py runs them through the kernel, tests/test_gconv_bounds_cpu.py through a numpy emulation of the kernel's
arithmetic, and the two cannot drift.  Nothing here needs a GPU: a layer is described by its torchvision topology (tests/resnext_ref.py),
and the GPU test asserts that the engine's own descriptors say the same.

Bound, per output element.  With s = gamma / sqrt(var + eps), shift = beta - mean * s and the layer's own GROUPED conv (*):
    B   = |s| (|W| * |x|)_grouped + |shift|
    tol = C 2^-22 B + 2^-24
(the terms are conv_edge_draws': the dropped lo x lo product, the weight split, the output re-split with half of lo's fp16 subnormal step
as the absolute floor, and the fp32 accumulation).  C is 4 x r_ref rounded up to a power of two, per shape, where r_ref = max err /
(2^-22 B + 2^-24) is the distance from fp64 of a numpy emulation of the kernel's arithmetic -- per channel block of max(cg, 16) channels
and per 32-wide K chunk of (ky, kx, ci), the products W_hi x_lo, W_lo x_hi, W_hi x_hi, each summed exactly and rounded to fp32 once, added
to one fp32 accumulator in that order -- measured on these draws by tests/test_gconv_bounds_cpu.py, which asserts that the constants
below follow from what it measures.  The 4 is the margin this suite gives a reference's own distance (tests/logits_lens.py) and has to
absorb the MFMA's internal order of summation.

Draws.  Image n of a layer's draw is seeded by (seed, n) alone: the same numbers at every batch size and batch index.  A draw is
randn.clamp_min(-0.5) * 1.5 (both signs), an eighth of its elements exact zeros, and within every group the channels c % cg in
[0, cg / 4) times 1e-3 (a band whose lo plane lies in fp16's subnormals) and those in [cg / 4, cg / 2) times 8.  Every value is a valid
(hi, lo) pair and the merged hi + lo planes are the truth the reference starts from."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

import resnext_ref as ref
from gpu_common import merge, split

BN_EPS = 1e-5
GROUPS = ref.GROUPS
TILE = 16
FENCE_ROWS = 256                            # pixel rows of `width` elements in front of and behind every output plane
SENTINEL_BITS = 0x7e00                      # an fp16 NaN no kernel produces

GDesc = namedtuple("GDesc", "arch name bn_name width cg stride hin hout")


def grouped_layers(arch):
    """Every grouped layer (a block's conv2) of the network, in forward order."""
    return [GDesc(arch, c[0], c[1], c[2], c[2] // GROUPS, c[5], c[7], c[8]) for c in ref.topology(arch) if c[11] > 1]


def distinct_layers(arch):
    """The first layer of every distinct (cg, stride, map)."""
    seen, out = set(), []
    for d in grouped_layers(arch):
        key = (d.cg, d.stride, d.hin)
        if key not in seen:
            seen.add(key)
            out.append(d)
    return out


def all_cases():
    return [d for arch in ref.ARCHS for d in distinct_layers(arch)]


def layer(arch, name):
    return next(d for d in grouped_layers(arch) if d.name == name)


def draw_seed(d):
    """The seed of a layer's draw in both test files: its place in its network, and which network."""
    return 1000 * list(ref.ARCHS).index(d.arch) + [g.name for g in grouped_layers(d.arch)].index(d.name) + 1


# r_ref of tests/test_gconv_bounds_cpu.py (batch 1; the 7 x 7 maps batch 3), per (arch, layer): cg, stride, map
R_REF = {
    ("resnext50_32x4d", "layer1.0.conv2"): 1.402,   # cg  4, stride 1, 56 x 56
    ("resnext50_32x4d", "layer2.0.conv2"): 1.119,   # cg  8, stride 2, 56 x 56
    ("resnext50_32x4d", "layer2.1.conv2"): 1.073,   # cg  8, stride 1, 28 x 28
    ("resnext50_32x4d", "layer3.0.conv2"): 0.914,   # cg 16, stride 2, 28 x 28
    ("resnext50_32x4d", "layer3.1.conv2"): 0.729,   # cg 16, stride 1, 14 x 14
    ("resnext50_32x4d", "layer4.0.conv2"): 0.789,   # cg 32, stride 2, 14 x 14
    ("resnext50_32x4d", "layer4.1.conv2"): 0.760,   # cg 32, stride 1, 7 x 7
    ("resnext101_32x8d", "layer1.0.conv2"): 1.268,  # cg  8, stride 1, 56 x 56
    ("resnext101_32x8d", "layer2.0.conv2"): 1.035,  # cg 16, stride 2, 56 x 56
    ("resnext101_32x8d", "layer2.1.conv2"): 1.010,  # cg 16, stride 1, 28 x 28
    ("resnext101_32x8d", "layer3.0.conv2"): 0.801,  # cg 32, stride 2, 28 x 28
    ("resnext101_32x8d", "layer3.1.conv2"): 0.626,  # cg 32, stride 1, 14 x 14
    ("resnext101_32x8d", "layer4.0.conv2"): 0.589,  # cg 64, stride 2, 14 x 14
    ("resnext101_32x8d", "layer4.1.conv2"): 0.755,  # cg 64, stride 1, 7 x 7
}
# 4 x r_ref rounded up to a power of two
C_TOL = {k: 2.0 ** math.ceil(math.log2(4 * v)) for k, v in R_REF.items()}        # 8 where r_ref > 1 (cg 4 and 8, and cg 16 on 32x8d's larger maps), else 4


def draws(d, batch, seed=None, device=None):
    """-> (x_hi, x_lo, x): the split-fp16 input planes [batch][hin][hin][width] of layer d and their merged value (fp32 holds hi + lo
    exactly)."""
    seed = draw_seed(d) if seed is None else seed
    shape = (d.hin, d.hin, d.width)
    x = torch.empty((batch,) + shape)
    g = torch.Generator()
    for n in range(batch):
        g.manual_seed(1000003 * seed + n)
        x[n] = torch.randn(shape, generator=g).clamp_min(-0.5) * 1.5
        x[n] = torch.where(torch.rand(shape, generator=g) >= 0.125, x[n], torch.zeros(()))      # exact zeros (+0 in both planes)
    pos = torch.arange(d.width) % d.cg
    band = torch.ones(d.width)
    band[pos < d.cg // 4] = 1e-3
    band[(pos >= d.cg // 4) & (pos < d.cg // 2)] = 8.0
    x *= band
    if device is not None:
        x = x.to(device)
    hi, lo = split(x)
    return hi, lo, merge(hi, lo)


def bn_affine(sd, d):
    s = sd[d.bn_name + ".weight"].double() / torch.sqrt(sd[d.bn_name + ".running_var"].double() + BN_EPS)
    return s, sd[d.bn_name + ".bias"].double() - sd[d.bn_name + ".running_mean"].double() * s


def gconv64(x, w, d):
    """The layer's own grouped conv in fp64 as one batched matrix product per tap (no conv library in between; the CPU test holds it to
    F.conv2d): x [B][hin][hin][width] (any float type), w fp64 [width][cg][3][3] -> fp64 [B][hout][hout][width].  Works on the CPU and on
    the device alike."""
    b, s, ho, cg = x.shape[0], d.stride, d.hout, d.cg
    xc = F.pad(x.double(), (0, 0, 1, 1, 1, 1))
    wg = w.view(GROUPS, cg, cg, 3, 3)                   # [group][out][in][ky][kx]
    acc = None
    for ky in range(3):
        for kx in range(3):
            tap = xc[:, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (ho - 1) + 1:s, :].reshape(-1, GROUPS, cg).transpose(0, 1)
            y = torch.bmm(tap, wg[:, :, :, ky, kx].transpose(1, 2))
            acc = y if acc is None else acc + y
    return acc.transpose(0, 1).reshape(b, ho, ho, d.width)


def reference(sd, d, x, w=None, shift=None):
    """-> (pre, want, B): the fp64 pre-activation s gconv(x) + shift, want = ReLU(pre), and the per-element B of the module docstring.
    w / shift: replacements for the layer's weight [width][cg][3][3] and shift [width] (the group-isolation cases)."""
    w = (sd[d.name + ".weight"] if w is None else w).double().to(x.device)
    s, sh = (t.to(x.device) for t in bn_affine(sd, d))
    if shift is not None:
        sh = shift.double().to(x.device)
    pre = gconv64(x, w, d) * s + sh
    b = gconv64(x.abs(), w.abs(), d) * s.abs() + sh.abs()
    return pre, torch.relu(pre), b


def tol(d, b):
    return C_TOL[(d.arch, d.name)] * 2.0 ** -22 * b + 2.0 ** -24


def preconditions(want):
    """conv_edge_draws.preconditions: no hi plane can overflow fp16, and at least 5 % of the elements are small next to the largest one."""
    top = want.abs().max().item()
    small = (want.abs() < 1e-2 * top).double().mean().item()
    assert top < 3e4, "max |want| = %g: a hi plane could overflow" % top
    assert small >= 0.05, "only %.1f %% of the elements are under 1 %% of the largest" % (100 * small)
    return top, small
