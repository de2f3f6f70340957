"""The draws and the bound of the any-width grouped 3x3 kernel's tests (csrc/mpx_gconvw.h, tile 18), in one place, by tests/gconv_draws.py's
rule: tests/test_gpu_regnet.py runs them through the kernel, tests/test_regnet_bounds_cpu.py through a numpy emulation of the kernel's
arithmetic, and the two cannot drift.  Nothing here needs a GPU: a layer is described by its torchvision topology (tests/regnet_ref.py), and
the GPU test asserts that the engine's own descriptors say the same.

Bound, per output element.  With s = gamma / sqrt(var + eps), shift = beta - mean * s and the layer's own GROUPED conv (*):
    B   = |s| (|W| * |x|)_grouped + |shift|
    tol = C 2^-22 B + 2^-24
(gconv_draws' terms).  C is 4 x r_ref rounded up to a power of two, per shape, where r_ref = max err / (2^-22 B + 2^-24) is the distance from
fp64 of a numpy emulation of the kernel's arithmetic -- per group and per 32-wide chunk of the flattened K = (ky, kx, ci) index, the products
W_hi x_lo, W_lo x_hi, W_hi x_hi, each summed exactly and rounded to fp32 once, added to one fp32 accumulator in that order -- measured on
these draws by tests/test_regnet_bounds_cpu.py, which re-measures r_ref on every run and holds it within a factor of two of the record below.

Draws.  gconv_draws': image n of a layer's draw is seeded by (seed, n) alone; randn.clamp_min(-0.5) * 1.5 (both signs), an eighth of its
elements exact zeros, and within every group the channels c % cg in [0, cg / 4) times 1e-3 and those in [cg / 4, cg / 2) times 8."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

import regnet_ref as ref
from gpu_common import merge, split

BN_EPS = 1e-5
TILE = 18
FENCE_ROWS = 256                            # pixel rows of `pitch` elements in front of and behind every output plane
SENTINEL_BITS = 0x7e00                      # an fp16 NaN no kernel produces

GDesc = namedtuple("GDesc", "arch name bn_name width cg groups stride hin hout")


def grouped_layers(arch):
    """Every grouped layer (a block's f.b with more than one group) of the network, in forward order."""
    return [GDesc(arch, c[0], c[1], c[2], c[2] // c[11], c[11], c[5], c[7], c[8]) for c in ref.topology(arch) if c[11] > 1]


def distinct_layers(arch):
    """The first layer of every distinct (cg, groups, stride, map)."""
    seen, out = set(), []
    for d in grouped_layers(arch):
        key = (d.cg, d.groups, d.stride, d.hin)
        if key not in seen:
            seen.add(key)
            out.append(d)
    return out


def all_cases():
    return [d for arch in ref.ARCHS for d in distinct_layers(arch)]


def batches(d):
    """Batch 1; the 14 x 14 and 7 x 7 output maps also at batch 3 (M = 196 / 49 / 147 is no multiple of 16: a 16-pixel tile crosses rows and images)."""
    return (1, 3) if d.hout <= 14 else (1,)


def layer(arch, name):
    return next(d for d in grouped_layers(arch) if d.name == name)


def draw_seed(d):
    """The seed of a layer's draw in both test files: its place in its network, and which network."""
    return 1000 * list(ref.ARCHS).index(d.arch) + [g.name for g in grouped_layers(d.arch)].index(d.name) + 1


# r_ref of tests/test_regnet_bounds_cpu.py at the largest batch of batches(d), per (arch, layer): cg, groups, stride, input map
R_REF = {
    ("regnet_x_400mf", "trunk_output.block1.block1-0.f.b.0"): 0.978,   # cg  16, groups  2, stride 2, 112 x 112
    ("regnet_x_400mf", "trunk_output.block2.block2-0.f.b.0"): 0.745,   # cg  16, groups  4, stride 2,  56 x 56
    ("regnet_x_400mf", "trunk_output.block2.block2-1.f.b.0"): 0.724,   # cg  16, groups  4, stride 1,  28 x 28
    ("regnet_x_400mf", "trunk_output.block3.block3-0.f.b.0"): 0.808,   # cg  16, groups 10, stride 2,  28 x 28
    ("regnet_x_400mf", "trunk_output.block3.block3-1.f.b.0"): 0.812,   # cg  16, groups 10, stride 1,  14 x 14
    ("regnet_x_400mf", "trunk_output.block4.block4-0.f.b.0"): 0.739,   # cg  16, groups 25, stride 2,  14 x 14
    ("regnet_x_400mf", "trunk_output.block4.block4-1.f.b.0"): 0.837,   # cg  16, groups 25, stride 1,   7 x 7
    ("regnet_x_800mf", "trunk_output.block1.block1-0.f.b.0"): 1.030,   # cg  16, groups  4, stride 2, 112 x 112
    ("regnet_x_800mf", "trunk_output.block2.block2-0.f.b.0"): 0.862,   # cg  16, groups  8, stride 2,  56 x 56
    ("regnet_x_800mf", "trunk_output.block2.block2-1.f.b.0"): 0.727,   # cg  16, groups  8, stride 1,  28 x 28
    ("regnet_x_800mf", "trunk_output.block3.block3-0.f.b.0"): 0.927,   # cg  16, groups 18, stride 2,  28 x 28
    ("regnet_x_800mf", "trunk_output.block3.block3-1.f.b.0"): 0.950,   # cg  16, groups 18, stride 1,  14 x 14
    ("regnet_x_800mf", "trunk_output.block4.block4-0.f.b.0"): 0.924,   # cg  16, groups 42, stride 2,  14 x 14
    ("regnet_x_800mf", "trunk_output.block4.block4-1.f.b.0"): 1.204,   # cg  16, groups 42, stride 1,   7 x 7
    ("regnet_x_1_6gf", "trunk_output.block1.block1-0.f.b.0"): 0.853,   # cg  24, groups  3, stride 2, 112 x 112
    ("regnet_x_1_6gf", "trunk_output.block1.block1-1.f.b.0"): 0.792,   # cg  24, groups  3, stride 1,  56 x 56
    ("regnet_x_1_6gf", "trunk_output.block2.block2-0.f.b.0"): 0.931,   # cg  24, groups  7, stride 2,  56 x 56
    ("regnet_x_1_6gf", "trunk_output.block2.block2-1.f.b.0"): 0.794,   # cg  24, groups  7, stride 1,  28 x 28
    ("regnet_x_1_6gf", "trunk_output.block3.block3-0.f.b.0"): 0.824,   # cg  24, groups 17, stride 2,  28 x 28
    ("regnet_x_1_6gf", "trunk_output.block3.block3-1.f.b.0"): 0.832,   # cg  24, groups 17, stride 1,  14 x 14
    ("regnet_x_1_6gf", "trunk_output.block4.block4-0.f.b.0"): 0.828,   # cg  24, groups 38, stride 2,  14 x 14
    ("regnet_x_1_6gf", "trunk_output.block4.block4-1.f.b.0"): 0.827,   # cg  24, groups 38, stride 1,   7 x 7
    ("regnet_x_3_2gf", "trunk_output.block1.block1-0.f.b.0"): 0.684,   # cg  48, groups  2, stride 2, 112 x 112
    ("regnet_x_3_2gf", "trunk_output.block1.block1-1.f.b.0"): 0.668,   # cg  48, groups  2, stride 1,  56 x 56
    ("regnet_x_3_2gf", "trunk_output.block2.block2-0.f.b.0"): 0.766,   # cg  48, groups  4, stride 2,  56 x 56
    ("regnet_x_3_2gf", "trunk_output.block2.block2-1.f.b.0"): 0.715,   # cg  48, groups  4, stride 1,  28 x 28
    ("regnet_x_3_2gf", "trunk_output.block3.block3-0.f.b.0"): 0.852,   # cg  48, groups  9, stride 2,  28 x 28
    ("regnet_x_3_2gf", "trunk_output.block3.block3-1.f.b.0"): 0.655,   # cg  48, groups  9, stride 1,  14 x 14
    ("regnet_x_3_2gf", "trunk_output.block4.block4-0.f.b.0"): 0.718,   # cg  48, groups 21, stride 2,  14 x 14
    ("regnet_x_3_2gf", "trunk_output.block4.block4-1.f.b.0"): 0.662,   # cg  48, groups 21, stride 1,   7 x 7
    ("regnet_x_8gf", "trunk_output.block2.block2-0.f.b.0"): 0.518,   # cg 120, groups  2, stride 2,  56 x 56
    ("regnet_x_8gf", "trunk_output.block2.block2-1.f.b.0"): 0.639,   # cg 120, groups  2, stride 1,  28 x 28
    ("regnet_x_8gf", "trunk_output.block3.block3-0.f.b.0"): 0.757,   # cg 120, groups  6, stride 2,  28 x 28
    ("regnet_x_8gf", "trunk_output.block3.block3-1.f.b.0"): 0.799,   # cg 120, groups  6, stride 1,  14 x 14
    ("regnet_x_8gf", "trunk_output.block4.block4-0.f.b.0"): 0.757,   # cg 120, groups 16, stride 2,  14 x 14
}
# 4 x r_ref rounded up to a power of two
C_TOL = {k: 2.0 ** math.ceil(math.log2(4 * v)) for k, v in R_REF.items()}


def draws(d, batch, seed=None, device=None):
    """-> (x_hi, x_lo, x): the split-fp16 input [batch][hin][hin][width] of layer d (dense: the GPU test places it into planes at the layer's
    pitch) and its merged value (fp32 holds hi + lo exactly)."""
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
    F.conv2d(groups=...)): x [B][hin][hin][width] (any float type), w fp64 [width][cg][3][3] -> fp64 [B][hout][hout][width]."""
    b, s, ho, cg, G = x.shape[0], d.stride, d.hout, d.cg, d.groups
    xc = F.pad(x.double(), (0, 0, 1, 1, 1, 1))
    wg = w.view(G, cg, cg, 3, 3)                        # [group][out][in][ky][kx]
    acc = None
    for ky in range(3):
        for kx in range(3):
            tap = xc[:, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (ho - 1) + 1:s, :].reshape(-1, G, cg).transpose(0, 1)
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
