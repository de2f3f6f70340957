"""The draws and per-element bounds of the ConvNeXt kernels' tests, in one place: tests/test_gpu_convnext.py runs them through the kernels,
tests/test_cnext_bounds_cpu.py through a numpy fp32 emulation of the kernels' stated order (csrc/mpx_cnext.h), and the two cannot drift.

Bound, per output element: tol = C_f * 2^-22 * B + 2^-24, with B the first-order magnitude bound of the element and C_f = 4 x r_ref rounded
up to a power of two, r_ref = the worst err / B of the fp32 TORCH restatement (F.conv2d + F.layer_norm, F.gelu) against fp64 on the same
draw -- reference against reference, never the engine.  tests/test_cnext_bounds_cpu.py measures r_ref on every run and holds the recorded
C_F to the rule.
  LayerNorm of v with per-element input bound E_c (how far v_c may be off, relative to one rounding: E_c = Bv_c + mean_c' Bv_c', the element's
  own magnitude bound and its share of the mean's), d = v - mean, r = 1 / sqrt(var + eps):
      B_c = |gamma_c| r (|d_c| + E_c + |d_c| mean_c'(|d_c'| E_c') / (var + eps)) + |beta_c|
  -- the numerator's own error, and the relative error of r (half that of var, whose derivative is 2 d / C).  Bv_c = |v_c| for the
  stand-alone LayerNorm (v = hi + lo is exact: the term then covers the subtraction's rounding), sum|w||x| + |bias| over the taps inside
  the map for the depthwise conv, mean_i |x_i| for the pooled LayerNorm.
  GELU epilogue: the existing per-layer rule of tests/test_gpu_efficientnet.py (LAYER_TOL relative to max(|want|, 1), times the K factor).
Condition on the LayerNorm draws: every pixel's fp64 var >= 1e-3 (with eps = 1e-6 a pixel whose channels are nearly equal amplifies fp32
rounding a thousandfold, in the reference as well); the draws carry a per-channel offset, as a conv bias gives, which ensures it."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-6
VAR_FLOOR = 1e-3

# C, hin, batch: the depthwise 7x7 + LayerNorm shapes
DW_CASES = [
    (96, 7, 1),         # every window hangs over an edge; 12 threads per pixel: not a divisor of 64
    (96, 7, 3),
    (96, 9, 3),         # exactly one interior pixel
    (192, 14, 2),
    (768, 7, 2),        # 96 threads per pixel
    (384, 13, 1),       # odd map; the last run of a row is partial
]
# rows, C: the stand-alone LayerNorm shapes (21 pixels per workgroup at C = 96, 2 at C = 768: 1, 147, 3136 and 50 leave 1, 1, 7 and 8 behind)
LN_CASES = [(1, 96), (49 * 3, 768), (56 * 56, 96), (50, 192)]
# hw, C, batch: the pooled LayerNorm shapes
POOL_CASES = [(49, 768, 2), (1, 96, 1)]
# r_ref per shape, in units of 2^-22: the fp32 torch restatement's worst err / B against fp64 as tests/test_cnext_bounds_cpu.py measured it
# (torch 2 CPU kernels; the test measures it again on every run and holds it within a factor of two of the record, since another vector
# width sums in another order) -- and C_f = 4 r_ref rounded up to a power of two, per shape.
R_REF = {("dw", 96, 7): 0.231, ("dw", 96, 9): 0.233, ("dw", 192, 14): 0.246, ("dw", 768, 7): 0.254, ("dw", 384, 13): 0.279,
         ("ln", 1, 96): 0.104, ("ln", 147, 768): 0.245, ("ln", 3136, 96): 0.322, ("ln", 50, 192): 0.242,
         ("pool", 49, 768): 0.026, ("pool", 1, 96): 0.138}


def pow2_ceil(v):
    return 2.0 ** int(np.ceil(np.log2(max(v, 2.0 ** -20))))


C_F = {k: pow2_ceil(4 * r) for k, r in R_REF.items()}


def valid_pairs(x):
    """fp32 -> the fp32 values hi + lo of split(x): what a pair of split-fp16 planes can hold."""
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    return hi.float() + lo.float()


def planes(shape, seed, offset=0.5):
    """fp32 [..., C]: both signs, exact zeros (10 %), a band of channels (the second eighth) scaled x 8, a per-channel offset N(0, offset) as
    a conv bias leaves it; every value a valid (hi, lo) pair."""
    g = torch.Generator().manual_seed(seed)
    c = shape[-1]
    x = torch.randn(shape, generator=g) + torch.randn(c, generator=g) * offset
    x[..., c // 8: c // 4] *= 8.0
    x[torch.rand(shape, generator=g) < 0.10] = 0.0
    return valid_pairs(x)


def ln_params(c, seed):
    """LayerNorm weight with both signs and magnitudes in [0.5, 1.5], bias N(0, 0.3)."""
    g = torch.Generator().manual_seed(seed)
    gamma = torch.empty(c).uniform_(0.5, 1.5, generator=g) * torch.where(torch.rand(c, generator=g) < 0.3, -1.0, 1.0)
    gamma[0] = -abs(gamma[0])
    return gamma, torch.randn(c, generator=g) * 0.3


def dw_params(c, seed):
    """Depthwise 7x7 weights [C][7][7] N(0, 1/7) and conv bias N(0, 0.3)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(c, 7, 7, generator=g) / 7.0, torch.randn(c, generator=g) * 0.3


def ln_want(v64, bv64, gamma, beta, eps=EPS):
    """fp64 LayerNorm over the last axis of v64 and the magnitude bound B of every element.  bv64: the per-element input bound Bv."""
    g64, b64 = gamma.double(), beta.double()
    mean = v64.mean(-1, keepdim=True)
    d = v64 - mean
    var = d.pow(2).mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    e = bv64 + bv64.mean(-1, keepdim=True)
    mag = g64.abs() * r * (d.abs() + e + d.abs() * (d.abs() * e).mean(-1, keepdim=True) / (var + eps)) + b64.abs()
    return d * r * g64 + b64, mag, var


def pool_bv(x64):
    """Bv of the pooled LayerNorm's input, x64 fp64 [B][hw][C]: the serial fp32 sum and the division leave the mean within (hw + 1) 2^-24
    mean|x| (tests/shared_kernel_draws.py) = (hw + 1) / 4 roundings of 2^-22 -- and never less than the mean's own magnitude bound."""
    return x64.abs().mean(1) * max(1.0, (x64.shape[1] + 1) / 4.0)


def tol(mag, c_f):
    return c_f * 2.0 ** -22 * mag + 2.0 ** -24


def dw_v(x, w, bias, dtype):
    """v = depthwise 7x7 (pad 3) of NHWC planes x + bias, and its magnitude bound sum|w||x| + |bias|, NHWC, in `dtype`."""
    c = x.shape[-1]
    xc = x.to(dtype).permute(0, 3, 1, 2)
    v = F.conv2d(xc, w.to(dtype)[:, None], bias.to(dtype), 1, 3, 1, c).permute(0, 2, 3, 1)
    bv = F.conv2d(xc.abs(), w.to(dtype).abs()[:, None], bias.to(dtype).abs(), 1, 3, 1, c).permute(0, 2, 3, 1)
    return v, bv


def dw_ln_torch_fp32(x, w, bias, gamma, beta, eps=EPS):
    """The fp32 torch restatement of the fused launch (the yardstick's other end)."""
    v, _ = dw_v(x, w, bias, torch.float32)
    return F.layer_norm(v, (x.shape[-1],), gamma, beta, eps)


def gelu_pre_activations(n, seed):
    """fp32 [n]: pre-activations through [-6, 6] -- a uniform sweep, exact zeros, both signs, the neighbourhood of the minimum (-0.75)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.empty(n).uniform_(-6.0, 6.0, generator=g)
    v[::17] = 0.0
    v[1::29] = -0.7518
    v[2::31] = torch.randn(len(v[2::31]), generator=g) * 0.01
    return v
