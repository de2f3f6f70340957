"""Helpers of the deletion / insertion tests (csrc/mpx_rankmask.h): the seeded draws, the fp64 reference of the blur through torch's own
conv2d on the CPU, and the error bound derived from the written order of masks.blur_fill / mpx_blur_fill.

Bound.  u = 2^-24 is the unit roundoff of fp32 (round to nearest: |fl(a) - a| <= u |a|); K = klen.
  row pass   h = fl(.. fl(fl(0 + fl(t_0 v_0)) + fl(t_1 v_1)) ..): every term passes through its product's rounding and at most K sums' (the
             first, onto +0.0, is exact), so  |h - sum_k t_k v_k| <= ((1 + u)^K - 1) sum_k |t_k| |v_k| <= K u (1 + K u) A,  A = |t| * |v| along x.
  column pass  the same over the rounded h:  K u (1 + K u) sum_k |t_k| |h_k|  for its own roundings, plus what it inherits,
             sum_k |t_k| |d h_k| <= K u (1 + K u) B,  with  |h_k| <= (1 + K u (1 + K u)) A_k  and  B = |t| * A along y
             = the correlation of |v| with the outer product |t| |t|^T, zero padded.
  together   |out - exact| <= 2 K u (1 + 2 K u) B  per element; the 1 + 2 K u covers every second-order term (K u <= 31 * 2^-24 = 1.9e-6).
The fp64 reference (the exact products t_i t_j of fp32 taps, K^2 sums) is off by at most K^2 * 2^-53 * B on its own, which is added.
"""
import numpy as np
import torch
import torch.nn.functional as F

from network_interpretation_imagenet_amd import masks, synth

IMG = 224
HW = IMG * IMG
U32 = 2.0 ** -24
U64 = 2.0 ** -53
ASYM_TAPS = np.array([0.5, 0.25, 0.125], dtype=np.float32)         # no symmetry: a convolution (flipped taps) gives another answer
KLEN_CASES = (1, 3, 11, 31)


def taps_for(klen):
    """The taps of a test case: [1.0] for klen 1, the asymmetric ones for klen 3, masks.gaussian_taps(klen, 5.0) otherwise."""
    if klen == 1:
        return np.array([1.0], dtype=np.float32)
    if klen == 3:
        return ASYM_TAPS.copy()
    return masks.gaussian_taps(klen, 5.0)


def noise_chw(seed):
    """f32[3,224,224] standard normal noise: a fill image, or a picture, with negative values everywhere."""
    return np.random.default_rng(seed).standard_normal((3, IMG, IMG)).astype(np.float32)


def conv2d_64(x, taps, absolute=False):
    """f64[3,224,224]: torch.nn.functional.conv2d (a correlation) of x with the outer product of the taps, padding klen // 2, in fp64;
    absolute=True takes |x| and |taps| (the magnitude B of the bound)."""
    t = np.asarray(taps, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    if absolute:
        t, x = np.abs(t), np.abs(x)
    k2 = torch.from_numpy(np.outer(t, t))[None, None]
    return F.conv2d(torch.from_numpy(x)[:, None], k2, padding=t.size // 2)[:, 0].numpy()


def blur_bound(x, taps):
    """|masks.blur_fill(x, taps) - conv2d_64(x, taps)| per element (module docstring)."""
    k = int(np.asarray(taps).size)
    mag = conv2d_64(x, taps, absolute=True)
    return (2 * k * U32 * (1 + 2 * k * U32) + k * k * U64) * mag


def superpixel_saliency(seed=0):
    """f32[224,224], constant on each of synth.grid_segments()' 196 superpixels, with several superpixels sharing a value and two of them
    at +0.0 and -0.0: every pixel is tied with at least 255 others."""
    seg = synth.grid_segments()
    vals = np.random.default_rng(seed).integers(-6, 7, size=int(seg.max()) + 1).astype(np.float32)
    vals[3], vals[100] = 0.0, -0.0
    return np.ascontiguousarray(vals[seg])


def tied_rank_reference(sal):
    """saliency_rank spelled out: sort the (value falling, pixel index rising) pairs."""
    flat = np.asarray(sal, dtype=np.float64).ravel() + 0.0          # both zeros as +0.0
    order = np.lexsort((np.arange(flat.size), -flat))
    rank = np.empty(flat.size, dtype=np.int32)
    rank[order] = np.arange(flat.size, dtype=np.int32)
    return rank.reshape(IMG, IMG)


def split16(o):
    """The engine's hi / lo planes of fp32 values, as int16 bit patterns: hi = f16(o), lo = f16(fl(o - f32(hi))) (split_f32)."""
    o = np.asarray(o, dtype=np.float32)
    hi = o.astype(np.float16)
    lo = (o - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.int16), lo.view(np.int16)
