"""The draws, the numpy emulation and the per-element bounds of the ViT kernels' tests (csrc/mpx_attn.h), in one place: tests/test_gpu_vit.py runs
the draws through the kernels, tests/test_attn_bounds_cpu.py through the emulation of the kernels' written contract, and the two cannot drift.

Bound, per output element, in the form DESIGN.md 22 uses: tol = C_f * 2^-22 * B + 2^-24, with B the first-order magnitude term of the element.
The constant is measured, not chosen: r_ref = the worst (err - 2^-24)+ / B of the EMULATION of the contract against fp64 on the same draw, in
units of 2^-22 -- the coefficient the magnitude term needs next to the absolute term, which is the floor of a split-fp16 pair --, and C_f = 4 x r_ref rounded up to a power of two (four is the factor every bound here uses).  tests/test_attn_bounds_cpu.py measures
r_ref on every run and holds it within a factor of two of the record below (DESIGN.md 23 has the same table).
  Attention, output channel d of query row i:  B_id = (sum_j p_ij |v_jd|) * (1 + S_i),  p = the fp64 softmax weights,
      S_i = max_j 0.125 * sum_c |q_ic| |k_jc|
  -- the sum's own roundings and those of the weights (expf, the split, the division) are relative to sum_j p_ij |v_jd|; an error of the
  logits, which is relative to their magnitude sum S_i, moves every weight by p_ij (ds_ij - sum_j' p_ij' ds_ij'), i.e. the output by at most 2
  S_i times the same sum.
  Token assembly:  B = |x| + |pos| (one fp32 add of exact operands, then the re-split).
  The LayerNorm of strided rows reuses DESIGN.md 22's bound (tests/cnext_draws.ln_want) unchanged."""
import numpy as np
import torch

F32 = np.float32
HD = 64

# T, heads, B: the attention shapes -- T = 1 (one key: the softmax is 1), 15 / 16 / 17 around the 16-row query block and key tile, 50 (vit_b_32:
# the second tile of the last 32-key step is partly masked), 197 (vit_b_16: 13 tiles, the last step's second tile is all padding); heads 1, 2
# (every T) and 12 (the networks' own, at their own T); B = 1 and 3
ATTN_CASES = [(1, 2, 1), (15, 2, 3), (16, 2, 1), (17, 2, 3), (17, 1, 1), (50, 2, 3), (197, 2, 1), (50, 12, 3), (197, 12, 1)]
# B, T, D: the token assembly shapes
TOK_CASES = [(1, 1, 8), (3, 5, 64), (3, 50, 768), (1, 197, 768)]
# r_ref per shape in units of 2^-22 as tests/test_attn_bounds_cpu.py measured it, and C_f = 4 r_ref rounded up to a power of two
R_REF = {("attn", 1, 2): 0.0, ("attn", 15, 2): 0.525, ("attn", 16, 2): 0.284, ("attn", 17, 2): 0.290, ("attn", 17, 1): 0.307, ("attn", 50, 2): 0.433,
         ("attn", 197, 2): 0.745, ("attn", 50, 12): 0.579, ("attn", 197, 12): 0.929,
         ("tok", 1, 1, 8): 0.228, ("tok", 3, 5, 64): 0.658, ("tok", 3, 50, 768): 0.698, ("tok", 1, 197, 768): 0.713}


def pow2_ceil(v):
    return 2.0 ** int(np.ceil(np.log2(max(v, 2.0 ** -20))))


C_F = {k: pow2_ceil(4 * r) for k, r in R_REF.items()}


def tol(mag, c_f):
    return c_f * 2.0 ** -22 * mag + 2.0 ** -24


def split(x):
    """fp32 ndarray -> (hi, lo) fp16 ndarrays of split_f32."""
    x = np.asarray(x, dtype=F32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(F32)).astype(np.float16)
    return hi, lo


def valid_pairs(x):
    hi, lo = split(x)
    return hi.astype(F32) + lo.astype(F32)


def qkv_planes(b, t, heads, seed):
    """fp32 ndarray [B][T][3 D] as in_proj writes it (Q at 0, K at D, V at 2 D), every value a valid (hi, lo) pair: N(0, 1) with both signs, 10 %
    exact zeros, a band of query rows (every fifth token) x 8 -- logits of standard deviation 8: rows near one-hot -- and another (every fifth
    + 1) x 1 / 8 -- rows near uniform --, and a per-channel offset N(0, 0.5) on V as a bias leaves it."""
    g = torch.Generator().manual_seed(seed)
    d = heads * HD
    x = torch.randn(b, t, 3 * d, generator=g)
    x[:, 0::5, :d] *= 8.0
    x[:, 1::5, :d] *= 0.125
    x[..., 2 * d:] += torch.randn(d, generator=g) * 0.5
    x[torch.rand(b, t, 3 * d, generator=g) < 0.10] = 0.0
    return valid_pairs(x.numpy())


def heads_of(x, heads):
    """[B][T][3 D] -> q, k, v each [B][heads][T][64]."""
    b, t, _ = x.shape
    d = heads * HD
    return tuple(x[..., i * d:(i + 1) * d].reshape(b, t, heads, HD).transpose(0, 2, 1, 3) for i in range(3))


def merge(o):
    """[B][heads][T][64] -> [B][T][D]."""
    b, h, t, _ = o.shape
    return o.transpose(0, 2, 1, 3).reshape(b, t, h * HD)


def attn_want(x, heads):
    """fp64 softmax(q k^T / 8) v of the planes x and the magnitude term B of every output element, both [B][T][D]."""
    q, k, v = (z.astype(np.float64) for z in heads_of(x, heads))
    s = 0.125 * (q @ k.transpose(0, 1, 3, 2))
    e = np.exp(s - s.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    big = (0.125 * (np.abs(q) @ np.abs(k).transpose(0, 1, 3, 2))).max(-1, keepdims=True)
    return merge(p @ v), merge((p @ np.abs(v)) * (1.0 + big))


def _mfma3(acc, a, b):
    """One 32-wide step of the three products into an fp32 accumulator: a, b = (hi, lo) pairs of fp16 arrays [..., M, 32] and [..., N, 32].  A
    product of two fp16 values and a sum of 32 of them are exact in fp64; each MFMA rounds its sum into the accumulator once."""
    (ah, al), (bh, bl) = a, b
    for x, y in ((ah, bl), (al, bh), (ah, bh)):
        acc = (acc.astype(np.float64) + x.astype(np.float64) @ np.swapaxes(y.astype(np.float64), -1, -2)).astype(F32)
    return acc


def emulate_attention(x, heads):
    """The contract of csrc/mpx_attn.h in numpy fp32, on planes x f32[B][T][3 D] of valid pairs: returns hi + lo of the output, [B][T][D]."""
    q, k, v = heads_of(x, heads)
    b, h, t, _ = q.shape
    tp = (t + 31) // 32 * 32
    (qh, ql), (kh, kl), (vh, vl) = split(q), split(k), split(v)
    acc = np.zeros((b, h, t, t), dtype=F32)                         # [query][key]: the kernel's K as the A operand, Q as B, transposed here
    for c0 in (0, 32):
        acc = _mfma3(acc.swapaxes(-1, -2), (kh[..., c0:c0 + 32], kl[..., c0:c0 + 32]), (qh[..., c0:c0 + 32], ql[..., c0:c0 + 32])).swapaxes(-1, -2)
    s = (F32(0.125) * acc).astype(F32)
    m = s.max(-1, keepdims=True)
    e = np.exp((s - m).astype(F32)).astype(F32)
    e = np.concatenate([e, np.zeros((b, h, t, tp - t), dtype=F32)], -1)          # keys >= T: the constant 0.f
    part = np.zeros((b, h, t, 4), dtype=F32)
    for j in range(tp):
        g = (j >> 2) & 3
        part[..., g] = (part[..., g] + e[..., j]).astype(F32)
    l = (((part[..., 0] + part[..., 1]).astype(F32) + part[..., 2]).astype(F32) + part[..., 3]).astype(F32)
    ph, pl = split((F32(1024.0) * e).astype(F32))
    pad = np.zeros((b, h, tp - t, HD), dtype=np.float16)
    vh, vl = np.concatenate([vh, pad], 2), np.concatenate([vl, pad], 2)
    o = np.zeros((b, h, HD, t), dtype=F32)                          # [channel][query]: V^T as the A operand, P as B
    for j0 in range(0, tp, 32):
        o = _mfma3(o, (vh[..., j0:j0 + 32, :].swapaxes(-1, -2), vl[..., j0:j0 + 32, :].swapaxes(-1, -2)), (ph[..., j0:j0 + 32], pl[..., j0:j0 + 32]))
    o = (o.swapaxes(-1, -2) / (F32(1024.0) * l).astype(F32)[..., None]).astype(F32)
    return valid_pairs(merge(o))


def tok_draw(b, t, d, seed):
    """(patch planes f32[B][T - 1][D] of valid pairs, class_token f32[D], pos f32[T][D]): both signs, exact zeros, magnitudes over three decades."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, max(t - 1, 0), d, generator=g) * 10.0 ** torch.randint(-1, 2, (b, max(t - 1, 0), d), generator=g).float()
    x[torch.rand(x.shape, generator=g) < 0.10] = 0.0
    cls = torch.randn(d, generator=g)
    pos = torch.randn(t, d, generator=g) * 0.5
    pos[torch.rand(t, d, generator=g) < 0.05] = 0.0
    return valid_pairs(x.numpy()), cls.numpy(), pos.numpy()


def tok_want(x, cls, pos):
    """fp64 tokens [B][T][D] and their magnitude term |x| + |pos|."""
    b = x.shape[0]
    rows = np.concatenate([np.broadcast_to(cls.astype(np.float64), (b, 1, cls.shape[0])), x.astype(np.float64)], 1)
    return rows + pos.astype(np.float64), np.abs(rows) + np.abs(pos.astype(np.float64))


def emulate_tokens(x, cls, pos):
    b = x.shape[0]
    rows = np.concatenate([np.broadcast_to(cls, (b, 1, cls.shape[0])), x], 1).astype(F32)
    return valid_pairs((rows + pos).astype(F32))
