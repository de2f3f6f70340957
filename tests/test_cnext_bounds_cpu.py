"""The per-element bounds of tests/test_gpu_convnext.py speak for the kernels only if the arithmetic they describe stays inside them: a
numpy fp32 emulation of the stated order of csrc/mpx_cnext.h (fma chain over the taps inside the map, row-major; the 8 channels of a group
ascending, then the groups ascending; centred two-pass variance; 1 / sqrt; ((d * r) * gamma) + beta; the re-split) and of the GELU epilogue,
run on the very draws the GPU tests use (tests/cnext_draws.py), against fp64.  The same run measures r_ref -- the fp32 torch restatement's own
worst err / B -- and holds the recorded C_F to the rule C_f = 4 r_ref rounded up to a power of two.  No GPU.
Measured here (r_ref / worst emulation err / bound at the recorded C_f), printed on every run: see DESIGN.md 22."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnext_draws as draws

F32 = np.float32


def _split_merge(v):
    hi = v.astype(np.float16)
    lo = (v - hi.astype(F32)).astype(np.float16)
    return hi.astype(F32) + lo.astype(F32)


def _fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in fp64; one fp64 add, then the rounding to fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def emulate_ln(v, gamma, beta, eps):
    """The kernels' LayerNorm of v f32[..., C] (C % 8 == 0), in their order."""
    c = v.shape[-1]
    g8 = v.reshape(v.shape[:-1] + (c // 8, 8))
    part = g8[..., 0]
    for j in range(1, 8):
        part = (part + g8[..., j]).astype(F32)
    s = part[..., 0]
    for g in range(1, c // 8):
        s = (s + part[..., g]).astype(F32)
    mean = (s / F32(c)).astype(F32)
    d = (g8 - mean[..., None, None]).astype(F32)
    sq = (d[..., 0] * d[..., 0]).astype(F32)
    for j in range(1, 8):
        sq = (sq + (d[..., j] * d[..., j]).astype(F32)).astype(F32)
    s = sq[..., 0]
    for g in range(1, c // 8):
        s = (s + sq[..., g]).astype(F32)
    var = (s / F32(c)).astype(F32)
    r = (F32(1.0) / np.sqrt((var + F32(eps)).astype(F32))).astype(F32)
    d = d.reshape(v.shape)
    y = ((((d * r[..., None]).astype(F32)) * gamma).astype(F32) + beta).astype(F32)
    return _split_merge(y)


def emulate_dw(x, w, bias):
    """v = fma chain over the 49 taps inside the map, row-major, from 0, then + bias: x f32[B][H][H][C], w f32[C][7][7]."""
    b, h, _, c = x.shape
    acc = np.zeros_like(x)
    for ky in range(7):
        for kx in range(7):
            dy, dx = ky - 3, kx - 3
            y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(h, h - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            acc[:, y0:y1, x0:x1] = _fma(np.broadcast_to(w[:, ky, kx], acc[:, y0:y1, x0:x1].shape), x[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx], acc[:, y0:y1, x0:x1])
    return (acc + bias).astype(F32)


def _report(kind, key, got, ref32, want, mag, var):
    assert var.min().item() >= draws.VAR_FLOOR, (kind, key, var.min().item())
    r_ref = ((ref32.double() - want).abs() / mag).max().item() / 2.0 ** -22
    c_f = draws.C_F[(kind,) + key]
    worst = ((got.double() - want).abs() / draws.tol(mag, c_f)).max().item()
    print("%s %s: min var %.3g, r_ref %.3f x 2^-22 -> C_f %g (recorded %g), emulation worst err / bound %.3f"
          % (kind, key, var.min().item(), r_ref, draws.pow2_ceil(4 * r_ref), c_f, worst))
    rec = draws.R_REF[(kind,) + key]
    assert c_f == draws.pow2_ceil(4 * rec) and 0.5 * rec <= r_ref <= 2.0 * rec, (kind, key, r_ref, rec, c_f)
    assert worst <= 1.0, (kind, key, worst)


@pytest.mark.parametrize("c,hin,batch", [t for t in draws.DW_CASES if t[2] != 1 or t[1] != 7])
def test_dwconv7x7_ln_order_stays_inside_its_bound(c, hin, batch):
    x = draws.planes((batch, hin, hin, c), seed=100 * c + hin)
    w, bias = draws.dw_params(c, seed=c + hin)
    gamma, beta = draws.ln_params(c, seed=7 * c + hin)
    v64, bv64 = draws.dw_v(x, w, bias, torch.float64)
    want, mag, var = draws.ln_want(v64, bv64, gamma, beta)
    got = torch.from_numpy(emulate_ln(emulate_dw(x.numpy(), w.numpy(), bias.numpy()), gamma.numpy(), beta.numpy(), draws.EPS))
    _report("dw", (c, hin), got, draws.dw_ln_torch_fp32(x, w, bias, gamma, beta), want, mag, var)
    assert (x == 0).any() and (x > 0).any() and (x < 0).any() and (gamma < 0).any()
    band = x[..., c // 8: c // 4].abs().mean().item()
    assert band > 3 * x[..., c // 4:].abs().mean().item()            # the x 8 band is there


@pytest.mark.parametrize("rows,c", draws.LN_CASES)
def test_layernorm_c_order_stays_inside_its_bound(rows, c):
    x = draws.planes((rows, c), seed=10 * rows + c)
    gamma, beta = draws.ln_params(c, seed=rows + c)
    want, mag, var = draws.ln_want(x.double(), x.double().abs(), gamma, beta)
    got = torch.from_numpy(emulate_ln(x.numpy(), gamma.numpy(), beta.numpy(), draws.EPS))
    _report("ln", (rows, c), got, F.layer_norm(x, (c,), gamma, beta, draws.EPS), want, mag, var)


@pytest.mark.parametrize("hw,c,batch", draws.POOL_CASES)
def test_global_avgpool_ln_order_stays_inside_its_bound(hw, c, batch):
    x = draws.planes((batch, hw, c), seed=hw + c)
    gamma, beta = draws.ln_params(c, seed=3 * hw + c)
    want, mag, var = draws.ln_want(x.double().mean(1), draws.pool_bv(x.double()), gamma, beta)
    s = np.zeros((batch, c), dtype=F32)
    for i in range(hw):
        s = (s + x.numpy()[:, i, :]).astype(F32)
    got = torch.from_numpy(emulate_ln((s / F32(hw)).astype(F32), gamma.numpy(), beta.numpy(), draws.EPS))
    _report("pool", (hw, c), got, F.layer_norm(x.mean(1), (c,), gamma, beta, draws.EPS), want, mag, var)


def test_gelu_epilogue_form_against_fp64():
    """gelu(v) = 0.5f v (1.0f + erff(v 0.70710678118654752f)) in fp32 on pre-activations through [-6, 6], against the fp64 erf form: the
    error stays within 8 x 2^-24 of max(|gelu|, |v| (1 - Phi)) -- erff within a few ulp of a value in [-1, 1] that is then cancelled against
    1 on the negative side, where the result is |v| times a small difference -- and far inside the layer rule the GPU test applies."""
    v = draws.gelu_pre_activations(20000, seed=1)
    assert v.min() < -5.9 and v.max() > 5.9 and (v == 0).any()
    e = torch.special.erf((v * F32(0.70710678118654752)).float())
    got = (F32(0.5) * v * (1.0 + e).float()).float()
    want = F.gelu(v.double())
    err = (got.double() - want).abs()
    bound = 8 * 2.0 ** -24 * torch.maximum(want.abs(), v.double().abs()) + 2.0 ** -30
    print("gelu form: worst err %.3e, worst err / bound %.3f, most negative output %.4f" % (err.max().item(), (err / bound).max().item(), want.min().item()))
    assert (err <= bound).all()
    assert abs(want.min().item() + 0.17) < 0.005                        # the negative lobe's minimum, -0.17 at v = -0.75


def test_the_draws_are_what_they_claim():
    x = draws.planes((3, 9, 9, 96), seed=1)
    assert torch.equal(draws.valid_pairs(x), x) and (x == 0).any() and (x < 0).any() and (x > 0).any()
    assert len({(k[1], k[2]) for k in draws.C_F if k[0] == "dw"}) == len({(c, h) for c, h, _b in draws.DW_CASES})
    assert all(("ln",) + t in draws.C_F for t in draws.LN_CASES) and all(("pool", hw, c) in draws.C_F for hw, c, _b in draws.POOL_CASES)
    assert all(math.log2(v) == int(math.log2(v)) for v in draws.C_F.values())
