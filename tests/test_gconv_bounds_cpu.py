"""The per-element bound of tests/test_gpu_resnext.py's grouped-layer test speaks for the kernel only if the arithmetic csrc/mpx_gconv.h
describes stays inside it: a numpy emulation of that arithmetic -- the packer's per-channel power-of-two scale into [512, 1024) and hi + lo
split, channel blocks of max(cg, 16) channels with block-diagonal zeros, K = (ky, kx, ci) over the block's channels padded to a multiple of
32, three products per K chunk of 32 (each summed exactly and rounded to fp32 once) added to one fp32 accumulator in the order hi*lo,
lo*hi, hi*hi, the epilogue acc * scale + shift, ReLU, the re-split -- on the very draws the GPU test uses (tests/gconv_draws.py), against
fp64.  It measures r_ref per shape, asserts that gconv_draws.R_REF / C_TOL are what follows from it, and checks on the reference alone the
preconditions the GPU test relies on.  No GPU."""
import math

import numpy as np
import pytest
import torch

import gconv_draws as gd
from network_interpretation_imagenet_amd import synth

F32 = np.float32
_measured = {}


def _batch(d):
    return 3 if d.hout == 7 else 1


def pack(sd, d):
    """The grouped packer's arithmetic (csrc/mpx_api.hip, pack_gconv_weights) in numpy: per channel block, (w_hi, w_lo) as float64
    [blocks][CB][KP] with k = (ky * 3 + kx) * CB + (input channel within the block), zeros off the block diagonal and behind tap 8; scale
    and shift fp32 [width]."""
    w = sd[d.name + ".weight"].float().numpy()                          # [width][cg][3][3]
    C, cg = d.width, d.cg
    cb = max(cg, 16)
    kp = (9 * cb + 31) // 32 * 32
    mx = np.abs(w).reshape(C, -1).max(1)
    e = 10 - np.frexp(mx)[1]
    sv = np.ldexp(w, e[:, None, None, None]).astype(F32)
    hi = sv.astype(np.float16)
    lo = (sv - hi.astype(F32)).astype(np.float16)
    top = np.abs(hi.astype(F32) + lo.astype(F32)).reshape(C, -1).max(1)
    assert ((top >= 512) & (top < 1024)).all()
    planes = np.zeros((2, C // cb, cb, kp))
    for co in range(C):
        blk, r = divmod(co, cb)
        c0 = co // cg * cg - blk * cb
        for t in range(9):
            planes[0, blk, r, t * cb + c0:t * cb + c0 + cg] = hi[co, :, t // 3, t % 3]
            planes[1, blk, r, t * cb + c0:t * cb + c0 + cg] = lo[co, :, t // 3, t % 3]
    s, sh = gd.bn_affine(sd, d)
    scale = np.ldexp(s.numpy(), -e).astype(F32)
    return planes[0], planes[1], scale, sh.numpy().astype(F32)


def _patches(x, d):
    """[B][hin][hin][width] -> [blocks][M][KP]: per channel block, k = (ky, kx, ci) with ci over the block's channels, zeros behind tap 8."""
    C, cb = d.width, max(d.cg, 16)
    kp = (9 * cb + 31) // 32 * 32
    s, ho = d.stride, d.hout
    x = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros((C // cb, x.shape[0] * ho * ho, kp))
    for t in range(9):
        ky, kx = divmod(t, 3)
        tap = x[:, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (ho - 1) + 1:s, :].reshape(-1, C // cb, cb)
        out[:, :, t * cb:(t + 1) * cb] = tap.transpose(1, 0, 2)
    return out


def emulate(d, packed, x_hi, x_lo):
    """The kernel's arithmetic for layer d -> (hi, lo) fp16 planes [M][width]."""
    w_hi, w_lo, scale, sh = packed
    xh, xl = _patches(x_hi.numpy().astype(np.float64), d), _patches(x_lo.numpy().astype(np.float64), d)
    nb, m, kp = xh.shape
    cb = w_hi.shape[1]
    acc = np.zeros((nb, m, cb), dtype=F32)
    for c in range(0, kp, 32):
        wh, wl = w_hi[:, :, c:c + 32], w_lo[:, :, c:c + 32]
        for xa, wa in ((xl[:, :, c:c + 32], wh), (xh[:, :, c:c + 32], wl), (xh[:, :, c:c + 32], wh)):
            acc = (acc + np.einsum("bmk,bck->bmc", xa, wa).astype(F32)).astype(F32)
    acc = acc.transpose(1, 0, 2).reshape(m, d.width)
    v = ((acc * scale).astype(F32) + sh).astype(F32)
    v = np.where(v <= 0, F32(0), v)
    hi = v.astype(np.float16)
    return hi, (v - hi.astype(F32)).astype(np.float16)


def measure(d):
    """One emulated case, computed once: (pre, want, B, hi, lo, got, r_ref)."""
    key = (d.arch, d.name)
    if key not in _measured:
        sd = synth.make_state_dict(d.arch)
        x = gd.draws(d, _batch(d))
        pre, want, b = (t.reshape(-1, d.width) for t in gd.reference(sd, d, x[2]))
        hi, lo = emulate(d, pack(sd, d), x[0], x[1])
        got = torch.from_numpy(hi.astype(np.float64) + lo.astype(np.float64))
        r_ref = ((got - want).abs() / (2.0 ** -22 * b + 2.0 ** -24)).max().item()
        _measured[key] = (pre, want, b, hi, lo, got, r_ref)
    return _measured[key]


CASES = gd.all_cases()
IDS = ["%s-%s" % (d.arch, d.name) for d in CASES]


def test_the_cases_are_every_distinct_grouped_shape_of_both_networks():
    assert sorted((d.cg, d.stride, d.hin) for d in CASES if d.arch == "resnext50_32x4d") == \
        sorted([(4, 1, 56), (8, 1, 28), (16, 1, 14), (32, 1, 7), (8, 2, 56), (16, 2, 28), (32, 2, 14)])
    assert sorted((d.cg, d.stride, d.hin) for d in CASES if d.arch == "resnext101_32x8d") == \
        sorted([(8, 1, 56), (16, 1, 28), (32, 1, 14), (64, 1, 7), (16, 2, 56), (32, 2, 28), (64, 2, 14)])
    assert set(gd.R_REF) == {(d.arch, d.name) for d in CASES} == set(gd.C_TOL)
    assert len({gd.draw_seed(d) for d in CASES}) == len(CASES)


@pytest.mark.parametrize("d", CASES, ids=IDS)
def test_emulated_arithmetic_stays_inside_the_bound_and_the_constant_follows(d):
    pre, want, b, hi, lo, got, r_ref = measure(d)
    key = (d.arch, d.name)
    print("r_ref %s %s cg %2d stride %d map %2d: %.3f (recorded %.3f, C %g)" % (d.arch, d.name, d.cg, d.stride, d.hin, r_ref, gd.R_REF[key], gd.C_TOL[key]))
    assert abs(r_ref - gd.R_REF[key]) <= 0.05 * gd.R_REF[key], "gconv_draws.R_REF is not what this file measures: %.3f" % r_ref
    assert gd.C_TOL[key] == 2.0 ** math.ceil(math.log2(4 * r_ref))
    assert ((got - want).abs() <= gd.tol(d, b)).all()
    neg = (pre < -gd.tol(d, b)).numpy()      # exact zeros where the pre-activation is clearly negative: +0 in both planes
    assert neg.any() and (hi.view(np.uint16)[neg] == 0).all() and (lo.view(np.uint16)[neg] == 0).all()


@pytest.mark.parametrize("d", CASES, ids=IDS)
def test_preconditions_hold_on_the_reference(d):
    x = gd.draws(d, _batch(d))
    assert all(torch.isfinite(t).all() for t in x)
    assert torch.equal(gd.merge(*gd.split(x[2])), x[2])                     # valid (hi, lo) pairs
    pos = torch.arange(d.width) % d.cg
    lo_band, hi_band = x[2][..., pos < d.cg // 4], x[2][..., (pos >= d.cg // 4) & (pos < d.cg // 2)]
    assert lo_band.abs().max() < 1e-2 and hi_band.abs().max() > 20
    # the dim band's lo plane lies in fp16's subnormals (below 2^-14), zeros are exact in both planes, both signs occur
    assert 0 < x[1][..., pos < d.cg // 4].float().abs().max() < 2.0 ** -14
    zero = x[2] == 0
    assert 0.1 < zero.float().mean() < 0.15 and (x[0][zero] == 0).all() and (x[1][zero] == 0).all()
    assert (x[2] < 0).any() and (x[2] > 0).any()
    # image n is the same numbers at every batch size
    assert torch.equal(gd.draws(d, 1)[2][0], x[2][0])
    if _batch(d) > 1:
        assert not torch.equal(x[2][0], x[2][1])
    _pre, want, b = measure(d)[:3]
    top, small = gd.preconditions(want)
    assert (b >= want.abs()).all()
    print("%s %s: max |want| %.3g, %.1f %% of the elements under 1 %% of it" % (d.arch, d.name, top, 100 * small))


def test_reference_is_grouped():
    """gconv64 against a dense conv of the zero-extended weight, and the bound's conv against the same on |.|."""
    d = gd.layer("resnext50_32x4d", "layer4.1.conv2")
    sd = synth.make_state_dict(d.arch)
    x = gd.draws(d, 2)[2]
    w = sd[d.name + ".weight"].double()
    dense = torch.zeros(d.width, d.width, 3, 3, dtype=torch.float64)
    for co in range(d.width):
        g = co // d.cg
        dense[co, g * d.cg:(g + 1) * d.cg] = w[co]
    want = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), dense, None, d.stride, 1).permute(0, 2, 3, 1)
    assert (gd.gconv64(x, w, d) - want).abs().max() <= 1e-12 * want.abs().max()
    for name in ("layer2.0.conv2", "layer1.0.conv2"):          # stride 2; cg = 4
        d = gd.layer("resnext50_32x4d", name)
        x = gd.draws(d, 1)[2]
        w = sd[d.name + ".weight"].double()
        want = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w, None, d.stride, 1, 1, gd.GROUPS).permute(0, 2, 3, 1)
        assert (gd.gconv64(x, w, d) - want).abs().max() <= 1e-12 * want.abs().max()
