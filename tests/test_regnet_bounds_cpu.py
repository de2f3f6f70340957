"""The per-element bound of tests/test_gpu_regnet.py's grouped-layer test speaks for the kernel only if the arithmetic csrc/mpx_gconvw.h
describes stays inside it: a numpy emulation of that contract -- the packer's per-channel power-of-two scale into [512, 1024) and hi + lo
split, per group K = (ky, kx, ci) over the group's cg channels FLATTENED and padded to a multiple of 32 (a 32-wide chunk may straddle taps),
three products per chunk (each summed exactly and rounded to fp32 once) added to one fp32 accumulator in the order hi*lo, lo*hi, hi*hi, the
epilogue acc * scale + shift, ReLU, the re-split -- on the very draws the GPU test uses (tests/regnet_draws.py), against fp64.  It
re-measures r_ref per shape on every run, holds it within a factor of two of regnet_draws.R_REF, asserts that C_TOL follows from the record,
and checks on the reference alone the preconditions the GPU test relies on.  No GPU."""
import math

import numpy as np
import pytest
import torch

import regnet_draws as gd
import regnet_ref as ref
from network_interpretation_imagenet_amd import synth

F32 = np.float32
_measured = {}
_sd = {}


def state_dict(arch):
    if arch not in _sd:
        _sd[arch] = synth.make_state_dict(arch)
    return _sd[arch]


def pack(sd, d):
    """The packer's arithmetic (csrc/mpx_api.hip, pack_gconvw_weights) in numpy: (w_hi, w_lo) as float64 [groups][cg][KP] with
    k = (ky * 3 + kx) * cg + ci and zeros behind tap 8; scale and shift fp32 [width]."""
    w = sd[d.name + ".weight"].float().numpy()                          # [width][cg][3][3]
    C, cg, G = d.width, d.cg, d.groups
    kp = (9 * cg + 31) // 32 * 32
    mx = np.abs(w).reshape(C, -1).max(1)
    e = 10 - np.frexp(mx)[1]
    sv = np.ldexp(w, e[:, None, None, None]).astype(F32)
    hi = sv.astype(np.float16)
    lo = (sv - hi.astype(F32)).astype(np.float16)
    top = np.abs(hi.astype(F32) + lo.astype(F32)).reshape(C, -1).max(1)
    assert ((top >= 512) & (top < 1024)).all()
    planes = np.zeros((2, G, cg, kp))
    for k, src in enumerate((hi, lo)):
        planes[k, :, :, :9 * cg] = src.astype(np.float64).reshape(G, cg, cg, 9).transpose(0, 1, 3, 2).reshape(G, cg, 9 * cg)
    s, sh = gd.bn_affine(sd, d)
    scale = np.ldexp(s.numpy(), -e).astype(F32)
    return planes[0], planes[1], scale, sh.numpy().astype(F32)


def _patches(x, d):
    """[B][hin][hin][width] -> [groups][M][KP]: per group, k = (ky, kx, ci) flattened over the group's channels, zeros behind tap 8."""
    cg, G = d.cg, d.groups
    kp = (9 * cg + 31) // 32 * 32
    s, ho = d.stride, d.hout
    x = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros((G, x.shape[0] * ho * ho, kp))
    for t in range(9):
        ky, kx = divmod(t, 3)
        tap = x[:, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (ho - 1) + 1:s, :].reshape(-1, G, cg)
        out[:, :, t * cg:(t + 1) * cg] = tap.transpose(1, 0, 2)
    return out


def emulate(d, packed, x_hi, x_lo):
    """The kernel's arithmetic for layer d -> (hi, lo) fp16 planes [M][width]."""
    w_hi, w_lo, scale, sh = packed
    xh, xl = _patches(x_hi.numpy().astype(np.float64), d), _patches(x_lo.numpy().astype(np.float64), d)
    G, m, kp = xh.shape
    acc = np.zeros((G, m, d.cg), dtype=F32)
    for c in range(0, kp, 32):
        wh, wl = w_hi[:, :, c:c + 32], w_lo[:, :, c:c + 32]
        for xa, wa in ((xl[:, :, c:c + 32], wh), (xh[:, :, c:c + 32], wl), (xh[:, :, c:c + 32], wh)):
            acc = (acc + np.matmul(xa, wa.transpose(0, 2, 1)).astype(F32)).astype(F32)
    acc = acc.transpose(1, 0, 2).reshape(m, d.width)
    v = ((acc * scale).astype(F32) + sh).astype(F32)
    v = np.where(v <= 0, F32(0), v)
    hi = v.astype(np.float16)
    return hi, (v - hi.astype(F32)).astype(np.float16)


def measure(d):
    """One emulated case at the largest batch the GPU test runs, computed once: (pre, want, B, hi, lo, got, r_ref)."""
    key = (d.arch, d.name)
    if key not in _measured:
        sd = state_dict(d.arch)
        x = gd.draws(d, gd.batches(d)[-1])
        pre, want, b = (t.reshape(-1, d.width) for t in gd.reference(sd, d, x[2]))
        hi, lo = emulate(d, pack(sd, d), x[0], x[1])
        got = torch.from_numpy(hi.astype(np.float64) + lo.astype(np.float64))
        r_ref = ((got - want).abs() / (2.0 ** -22 * b + 2.0 ** -24)).max().item()
        _measured[key] = (pre, want, b, hi, lo, got, r_ref)
    return _measured[key]


CASES = gd.all_cases()
IDS = ["%s-%s" % (d.arch, d.name) for d in CASES]


def test_the_cases_are_every_distinct_grouped_shape_of_the_five_networks():
    """(cg, groups, stride, input map): stride 2 in block 0 of every stage, stride 1 in the others; the 8GF network's first stage is dense."""
    want = {}
    for arch in ref.ARCHS:
        _id, widths, depths, gw, groups, _p, _m, _n = ref.TABLE[arch]
        rows, h = [], 112
        for w, dpt, g in zip(widths, depths, groups):
            if g > 1:
                rows.append((w // g, g, 2, h))
                if dpt > 1:
                    rows.append((w // g, g, 1, h // 2))
            h //= 2
        want[arch] = sorted(rows)
    for arch in ref.ARCHS:
        assert sorted((d.cg, d.groups, d.stride, d.hin) for d in CASES if d.arch == arch) == want[arch], arch
    assert len(CASES) == 7 + 7 + 8 + 8 + 5
    assert {d.cg for d in CASES} == {16, 24, 48, 120} and {7, 17, 25, 38, 42} <= {d.groups for d in CASES}
    assert max(d.hin * d.hin * d.width for d in CASES) == 112 * 112 * 96
    assert set(gd.R_REF) == {(d.arch, d.name) for d in CASES} == set(gd.C_TOL)
    assert len({gd.draw_seed(d) for d in CASES}) == len(CASES)


@pytest.mark.parametrize("d", CASES, ids=IDS)
def test_emulated_arithmetic_stays_inside_the_bound_and_the_constant_follows(d):
    pre, want, b, hi, lo, got, r_ref = measure(d)
    key = (d.arch, d.name)
    print("r_ref %s %s cg %3d groups %2d stride %d map %3d: %.3f (recorded %.3f, C %g)"
          % (d.arch, d.name, d.cg, d.groups, d.stride, d.hin, r_ref, gd.R_REF[key], gd.C_TOL[key]))
    assert gd.R_REF[key] / 2 <= r_ref <= 2 * gd.R_REF[key], "regnet_draws.R_REF is not what this file measures: %.3f" % r_ref
    assert gd.C_TOL[key] == 2.0 ** math.ceil(math.log2(4 * gd.R_REF[key]))
    assert ((got - want).abs() <= gd.tol(d, b)).all()
    neg = (pre < -gd.tol(d, b)).numpy()      # exact zeros where the pre-activation is clearly negative: +0 in both planes
    assert neg.any() and (hi.view(np.uint16)[neg] == 0).all() and (lo.view(np.uint16)[neg] == 0).all()


@pytest.mark.parametrize("d", CASES, ids=IDS)
def test_preconditions_hold_on_the_reference(d):
    batch = gd.batches(d)[-1]
    x = gd.draws(d, batch)
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
    if batch > 1:
        assert not torch.equal(x[2][0], x[2][1])
    _pre, want, b = measure(d)[:3]
    top, small = gd.preconditions(want)
    assert (b >= want.abs()).all()
    print("%s %s: max |want| %.3g, %.1f %% of the elements under 1 %% of it" % (d.arch, d.name, top, 100 * small))


def test_reference_is_grouped():
    """gconv64 against F.conv2d(groups=...) on a stride-1 cg = 120 layer, a stride-2 cg = 24 layer with 17 groups and a cg = 16 layer with 25."""
    for arch, name in (("regnet_x_8gf", "trunk_output.block4.block4-0.f.b.0"), ("regnet_x_1_6gf", "trunk_output.block3.block3-0.f.b.0"),
                       ("regnet_x_400mf", "trunk_output.block4.block4-1.f.b.0")):
        d = gd.layer(arch, name)
        x = gd.draws(d, 1)[2]
        w = state_dict(arch)[d.name + ".weight"].double()
        want = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w, None, d.stride, 1, 1, d.groups).permute(0, 2, 3, 1)
        assert (gd.gconv64(x, w, d) - want).abs().max() <= 1e-12 * want.abs().max()
