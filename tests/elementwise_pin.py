"""The cases behind tests/golden/elementwise_digests.json: the public element-wise entries that share a kernel template (the run-form depthwise
conv, the global average pools, the no-padding stride-2 pair-copy max pools, the LayerNorm over C) on fixed inputs, and the sha256 of every
output plane.  tests/golden/make_elementwise_digests.py records them, tests/test_gpu_elementwise_pin.py replays them.

Inputs are split-fp16 planes drawn on the CPU from numpy's frozen RandomState stream, seeded per case by the crc32 of the case's id.  Every
case mixes in: -0.0 (in one plane and in both), values above 6, values below -90 (expf(-x) overflows in silu), channel 1 all -0.0 in both planes
(an all -0.0 window and column), channel 2 one constant pair (ties inside every max window), channel 3 two DIFFERENT pairs of one sum drawn per
pixel ((2, 0) and (1, 1): a tie that only "the first wins" decides), and the last two channels exact zeros (pad channels; the depthwise
weights, scale and shift are zero there too).  Batch 3 everywhere, so the last workgroup is partial."""
import hashlib
import zlib

import numpy as np
import torch
from gpu_common import ptr as _p

BATCH = 3
EPS = 1e-6
GUARD = 64          # NaN halves behind every output plane: a kernel must leave them alone

DW_SHAPES = [(hin, stride, pitch) for hin in (1, 5, 6, 9) for stride in (1, 2) for pitch in (8, 24)]
ACTS = ((0, 0), (1, 0), (0, 1), (1, 1))


def cases():
    """-> [(family, id, args)], in a fixed order."""
    out = []
    for hin, stride, pitch in DW_SHAPES:
        out.append(("dw", "dwconv3x3_bn/hin%d/s%d/p%d" % (hin, stride, pitch), (3, hin, stride, pitch, None)))
    for k in (3, 5):
        for hin, stride, pitch in DW_SHAPES:
            for act in ACTS:
                out.append(("dwact", "dwconv_bn_act/k%d/hin%d/s%d/p%d/act%d%d" % ((k, hin, stride, pitch) + act), (k, hin, stride, pitch, act)))
    for entry in ("global_avgpool", "global_avgpool_clamp6", "global_avgpool_silu"):
        for hw in (1, 7, 49):
            for c in (8, 40):
                out.append(("gap", "%s/hw%d/c%d" % (entry, hw, c), (entry, hw, c)))
    for entry, hins in (("maxpool2x2s2", (2, 6)), ("maxpool3x3s2p0", (3, 7))):
        for hin in hins:
            for c in (8, 24):
                out.append(("maxpool", "%s/hin%d/c%d" % (entry, hin, c), (entry, hin, c)))
    for c in (96, 384, 768):
        for rows in (1, 7):
            for mb in (1, 0):
                out.append(("ln", "layernorm_c/C%d/rows%d/mb%d" % (c, rows, mb), (c, rows, None, mb)))
                for in_stride in (1, 3):
                    out.append(("ln", "layernorm_rows/C%d/rows%d/stride%d/mb%d" % (c, rows, in_stride, mb), (c, rows, in_stride, mb)))
    return out


def _rs(case_id, salt=b""):
    return np.random.RandomState(zlib.crc32(case_id.encode() + salt))


def planes(rs, pixels, pitch):
    """-> (hi, lo) fp16 [pixels][pitch] with the mix of the module docstring."""
    x = (rs.standard_normal((pixels, pitch)) * 3.0).astype(np.float32)
    m = rs.random_sample(x.shape)
    x[m < 0.04] *= 4.0                                                      # beyond +-6
    x[(m >= 0.04) & (m < 0.07)] = 8.5
    x[(m >= 0.07) & (m < 0.11)] = -100.0 - 100.0 * rs.random_sample(int(((m >= 0.07) & (m < 0.11)).sum())).astype(np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    neg0 = np.float16(-0.0)
    z1, z2 = (m >= 0.11) & (m < 0.14), (m >= 0.14) & (m < 0.17)
    hi[z1], lo[z1] = neg0, np.float16(0.0)                                  # hi + lo = +0
    hi[z2], lo[z2] = neg0, neg0                                             # hi + lo = -0
    hi[:, 1], lo[:, 1] = neg0, neg0
    hi[:, 2], lo[:, 2] = np.float16(1.5), np.float16(2.0 ** -12)
    pick = rs.randint(0, 2, size=pixels).astype(bool)
    hi[:, 3], lo[:, 3] = np.where(pick, np.float16(2.0), np.float16(1.0)), np.where(pick, np.float16(0.0), np.float16(1.0))
    hi[:, pitch - 2:], lo[:, pitch - 2:] = np.float16(0.0), np.float16(0.0)
    return np.ascontiguousarray(hi), np.ascontiguousarray(lo)


def dw_weights(rs, k, pitch):
    """-> w [k * k][pitch], scale, shift [pitch] fp32, zero on the two pad channels; both signs of the scale."""
    w = (rs.standard_normal((k * k, pitch)) * (2.0 / (k * k)) ** 0.5).astype(np.float32)
    sc = (rs.uniform(0.5, 2.5, pitch) * np.where(rs.random_sample(pitch) < 0.3, -1.0, 1.0)).astype(np.float32)
    sc[0] = -abs(sc[0])
    sh = (rs.standard_normal(pitch) * 0.5).astype(np.float32)
    w[:, pitch - 2:], sc[pitch - 2:], sh[pitch - 2:] = 0.0, 0.0, 0.0
    return w, sc, sh


def inputs(family, case_id, args):
    """-> the case's host arrays, in the order run() uploads them."""
    rs = _rs(case_id)
    if family in ("dw", "dwact"):
        k, hin, stride, pitch, _ = args
        return planes(rs, BATCH * hin * hin, pitch) + dw_weights(rs, k, pitch)
    if family == "gap":
        _, hw, c = args
        return planes(rs, BATCH * hw, c)
    if family == "maxpool":
        _, hin, c = args
        return planes(rs, BATCH * hin * hin, c)
    c, rows, in_stride, _ = args
    gamma = (rs.standard_normal(c) * 0.5 + 1.0).astype(np.float32)
    beta = (rs.standard_normal(c) * 0.5).astype(np.float32)
    return planes(rs, rows * (in_stride or 1), c) + (gamma, beta)


def inputs_digest():
    """One sha256 over every case's inputs: tells a drift of the generator from a change of a kernel."""
    h = hashlib.sha256()
    for family, case_id, args in cases():
        for a in inputs(family, case_id, args):
            h.update(a.tobytes())
    return h.hexdigest()


def run(eng, family, case_id, args):
    """Runs one case through the engine's library.  -> [sha256 of the output hi plane, of the lo plane]."""
    from network_interpretation_imagenet_amd import _lib
    lib, h, dev = eng._lib, eng._h, eng.device
    up = [torch.from_numpy(a).to(dev) for a in inputs(family, case_id, args)]
    xh, xl = up[0], up[1]
    if family in ("dw", "dwact"):
        k, hin, stride, pitch, act = args
        ho = (hin - 1) // stride + 1
        n_out = BATCH * ho * ho * pitch
    elif family == "gap":
        entry, hw, c = args
        n_out = BATCH * c
    elif family == "maxpool":
        entry, hin, c = args
        ho = hin // 2 if entry == "maxpool2x2s2" else (hin - 3) // 2 + 1
        n_out = BATCH * ho * ho * c
    else:
        c, rows, in_stride, mb = args
        n_out = rows * c
    oh = torch.full((n_out + GUARD,), float("nan"), dtype=torch.float16, device=dev)
    ol = torch.full_like(oh, float("nan"))
    st = eng._stream()
    if family == "dw":
        rc = lib.mpx_dwconv3x3_bn(h, _p(xh), _p(xl), _p(up[2]), _p(up[3]), _p(up[4]), _p(oh), _p(ol), BATCH, hin, pitch, stride, st)
    elif family == "dwact":
        rc = lib.mpx_dwconv_bn_act(h, _p(xh), _p(xl), _p(up[2]), _p(up[3]), _p(up[4]), _p(oh), _p(ol), BATCH, hin, pitch, k, stride, act[0], act[1], st)
    elif family == "gap":
        rc = getattr(lib, "mpx_" + entry)(h, _p(xh), _p(xl), _p(oh), _p(ol), BATCH, hw, c, st)
    elif family == "maxpool":
        rc = getattr(lib, "mpx_" + entry)(h, _p(xh), _p(xl), _p(oh), _p(ol), BATCH, hin, c, st)
    elif in_stride is None:
        rc = lib.mpx_layernorm_c(h, _p(xh), _p(xl), _p(up[2]), _p(up[3]), EPS, _p(oh), _p(ol), rows, c, mb, st)
    else:
        rc = lib.mpx_layernorm_rows(h, _p(xh), _p(xl), _p(up[2]), _p(up[3]), EPS, _p(oh), _p(ol), rows, in_stride, c, mb, st)
    _lib.check(h, rc, case_id)
    torch.cuda.synchronize()
    assert torch.isnan(oh[n_out:]).all() and torch.isnan(ol[n_out:]).all(), case_id + ": wrote behind its output planes"
    return [hashlib.sha256(t[:n_out].cpu().numpy().tobytes()).hexdigest() for t in (oh, ol)]
