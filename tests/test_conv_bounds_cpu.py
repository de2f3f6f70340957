"""The per-element bound of tests/test_gpu_conv_edges.py speaks for the kernels only if the arithmetic DESIGN.md 3 describes stays inside it: a
numpy emulation of that arithmetic -- the library's own weight packer (per-channel power-of-two scale into [512, 1024), hi + lo split), three
fp32 products per K chunk of 32 accumulated in fp32 in the order hi*lo, lo*hi, hi*hi, the epilogue acc * scale + shift (+ res), ReLU, the
re-split -- on the very draws the GPU test uses (tests/conv_edge_draws.py), against fp64.  It measures r_ref = max err / (2^-22 B + 2^-24),
asserts that conv_edge_draws.C_TOL is 4 x the worst r_ref rounded up to a power of two, checks on the reference alone the preconditions the
GPU test relies on, and shows an error the suite's older max norm passes and the per-element bound does not.  No GPU."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_edge_draws as ced
from network_interpretation_imagenet_amd import _lib, synth

F32 = np.float32
ARCH = "resnet101"
# K = 64, 576, 2048, 4608, the residual epilogue (K = 512), a layer without ReLU and fc (fp32 output, no BatchNorm); batch
EMULATED = [("layer1.0.conv1", 1), ("layer1.0.conv2", 1), ("layer4.1.conv1", 3), ("layer4.1.conv2", 3), ("layer4.2.conv3", 3),
            ("layer1.0.downsample.0", 1), ("fc", 129)]
_measured = {}


@functools.lru_cache(maxsize=None)
def state_dict(kind, arch=ARCH):
    if kind == "synthetic":
        return synth.make_state_dict(arch)
    from oracle import trained_like
    return trained_like.make_trained_like_state_dict(arch)


def _row_major(plane, rows, k):
    """Undo the piece-major order of a packed weight plane (include/mpx.h, mpx_pack_conv_weights)."""
    row = np.arange(rows)[:, None]
    kk = np.arange(k)[None, :]
    r = row % 16
    at = ((((row // 16) * (k // 32) + kk // 32) * 16 + r) * 4 + (((kk // 8) % 4) ^ ((r // 8) * 2))) * 8 + kk % 8
    return plane.ravel()[at]


def pack(mpx_lib, sd, d):
    """The library's packer on layer d: (w_hi, w_lo) fp16 [cout][K] with k = (ky, kx, ci), scale and shift fp32 [cout]."""
    cd = _lib.ConvDesc()
    cd.cin, cd.cout, cd.ksize = d.cin, d.cout, d.ksize
    cd.k_packed = d.ksize * d.ksize * d.cin
    cd.cout_pad = (d.cout + 127) // 128 * 128
    hi = np.zeros((cd.cout_pad, cd.k_packed), dtype=np.uint16)
    lo = np.zeros_like(hi)
    sc = np.zeros(cd.cout_pad, dtype=F32)
    sh = np.zeros(cd.cout_pad, dtype=F32)
    arr = lambda key: np.ascontiguousarray(sd[key].float().numpy())
    w = arr(d.name + ".weight").reshape(d.cout, d.cin, d.ksize, d.ksize)
    if d.bn_name:
        bn = [arr(d.bn_name + k) for k in (".weight", ".bias", ".running_mean", ".running_var")]
    else:
        bn = [None, arr(d.name + ".bias"), None, None]
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    rc = mpx_lib.mpx_pack_conv_weights(C.byref(cd), p(w), None, p(bn[0]), p(bn[1]), p(bn[2]), p(bn[3]), ced.BN_EPS, p(hi), p(lo), p(sc), p(sh))
    assert rc == 0
    unpack = lambda pl: _row_major(pl, cd.cout_pad, cd.k_packed).view(np.float16)[:d.cout].astype(F32)
    w_hi, w_lo = unpack(hi), unpack(lo)
    top = np.abs(w_hi + w_lo).max(1)
    assert ((top >= 512) & (top < 1024)).all()                      # the packer's scaling, as DESIGN.md 3 states it
    return w_hi, w_lo, sc[:d.cout], sh[:d.cout]


def _patches(x, d):
    """[B][hin][hin][cin] -> [M][K] with k = (ky, kx, ci), ci fastest: the K order of the packed weights."""
    k, s, ho = d.ksize, d.stride, d.hout
    if d.pad:
        x = np.pad(x, ((0, 0), (d.pad, d.pad), (d.pad, d.pad), (0, 0)))
    taps = [x[:, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (ho - 1) + 1:s, :] for ky in range(k) for kx in range(k)]
    return np.concatenate(taps, axis=-1).reshape(-1, k * k * d.cin)


def split_merge(v):
    hi = v.astype(np.float16)
    lo = (v - hi.astype(F32)).astype(np.float16)
    return hi, lo


def emulate(d, packed, x_hi, x_lo, res, shift=None):
    """The kernels' arithmetic for layer d -> (hi, lo) fp16 planes [M][cout]; fc: the fp32 output twice."""
    w_hi, w_lo, scale, sh = packed
    sh = sh if shift is None else shift
    xh, xl = _patches(x_hi.numpy().astype(np.float64), d), _patches(x_lo.numpy().astype(np.float64), d)
    w_hi, w_lo = w_hi.astype(np.float64), w_lo.astype(np.float64)
    acc = np.zeros((xh.shape[0], d.cout), dtype=F32)
    for c in range(0, xh.shape[1], 32):
        wh, wl = w_hi[:, c:c + 32].T, w_lo[:, c:c + 32].T
        # one MFMA = one product: the 32 terms (each exact: 11 x 11 bits) summed without intermediate rounding -- fp64 holds them -- and
        # rounded to fp32 once, then added to the fp32 accumulator
        for xa, wa in ((xl[:, c:c + 32], wh), (xh[:, c:c + 32], wl), (xh[:, c:c + 32], wh)):
            acc = (acc + (xa @ wa).astype(F32)).astype(F32)
    v = ((acc * scale).astype(F32) + sh).astype(F32)
    if res is not None:
        r = (res[0].numpy().astype(F32) + res[1].numpy().astype(F32)).reshape(-1, d.cout)
        v = (v + r).astype(F32)
    if d.relu:
        v = np.where(v <= 0, F32(0), v)
    if d.name == "fc":
        return v, v
    return split_merge(v)


def _case(mpx_lib, kind, name, batch, mixed):
    sd = state_dict(kind)
    d = ced.layer_desc(ARCH, name)
    x, res = ced.draws(d, batch, ced.draw_seed(ARCH, name), mixed)
    pre, want, b = ced.reference(sd, d, x[2], res[2] if res else None)
    return sd, d, x, res, pre, want.reshape(-1, d.cout), b.reshape(-1, d.cout)


def measure(mpx_lib, kind, name, batch, mixed):
    """One emulated case, computed once: (d, pre, want, B, hi, lo, got, r_ref)."""
    key = (kind, name, batch, mixed)
    if key not in _measured:
        sd, d, x, res, pre, want, b = _case(mpx_lib, kind, name, batch, mixed)
        hi, lo = emulate(d, pack(mpx_lib, sd, d), x[0], x[1], res[:2] if res else None)
        got = torch.from_numpy(hi.astype(np.float64) + lo.astype(np.float64)) if d.name != "fc" else torch.from_numpy(hi.astype(np.float64))
        floor = 2.0 ** -24 if d.name != "fc" else 0.0
        r_ref = ((got - want).abs() / (2.0 ** -22 * b + floor)).max().item()
        _measured[key] = (d, pre.reshape(-1, d.cout), want, b, hi, lo, got, r_ref)
    return _measured[key]


@pytest.mark.parametrize("name,batch", EMULATED)
@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mixed"])
@pytest.mark.parametrize("kind", ["synthetic", "trained_like"])
def test_emulated_arithmetic_stays_inside_the_bound(mpx_lib, kind, name, batch, mixed):
    d, pre, want, b, hi, lo, got, r_ref = measure(mpx_lib, kind, name, batch, mixed)
    print("r_ref %-12s %-14s K = %4d %s: %.3f (max norm: %.2e)" % (kind, name, d.cin * d.ksize ** 2, "mixed" if mixed else "plain", r_ref,
                                                                   (got - want).abs().max().item() / max(want.abs().max().item(), 1.0)))
    assert ((got - want).abs() <= ced.tol(b, d.name != "fc")).all()
    assert ced.max_norm_ok(got, want)
    if d.relu:           # exact zeros where the pre-activation is clearly negative: +0 in both planes
        neg = (pre < -ced.tol(b)).numpy()
        assert neg.any() and (hi.view(np.uint16)[neg] == 0).all() and (lo.view(np.uint16)[neg] == 0).all()


def test_c_tol_is_four_times_the_worst_r_ref(mpx_lib):
    """The constant the GPU test uses follows from what this file measures (the cases above, computed once)."""
    worst = max(measure(mpx_lib, kind, name, batch, mixed)[7] for kind in ("synthetic", "trained_like") for mixed in (False, True)
                for name, batch in EMULATED)
    print("worst r_ref %.3f over %d cases; recorded %.3f; C_TOL %g" % (worst, len(_measured), ced.R_REF_MAX, ced.C_TOL))
    assert abs(worst - ced.R_REF_MAX) <= 0.05 * ced.R_REF_MAX, "conv_edge_draws.R_REF_MAX is not what this file measures: %.3f" % worst
    assert ced.C_TOL == 2.0 ** math.ceil(math.log2(4 * worst))


# ------------------------------------------------------------------------------------------------
# the preconditions of the GPU test, on the reference alone
# ------------------------------------------------------------------------------------------------
def _few_images(d):
    """Images 0 .. n - 1 of a draw (the same numbers at every batch size): enough of them for a few thousand output elements."""
    return 129 if d.name == "fc" else (1 if d.hout >= 28 else 2 if d.hout == 14 else 4)


def _gpu_draws():
    """(arch, weights, layer, mixed, with_res) of every draw tests/test_gpu_conv_edges.py makes through mpx_conv_bn_act."""
    out = [("resnet101", "synthetic", d.name, False, bool(d.residual)) for d in ced.distinct_shapes("resnet101")]
    names = sorted({n for layers in ced.FORM_LAYERS.values() for n in layers})
    out += [("resnet101", "synthetic", n, False, bool(ced.layer_desc("resnet101", n).residual)) for n in names]
    out += [("resnet101", "trained_like", n, True, bool(ced.layer_desc("resnet101", n).residual)) for n in names]
    out += [("resnet101", "trained_like", n, False, False) for n in ced.QUIET_CHANNEL_LAYERS]
    out += [("resnet18", "synthetic", n, False, True) for n in ced.R18_RESIDUAL_LAYERS + (ced.R18_HANDOVER_LAYER,)]
    out += [("resnet50", "synthetic", "fc", False, False)]
    return sorted(set(out))


@pytest.mark.parametrize("arch,kind,name,mixed,with_res", _gpu_draws())
def test_preconditions_hold_on_the_reference(arch, kind, name, mixed, with_res):
    d = ced.layer_desc(arch, name)
    x, res = ced.draws(d, _few_images(d), ced.draw_seed(arch, name), mixed, with_res=with_res)
    for t in x[:2] + (res[:2] if res else ()):
        assert torch.isfinite(t).all()
    assert torch.equal(ced.merge(*ced.split(x[2])), x[2])                   # valid (hi, lo) pairs
    _pre, want, _b = ced.reference(state_dict(kind, arch), d, x[2], res[2] if res else None)
    top, small = ced.preconditions(want)
    if kind == "trained_like" and not mixed and name in ced.QUIET_CHANNEL_LAYERS:
        assert (_b.reshape(-1, d.cout).max(0).values < 0.01 * _b.max()).any()
    print("%s %s %s %s: max |want| %.3g, %.1f %% of the elements under 1 %% of it" % (arch, kind, name, "mixed" if mixed else "plain", top, 100 * small))
    if mixed:
        c = d.cin
        assert x[2][..., : c // 4].abs().max() < 1e-2 and x[2][..., c // 4: c // 2].abs().max() > 20


@pytest.mark.parametrize("stage", ced.DUAL_STAGES)
def test_preconditions_hold_on_the_dual_reference(stage):
    d3, dd = ced.layer_desc("resnet50", "layer%d.0.conv3" % stage), ced.layer_desc("resnet50", "layer%d.0.downsample.0" % stage)
    n = _few_images(d3)
    t2, _ = ced.draws(d3, n, ced.draw_seed("resnet50", d3.name), False, with_res=False)
    x, _ = ced.draws(dd, n, ced.draw_seed("resnet50", dd.name), False)
    _pre, want, b = ced.dual_reference(state_dict("synthetic", "resnet50"), d3, dd, t2[2], x[2])
    ced.preconditions(want)
    assert (b >= want.abs()).all()


def test_conv64_is_the_layers_own_conv():
    sd = state_dict("synthetic")
    for name in ("layer2.0.conv2", "layer2.0.downsample.0", "layer4.1.conv2"):          # 3x3 stride 2, 1x1 stride 2, 3x3 stride 1
        d = ced.layer_desc(ARCH, name)
        x, _ = ced.draws(d, 2, 3, True)
        w = sd[name + ".weight"].double()
        want = F.conv2d(x[2].double().permute(0, 3, 1, 2), w, None, d.stride, d.pad).permute(0, 2, 3, 1)
        got = ced.conv64(x[2], w, d, chunk_elems=d.hin * d.hin * d.cin)                # one image per chunk: the chunking too
        assert (got - want).abs().max() <= 1e-12 * want.abs().max()


# ------------------------------------------------------------------------------------------------
# the two checks differ
# ------------------------------------------------------------------------------------------------
def test_max_norm_passes_what_the_per_element_bound_catches(mpx_lib):
    """One output channel's shift off by 2^-12 |shift|, on a channel whose B is under 1 % of the tensor's largest (trained-like BatchNorm:
    layer1.0.downsample.1 has channels whose scale is a thousandth of their neighbours')."""
    sd, name = state_dict("trained_like"), "layer1.0.downsample.0"
    d = ced.layer_desc(ARCH, name)
    x, _ = ced.draws(d, 1, ced.draw_seed(ARCH, name), False)
    _pre, want, b = ced.reference(sd, d, x[2], None)
    want, b = want.reshape(-1, d.cout), b.reshape(-1, d.cout)
    packed = pack(mpx_lib, sd, d)
    b_ch = b.max(0).values
    quiet = (b_ch < 0.01 * b.max()).numpy()
    assert quiet.any()
    shift = packed[3]
    ch = int(np.argmax(np.where(quiet, np.abs(shift), 0)))
    assert quiet[ch] and shift[ch] != 0
    merged = lambda hl: torch.from_numpy(hl[0].astype(np.float64) + hl[1].astype(np.float64))
    good = merged(emulate(d, packed, x[0], x[1], None))
    assert ((good - want).abs() <= ced.tol(b)).all() and ced.max_norm_ok(good, want)
    off = shift.copy()
    off[ch] = F32(shift[ch] * (1 + 2.0 ** -12))
    bad = merged(emulate(d, packed, x[0], x[1], None, shift=off))
    assert torch.equal(bad[:, np.arange(d.cout) != ch], good[:, np.arange(d.cout) != ch])
    over = ((bad - want).abs() > ced.tol(b))
    print("channel %d: shift %.4g, B <= %.3g of %.3g; max norm %.2e of 4e-6; %d of %d elements of the channel over their bound, worst err / tol %.1f"
          % (ch, shift[ch], b_ch[ch], b.max(), (bad - want).abs().max().item() / max(want.abs().max().item(), 1.0), int(over.sum()), want.shape[0],
             ((bad - want).abs() / ced.tol(b)).max().item()))
    assert ced.max_norm_ok(bad, want)                                   # the older check passes it
    assert over[:, ch].any() and not over[:, np.arange(d.cout) != ch].any()     # the per-element bound does not


# ------------------------------------------------------------------------------------------------
# tile geometry
# ------------------------------------------------------------------------------------------------
def test_tile_table_and_edge_batches():
    assert sorted(ced.TILE_PIXELS) + [6, 12] == sorted(set(ced.ALL_TILES) - {6, 12}) + [6, 12]
    assert len(ced.distinct_shapes("resnet101")) == 23 == len(ced.distinct_shapes("resnet50"))
    l4, l2 = ced.layer_desc(ARCH, "layer4.1.conv2"), ced.layer_desc(ARCH, "layer2.1.conv2")
    assert ced.patch_tile(l4, 6) == ced.patch_tile(l4, 12) == "PatchTile2" and ced.tile_pixels(l4, 12) == 192       # 7x7 maps: 192 pixels
    assert ced.patch_tile(l2, 6) == "PatchTile0" and ced.patch_tile(ced.layer_desc(ARCH, "layer1.1.conv2"), 6) == "PatchTile1"
    assert not ced.accepts(ced.layer_desc(ARCH, "layer1.1.conv2"), 12) and not ced.accepts(ced.layer_desc("resnet18", "layer3.1.conv2"), 12)
    assert ced.accepts(ced.layer_desc("resnet18", ced.R18_HANDOVER_LAYER), 12)
    seen = set()
    for tile, names in ced.FORM_LAYERS.items():
        for name in names:
            d = ced.layer_desc(ARCH, name)
            assert ced.accepts(d, tile), (tile, name)
            p, howo = ced.tile_pixels(d, tile), d.hout * d.hout
            for cls, batch in ced.edge_batches(d, tile).items():
                r = {"1": 1, "P-1": p - 1, "0": 0}[cls]
                if batch is None:                                       # the helper says so: no batch at all has this residue
                    assert all(b * howo % p != r for b in range(1, p + 1)), (tile, name, cls)
                    continue
                seen.add((tile, cls))
                assert batch * howo % p == r and ced.expected_kernels(d, tile, batch, bool(d.residual)) == 1 << tile
                smaller = [b for b in range(1, batch) if b * howo % p == r and ced.expected_kernels(d, tile, b, bool(d.residual)) == 1 << tile]
                assert not smaller, (tile, name, cls, smaller)
    # every form but the weights-in-registers kernel (K = 256 exists on 14 x 14 maps and larger only) meets all three classes somewhere
    assert seen == {(t, c) for t in ced.ALL_TILES for c in ced.RESIDUES} - {(14, "1"), (14, "P-1")}
    # the persistent forms' batches are their round(s) of tiles and no more than one residue period above
    d = ced.layer_desc(ARCH, "layer4.2.conv3")
    assert ced.edge_batches(d, 10) == {"1": 81, "P-1": 175, "0": 128} and ced.expected_kernels(d, 10, 80, True) == 1 << 7
    d = ced.layer_desc(ARCH, "layer3.5.conv3")
    assert ced.edge_batches(d, 14)["0"] == 48 and ced.expected_kernels(d, 14, 32, True) == 1 << 7 and ced.expected_kernels(d, 14, 48, False) == 1 << 10
    # a split launch (the images behind the last whole round go to tile 2) is not an edge batch: the kernel must own the last tile
    d = ced.layer_desc(ARCH, "layer4.1.conv1")
    assert ced.expected_kernels(d, 13, 721, False) == (1 << 13 | 1 << 2) and ced.edge_batches(d, 13)["1"] == 1233
    assert ced.expected_kernels(d, 9, 700, False) == (1 << 9 | 1 << 2)           # tests/test_gpu_parity.py test_conv256_kernel's split case
