"""Where the constants of tests/test_gpu_fused_edges.py come from, without a GPU.  The block tail (csrc/mpx_btail.h) keeps conv2's output -- and,
with t1 = NULL, conv1's -- inside the launch, so its block output cannot be held to a single layer's bound: this file emulates the CHAIN with
tests/test_conv_bounds_cpu.py's numpy model of the kernels' arithmetic, layer after layer, each stage fed the emulated hi / lo planes of the one
before, with the library's own packer for the plain layers and a numpy restatement of build_fused (csrc/mpx_api.hip) for layer1.0's
K-concatenated conv3 + downsample.  It measures r_chain = max err / (2^-22 B + 2^-24) against the fp64 chain of fused_edge_draws, asserts that
fused_edge_draws.C_CHAIN is 4 x the worst r_chain rounded up to a power of two, checks the preconditions on every reference the GPU file uses,
shows an error on the block output that the max norm passes and the per-element bound does not, and counts the tile geometry by hand."""
import math

import numpy as np
import pytest
import torch

import conv_edge_draws as ced
import fused_edge_draws as fed
import test_conv_bounds_cpu as cb

F32 = np.float32
CHAINS = [(0, True), (0, False), (1, False), (2, False)]            # (block of layer1, whole: conv1 runs in the launch too)
KINDS = ("synthetic", "trained_like")
_measured = {}


def pack_fused(sd, d3, dd):
    """build_fused (csrc/mpx_api.hip) in numpy: per output channel s = max(|s3|, |sd|), the row [W3 s3/s | Wd sd/s] rounded to fp32 once, scaled by
    the power of two that puts its largest entry into [512, 1024), split into hi + lo; scale = s 2^-e, shift = shift3 + shiftd from fp64."""
    f = lambda key: sd[key].float().numpy().astype(np.float64)         # the engine keeps fp32 host copies and folds them in double
    eps = np.float64(F32(ced.BN_EPS))
    s3 = f(d3.bn_name + ".weight") / np.sqrt(f(d3.bn_name + ".running_var") + eps)
    sdn = f(dd.bn_name + ".weight") / np.sqrt(f(dd.bn_name + ".running_var") + eps)
    s = np.maximum(np.abs(s3), np.abs(sdn))
    s = np.where((s > 0) & np.isfinite(s), s, 1.0)
    row = np.concatenate([(f(d3.name + ".weight").reshape(d3.cout, d3.cin) * (s3 / s)[:, None]).astype(F32),
                          (f(dd.name + ".weight").reshape(dd.cout, dd.cin) * (sdn / s)[:, None]).astype(F32)], axis=1)
    mx = np.abs(row).max(1)
    e = np.where(mx > 0, 10 - np.frexp(mx)[1], 0)
    sv = np.ldexp(row, e[:, None]).astype(F32)
    w_hi = sv.astype(np.float16)
    w_lo = (sv - w_hi.astype(F32)).astype(np.float16)
    shift = (f(d3.bn_name + ".bias") - f(d3.bn_name + ".running_mean") * s3) + (f(dd.bn_name + ".bias") - f(dd.bn_name + ".running_mean") * sdn)
    top = np.abs(w_hi.astype(F32) + w_lo.astype(F32)).max(1)
    assert ((top >= 512) & (top < 1024)).all()
    return w_hi.astype(F32), w_lo.astype(F32), np.ldexp(s, -e).astype(F32), shift.astype(F32)


def _planes(hl, d, batch):
    return tuple(torch.from_numpy(np.ascontiguousarray(q)).view(batch, d.hout, d.hout, d.cout) for q in hl)


def emulate_chain(mpx_lib, sd, t, t1, x, whole, fused=None):
    """The block output of tail t as the emulated kernels compute it -> (hi, lo) fp16 [M][256].  t1 / x: (hi, lo, merged) planes."""
    batch = x[0].shape[0]
    th, tl = t1[0], t1[1]
    if whole:
        th, tl = _planes(cb.emulate(t.d1, cb.pack(mpx_lib, sd, t.d1), x[0], x[1], None), t.d1, batch)
    t2 = _planes(cb.emulate(t.d2, cb.pack(mpx_lib, sd, t.d2), th, tl, None), t.d2, batch)
    if t.dd is None:
        return cb.emulate(t.d3, cb.pack(mpx_lib, sd, t.d3), t2[0], t2[1], x[:2])
    cat = t.d3._replace(cin=t.d3.cin + t.dd.cin, residual=0)                   # one K-concatenated 1x1 layer over [t2 | x]
    fused = pack_fused(sd, t.d3, t.dd) if fused is None else fused
    return cb.emulate(cat, fused, torch.cat([t2[0], x[0]], -1), torch.cat([t2[1], x[1]], -1), None)


def _merged(hl):
    return torch.from_numpy(hl[0].astype(np.float64) + hl[1].astype(np.float64))


def measure(mpx_lib, kind, k, whole, mixed):
    """One emulated chain on image 0 of the GPU test's draw, computed once: (pre, want, B, hi, lo, got, r_chain)."""
    key = (kind, k, whole, mixed)
    if key not in _measured:
        sd, t = cb.state_dict(kind), fed.block_tail(k)
        t1, x = fed.tail_draws(t, 1, mixed)
        pre, want, b = (q.reshape(-1, t.d3.cout) for q in fed.tail_reference(sd, t, t1[2], x[2], whole))
        hi, lo = emulate_chain(mpx_lib, sd, t, t1, x, whole)
        got = _merged((hi, lo))
        r = ((got - want).abs() / (2.0 ** -22 * b + 2.0 ** -24)).max().item()
        _measured[key] = (pre, want, b, hi, lo, got, r)
    return _measured[key]


@pytest.mark.parametrize("k,whole", CHAINS)
@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mixed"])
@pytest.mark.parametrize("kind", KINDS)
def test_emulated_chain_stays_inside_the_bound(mpx_lib, kind, k, whole, mixed):
    pre, want, b, hi, lo, got, r = measure(mpx_lib, kind, k, whole, mixed)
    print("r_chain %-12s layer1.%d%s %s: %.3f (max norm: %.2e)" % (kind, k, " whole" if whole else "", "mixed" if mixed else "plain", r,
                                                                   (got - want).abs().max().item() / max(want.abs().max().item(), 1.0)))
    assert ((got - want).abs() <= fed.tol_chain(b)).all()
    assert ced.max_norm_ok(got, want)
    neg = (pre < -fed.tol_chain(b)).numpy()                 # exact zeros where the pre-activation is clearly negative: +0 in both planes
    assert neg.any() and (hi.view(np.uint16)[neg] == 0).all() and (lo.view(np.uint16)[neg] == 0).all()


def test_c_chain_is_four_times_the_worst_r_chain(mpx_lib):
    worst = max(measure(mpx_lib, kind, k, whole, mixed)[6] for kind in KINDS for mixed in (False, True) for k, whole in CHAINS)
    print("worst r_chain %.3f over %d chains; recorded %.3f; C_CHAIN %g" % (worst, len(_measured), fed.R_CHAIN_MAX, fed.C_CHAIN))
    assert abs(worst - fed.R_CHAIN_MAX) <= 0.05 * fed.R_CHAIN_MAX, "fused_edge_draws.R_CHAIN_MAX is not what this file measures: %.3f" % worst
    assert fed.C_CHAIN == 2.0 ** math.ceil(math.log2(4 * worst))


def test_the_propagated_error_of_t2_is_small_next_to_the_last_layers_own(mpx_lib):
    """Why no first-order propagated term |s3| (|W3| * tol_t2) is in the bound (it is about 16 x the single-layer term): with the last layer fed
    the fp64 chain's rounded t2 instead of the emulated one, r is 0.74; the whole chain's is 1.17 -- t2's own error costs less than the last
    layer's rounding does (layer1.1, trained-like, mixed)."""
    sd, t = cb.state_dict("trained_like"), fed.block_tail(1)
    t1, x = fed.tail_draws(t, 1, True)
    _pre, want, b = (q.reshape(-1, 256) for q in fed.tail_reference(sd, t, t1[2], x[2]))
    t2 = ced.split(fed.round_split(ced.reference(sd, t.d2, t1[2], None)[1]))
    alone = _merged(cb.emulate(t.d3, cb.pack(mpx_lib, sd, t.d3), t2[0], t2[1], x[:2]))
    r_alone = ((alone - want).abs() / (2.0 ** -22 * b + 2.0 ** -24)).max().item()
    r_chain = measure(mpx_lib, "trained_like", 1, False, True)[6]
    print("layer1.1 trained-like mixed: r of conv3 alone on the reference's t2 %.3f, of the chain %.3f" % (r_alone, r_chain))
    assert r_chain <= 2 * r_alone


# ------------------------------------------------------------------------------------------------
# the preconditions of the GPU test, on the references alone
# ------------------------------------------------------------------------------------------------
def _report(what, want):
    top, small = ced.preconditions(want)
    print("%s: max |want| %.3g, %.1f %% of the elements under 1 %% of it" % (what, top, 100 * small))


@pytest.mark.parametrize("k,whole", CHAINS)
@pytest.mark.parametrize("kind,mixed", [("synthetic", False), ("trained_like", True)])
def test_preconditions_hold_on_the_block_tail_references(kind, mixed, k, whole):
    """Block output and next conv1 (here: of the reference's own rounded block output) of image 0 of every draw the GPU file launches."""
    sd, t = cb.state_dict(kind), fed.block_tail(k)
    t1, x = fed.tail_draws(t, 1, mixed)
    for q in t1[:2] + x[:2]:
        assert torch.isfinite(q).all()
    _pre, want, b = fed.tail_reference(sd, t, t1[2], x[2], whole)
    assert (b >= want.abs()).all()
    _report("layer1.%d%s %s out" % (k, " whole" if whole else "", kind), want)
    _report("layer1.%d%s %s next conv1" % (k, " whole" if whole else "", kind), fed.next_reference(sd, t.dn, fed.round_split(want))[1])


@pytest.mark.parametrize("arch,kind,mixed,k", [("resnet50", "synthetic", False, 1), ("resnet50", "synthetic", False, 2),
                                               ("resnet101", "trained_like", True, 1), ("resnet101", "trained_like", True, 2)])
def test_preconditions_hold_on_the_pointwise_tail_references(arch, kind, mixed, k):
    sd, t = cb.state_dict(kind, arch), fed.pointwise_tail(k, arch)
    t2, x = fed.ptail_draws(t, 1, mixed, arch=arch)
    _pre, want, _b = ced.reference(sd, t.d3, t2[2], x[2])
    _report("%s layer2.%d %s out" % (arch, k, kind), want)
    _report("%s layer2.%d %s next conv1" % (arch, k, kind), fed.next_reference(sd, t.dn, fed.round_split(want))[1])


@pytest.mark.parametrize("kind,mixed", [("synthetic", False), ("synthetic", True), ("trained_like", True)])
def test_preconditions_hold_on_the_stem_references(kind, mixed):
    """Images 0 (all kept), 1 (all removed: relu(shift) everywhere, B = |shift|) and 2 (about half)."""
    sd = cb.state_dict(kind)
    hi, lo, x = fed.stem_draws(3, mixed)
    assert torch.equal(ced.merge(hi, lo), x) and (x[1] == 0).all() and (x[0] != 0).any(-1).all()
    frac = (x[2] != 0).any(-1).double().mean().item()
    assert 0.3 < frac < 0.7
    pre, want, b = ced.reference(sd, fed.STEM, x, None)
    _s, shift = ced.bn_affine(sd, fed.STEM)
    assert torch.equal(b[1], shift.abs().expand_as(b[1])) and torch.equal(want[1], torch.relu(shift).expand_as(want[1]))
    _report("stem %s %s" % (kind, "mixed" if mixed else "plain"), want)
    pw, ptol, zero = fed.pool_reference(pre, want, b)
    _report("stem + pool %s %s" % (kind, "mixed" if mixed else "plain"), pw)
    assert zero.any() and (pw[zero] == 0).all() and (ptol >= 2.0 ** -24).all()
    if mixed:
        assert x[..., 0].abs().max() < 1e-2 and x[..., 1].abs().max() > 20


# ------------------------------------------------------------------------------------------------
# the two checks differ
# ------------------------------------------------------------------------------------------------
def test_max_norm_passes_what_the_chain_bound_catches(mpx_lib):
    """Trained-like layer1.0's block output, the folded shift (shift3 + shift_d, build_fused) of its quietest channel off by 2^-10 of itself: the
    max norm of the tensor passes it, the per-element bound turns red on that channel and on no other."""
    sd, t = cb.state_dict("trained_like"), fed.block_tail(0)
    t1, x = fed.tail_draws(t, 1, False)
    _pre, want, b = (q.reshape(-1, 256) for q in fed.tail_reference(sd, t, t1[2], x[2]))
    fused = pack_fused(sd, t.d3, t.dd)
    b_ch = b.max(0).values.numpy()
    shift = fused[3]
    quiet = b_ch < 0.01 * b.max().item()                    # (19: layer1.0.downsample has such channels, and bn3's scale there is as small)
    assert quiet.any()
    ch = int(np.argmax(np.where(quiet, (want > 0).sum(0).numpy(), -1)))    # the quiet channel the ReLU hides least
    assert quiet[ch] and shift[ch] != 0 and (want[:, ch] > 0).any()
    good = _merged(emulate_chain(mpx_lib, sd, t, t1, x, False))
    assert ((good - want).abs() <= fed.tol_chain(b)).all() and ced.max_norm_ok(good, want)
    off = shift.copy()
    off[ch] = F32(shift[ch] * (1 + 2.0 ** -10))
    bad = _merged(emulate_chain(mpx_lib, sd, t, t1, x, False, fused=fused[:3] + (off,)))
    others = np.arange(256) != ch
    assert torch.equal(bad[:, others], good[:, others])
    over = (bad - want).abs() > fed.tol_chain(b)
    print("channel %d: shift %.4g, B <= %.3g of %.3g; max norm %.2e of 4e-6; %d of %d elements of the channel over their bound, worst err / tol %.1f"
          % (ch, shift[ch], b_ch[ch], b.max(), (bad - want).abs().max().item() / max(want.abs().max().item(), 1.0), int(over.sum()), want.shape[0],
             ((bad - want).abs() / fed.tol_chain(b)).max().item()))
    assert ced.max_norm_ok(bad, want)
    assert over[:, ch].any() and not over[:, others].any()


# ------------------------------------------------------------------------------------------------
# geometry, counted by hand
# ------------------------------------------------------------------------------------------------
def test_geometry_and_batches():
    assert fed.BT_TILES_PER_IMAGE == 28 and fed.POOL_BLOCKS_PER_IMAGE == 56 and fed.PT_PIXELS == 784
    # block tail, 256 CUs: 28 tiles on a grid of 32 (four workgroups without a tile); 532 tiles on 512 workgroups; 1036 tiles: a third tile
    assert fed.tail_batches(256) == [1, 19, 37]
    assert (fed.tail_tiles(1), fed.tail_grid(1, 256)) == (28, 32) and (fed.tail_tiles(18), fed.tail_grid(18, 256)) == (504, 504)
    assert (fed.tail_tiles(19), fed.tail_grid(19, 256)) == (532, 512) and (fed.tail_tiles(36), fed.tail_tiles(37)) == (1008, 1036)
    assert fed.tail_batches(304) == [1, 22, 44]             # 608 workgroups: 22 * 28 = 616, 44 * 28 = 1232 > 1216
    # pointwise tail: 784 B mod 128 is a multiple of 16; ragged 16, ragged 112, none (49 whole tiles), 515 tiles on 512 workgroups (ragged 64)
    assert fed.ptail_batches(256) == [1, 7, 8, 84]
    assert [fed.ptail_ragged(b) for b in (1, 7, 8, 84, 169)] == [16, 112, 0, 64, 16]
    assert fed.ptail_tiles(8) == 49 and fed.ptail_tiles(83) == 509 and fed.ptail_tiles(84) == 515 and fed.ptail_grid(84, 256) == 512
    assert fed.ptail_tiles(169) == 1036 and fed.ptail_grid(7, 256) == 43
    # stem: 112^2 = 49 * 256 pixels per image; P = 192 needs three images
    assert {t: fed.stem_batches(t) for t in fed.STEM_TILES} == {0: [1], 1: [1], 2: [1], 4: [1, 3], 7: [1]}
    assert ced.accepts(fed.STEM, 4) and fed.STEM.hout == (fed.STEM.hin + 2 * fed.STEM.pad - fed.STEM.ksize) // fed.STEM.stride + 1
    # the tails' layers are the topology's
    t = fed.block_tail(0)
    assert (t.d1.name, t.d2.name, t.d3.name, t.dd.name, t.dn.name) == ("layer1.0.conv1", "layer1.0.conv2", "layer1.0.conv3", "layer1.0.downsample.0", "layer1.1.conv1")
    t = fed.block_tail(2)
    assert t.dd is None and t.dn.name == "layer2.0.conv1" and t.dn.cout == 128 and t.dn.hin == 56
    p = fed.pointwise_tail(2)
    assert (p.d3.name, p.dn.name, p.d3.cin, p.d3.cout, p.dn.cout, p.d3.hout) == ("layer2.2.conv3", "layer2.3.conv1", 128, 512, 128, 28)
    keep = fed.stem_keep(3)
    assert keep[0].all() and not keep[1].any() and 60 < keep[2].sum() < 140
