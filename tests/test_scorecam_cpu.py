"""CPU tests of the Score-CAM path's host half: the C-ABI's declarations and bindings, the numpy restatements of masks.py (the ones
csrc/mpx_cam.h and csrc/mpx_softmask.h's MapWeights are held to on the GPU) against literal loops, against torch's F.interpolate and
against the published order of the method, the liveness of the pool's input in every architecture's plan, and the refusals that happen
before anything touches a device."""
import json
import os
import re

import numpy as np
import pytest
import torch

import plan_text
import scorecam_ref as ref
from network_interpretation_imagenet_amd import _lib, masks
from network_interpretation_imagenet_amd.engine import ARCH_IDS

IMG = 224
SYMBOLS = ("mpx_pool_input", "mpx_planes_to_chw", "mpx_cam_cells", "mpx_cam_apply", "mpx_cam_combine")
POOL_KINDS = {"2", "11", "12", "17", "20"}      # OP_AVGPOOL, OP_AVGPOOL6, OP_AVGLOGITS, OP_AVGPOOLSILU, OP_AVGPOOLLN (csrc/mpx_api.hip OpKind)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------------------------------
# declaration and binding
# ------------------------------------------------------------------------------------------------------------------------------------
def _header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__)))
    with open(os.path.join(root, "include", "mpx.h")) as fh:
        return fh.read()


def test_symbols_are_declared_and_bound_with_the_headers_argument_counts():
    header = _header()
    for name in SYMBOLS:
        decl = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M | re.S)
        assert decl, "%s is not declared in include/mpx.h" % name
        params = [p for p in decl.group(1).split(",") if p.strip()]
        assert name in _lib.SIGNATURES, "%s is not bound in _lib.SIGNATURES" % name
        assert len(_lib.SIGNATURES[name][1]) == len(params), (name, len(_lib.SIGNATURES[name][1]), len(params))
    assert [len(_lib.SIGNATURES[n][1]) for n in SYMBOLS] == [7, 10, 9, 11, 10]
    lo, hi = (int(re.search(r"#define MPX_CAM_GRID_%s (\d+)" % w, header).group(1)) for w in ("MIN", "MAX"))
    assert (lo, hi) == (2, 16) == (_lib.CAM_GRID_MIN, _lib.CAM_GRID_MAX) == (masks.CAM_GRID_MIN, masks.CAM_GRID_MAX)


def test_symbols_are_exported(mpx_lib):
    for name in SYMBOLS:
        assert getattr(mpx_lib, name) is not None


# ------------------------------------------------------------------------------------------------------------------------------------
# upsampling
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [2, 3, 7, 13, 16])
def test_axis_against_a_literal_loop(g):
    i0, i1, f = masks.cam_axis(g)
    w0, w1, wf = ref.axis_loop(g)
    assert (i0 == w0).all() and (i1 == w1).all() and f.dtype == np.float32 and (_bits(f) == _bits(wf)).all()
    assert i0[0] == 0 and f[0] == 0 and i0[223] == g - 1 and i1[223] == g - 1
    assert i0.min() == 0 and i0.max() == g - 1 and (i1 <= g - 1).all() and (f >= 0).all() and (f < 1).all()


@pytest.mark.parametrize("g", [2, 3, 7, 13, 16])
def test_upsample_against_torch_and_a_scalar_loop(g):
    rng = np.random.default_rng(g)
    G = rng.random((4, g, g), dtype=np.float32)
    up = masks.cam_upsample(G)
    assert up.dtype == np.float32 and up.shape == (4, IMG, IMG)
    d = float(np.abs(up - ref.torch_upsample(G).numpy()).max())
    print("g = %d: max |cam_upsample - F.interpolate| = %.3e" % (g, d))
    assert d <= 4e-6            # twice the largest difference measured (1.85e-6 at g = 16): torch rounds the source coordinate in fp32
    pixels = [(0, 0), (0, 223), (223, 0), (223, 223), (15, 16), (111, 112), (112, 111), (100, 7), (7, 100), (208, 209)]
    want = ref.upsample_loop(G[1], pixels)
    assert (_bits([up[1, y, x] for y, x in pixels]) == _bits(want)).all()
    assert (masks.cam_upsample(G[0]) == up[0]).all()                # a single [g, g] map


@pytest.mark.parametrize("g", range(2, 17))
def test_all_ones_and_all_zeros_are_exact(g):
    assert (masks.cam_upsample(np.ones((1, g, g), np.float32)) == 1.0).all()
    z = masks.cam_upsample(np.zeros((1, g, g), np.float32))
    assert (z == 0.0).all() and not np.signbit(z).any()
    assert (masks.cam_weights(np.ones((1, g, g), np.float32)) == 1.0).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# cells
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", ref.GRIDS)
def test_cells_extremes_validity_and_negative_maps(g):
    act = ref.activations(9, g)
    cells, lo, hi, valid = masks.cam_cells(act)
    assert cells.dtype == np.float32 and cells.shape == act.shape and lo.dtype == hi.dtype == np.float32 and valid.dtype == np.uint8
    up = masks.cam_upsample(act)
    assert (_bits(lo) == _bits(up.min(axis=(1, 2)))).all() and (_bits(hi) == _bits(up.max(axis=(1, 2)))).all()
    assert valid.tolist() == [1, 0, 0, 1, 1, 1, 1, 1, 1]
    for c in (1, 2):                                                # constant and all-zero: invalid, cells +0.0
        assert (cells[c] == 0).all() and not np.signbit(cells[c]).any()
    for c in np.flatnonzero(valid):
        want = (act[c] - lo[c]) / np.float32(hi[c] - lo[c])         # fp32: a rounded difference, a rounded divisor, one rounded quotient
        assert want.dtype == np.float32 and (_bits(cells[c]) == _bits(want)).all()
    assert (act[3] < 0).all() and valid[3] and abs(float(cells[3].min())) < 0.1 and 0.9 < float(cells[3].max()) < 1.1      # a negative map
    if g > 2:                                                       # the interior peak: no pixel centre reaches it
        assert hi[0] < act[0].max() and cells[0].max() > 1.0
    w = masks.cam_upsample(cells[valid.astype(bool)])
    assert w.min() >= -3e-7 and w.max() <= 1 + 3e-7                 # the unclamped weight leaves [0, 1] by rounding only


def test_cells_of_one_channel_and_of_many():
    act = ref.activations(70, 7)                                    # more than one block of the restatement's loop
    cells, lo, hi, valid = masks.cam_cells(act)
    for c in (0, 5, 63, 64, 69):
        one = masks.cam_cells(act[c:c + 1])
        assert (_bits(one[0][0]) == _bits(cells[c])).all() and one[1][0] == lo[c] and one[2][0] == hi[c] and one[3][0] == valid[c]


# ------------------------------------------------------------------------------------------------------------------------------------
# weights
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", ref.GRIDS)
def test_weights_lie_in_the_unit_interval_and_equal_the_published_order(g):
    act = ref.activations(12, g)
    cells, _lo, _hi, valid = masks.cam_cells(act)
    keep = valid.astype(bool)
    w = masks.cam_weights(cells[keep])
    assert w.dtype == np.float32 and w.shape == (int(keep.sum()), IMG, IMG)
    assert w.min() == 0.0 and w.max() == 1.0 and not np.signbit(w[w == 0]).any()      # exactly [0, 1]; the extremes are reached
    d = float(np.abs(w - ref.published_weights(act[keep])).max())
    print("g = %d: max |cam_weights - published order| = %.3e" % (g, d))
    assert d <= 6e-6            # measured <= 2.8e-6: torch's coordinate rounding, carried through the min-max
    assert (masks.cam_weights(ref.cells(3, g))[-1] == 1.0).all()    # the all-ones row
    both = masks.cam_weights(np.array([[[-0.5, -0.5], [-0.5, -0.5]], [[1.5, 1.5], [1.5, 1.5]]], dtype=np.float32))
    assert (both[0] == 0).all() and not np.signbit(both[0]).any() and (both[1] == 1).all()      # the clamp, both sides


# ------------------------------------------------------------------------------------------------------------------------------------
# combine
# ------------------------------------------------------------------------------------------------------------------------------------
def _combine_job(c=64, g=7, k=5, seed=0):
    rng = np.random.default_rng(seed)
    act = np.maximum(rng.standard_normal((c, g, g)).astype(np.float32), 0)      # post-ReLU
    return act, rng.random((c, k), dtype=np.float32)


def test_combine_is_the_written_order_and_does_not_depend_on_the_cut():
    act, scores = _combine_job()
    low, sal = masks.cam_combine(act, scores)
    assert low.dtype == sal.dtype == np.float32 and low.shape == (5, 7, 7) and sal.shape == (5, IMG, IMG)
    want = np.float32(0.0)
    for r in range(len(act)):                                       # one (class, cell) by hand: a rounded product, then a rounded sum
        want = np.float32(want + np.float32(scores[r, 2] * act[r, 3, 4]))
    assert low[2, 3, 4] == want
    up = masks.cam_upsample(low)
    assert (_bits(sal) == _bits(np.where(up > 0, up, np.float32(0)))).all()
    for cut in (1, 32, 33, 63):
        a = masks.cam_combine(act[:cut], scores[:cut])
        b = masks.cam_combine(act[cut:], scores[cut:], low0=a[0])
        assert (_bits(b[0]) == _bits(low)).all() and (_bits(b[1]) == _bits(sal)).all(), cut


def test_combine_against_the_published_order_in_fp64():
    """|restatement - fp64| <= 4 x |published order in fp32 torch - fp64|: reference against reference, factor 4."""
    act, scores = _combine_job()
    _low, sal = masks.cam_combine(act, scores)
    exact = ref.published_combine(act, scores, torch.float64)
    ours = float(np.abs(sal.astype(np.float64) - exact).max())
    theirs = float(np.abs(ref.published_combine(act, scores, torch.float32).astype(np.float64) - exact).max())
    print("combine at C = 64, g = 7, K = 5: |restatement - fp64| = %.3e, |published fp32 - fp64| = %.3e, map max %.3e" % (ours, theirs, exact.max()))
    assert theirs > 0 and ours <= 4 * theirs


def test_combine_relu_writes_positive_zero_and_no_rows_give_zero_maps():
    act, scores = _combine_job(8, 7, 2, seed=1)
    low, sal = masks.cam_combine(act, -scores)                      # every sum <= 0
    assert (low <= 0).all() and (low < 0).any() and (sal == 0).all() and not np.signbit(sal).any()
    low, sal = masks.cam_combine(act[:0], scores[:0])
    assert low.shape == (2, 7, 7) and sal.shape == (2, IMG, IMG) and (low == 0).all() and (sal == 0).all()
    assert not np.signbit(low).any() and not np.signbit(sal).any()


# ------------------------------------------------------------------------------------------------------------------------------------
# the plan: the pool's input is alive behind the forward
# ------------------------------------------------------------------------------------------------------------------------------------
def test_the_pools_input_is_live_behind_the_forward_in_every_plan(mpx_lib, golden_dir):
    """For every architecture: either no op list has a global-pool op, or every op list the architecture has (a list without records is a
    variant the architecture does not have) holds exactly one, and no op behind it writes (out, z) the buffer it reads -- the tap reads
    that buffer after the whole forward."""
    with open(os.path.join(golden_dir, "plan_digests.json")) as fh:
        archs = sorted(json.load(fh))
    assert archs == sorted(ARCH_IDS)
    with_pool, without = [], []
    for arch in archs:
        rc, text = plan_text.describe(mpx_lib, ARCH_IDS[arch])
        assert rc == 0, arch
        sec = plan_text.by_section(text)
        lists = [plan_text.records(sec[s]) for s in ("ops", "ops_bt", "ops_pt", "ops_pt0") if sec[s]]
        assert lists and sec["ops"], arch
        counts = [sum(o["kind"] in POOL_KINDS for o in ops) for ops in lists]
        if not any(counts):
            without.append(arch)
            continue
        assert counts == [1] * len(lists), (arch, counts)
        with_pool.append(arch)
        for ops in lists:
            at = next(i for i, o in enumerate(ops) if o["kind"] in POOL_KINDS)
            src = ops[at]["in"]
            assert int(src) >= 0 and int(ops[at]["hin"]) >= 1 and int(ops[at]["c"]) >= 8, (arch, ops[at])
            assert ops[at]["out"] != src
            for o in ops[at + 1:]:
                assert o["out"] != src and o["z"] != src, (arch, o)
    assert {"resnet18", "resnet50", "mobilenet_v2", "squeezenet1_1", "efficientnet_b0", "convnext_tiny", "densenet121"} <= set(with_pool)
    assert {"vgg11", "vgg19_bn", "alexnet", "vit_b_16", "vit_b_32"} <= set(without)
    assert {"mnist_net", "cifar_resnet20"} <= set(with_pool)        # the small networks pool too; mpx_pool_input refuses them as small


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals before the device
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [
    np.zeros((4, 7, 7), dtype=np.float64), np.zeros((4, 7, 6), dtype=np.float32), np.zeros((7, 7), dtype=np.float32),
    np.zeros((0, 7, 7), dtype=np.float32), np.zeros((4, 1, 1), dtype=np.float32), np.zeros((4, 17, 17), dtype=np.float32),
    np.full((2, 7, 7), np.nan, dtype=np.float32), np.full((2, 7, 7), np.inf, dtype=np.float32)],
    ids=["f64", "not-square", "2d", "no-channel", "g1", "g17", "nan", "inf"])
def test_check_activations_refuses(bad):
    with pytest.raises(ValueError):
        masks.check_activations(bad)
    with pytest.raises(ValueError):
        masks.cam_cells(bad)


def test_restatements_refuse_wrong_shapes():
    ok = masks.check_activations(np.ones((3, 16, 16), dtype=np.float32)[:, ::1])
    assert ok.flags["C_CONTIGUOUS"] and masks.check_activations(np.ones((1, 2, 2), dtype=np.float32)).shape == (1, 2, 2)
    act, scores = _combine_job(4, 7, 2)
    for args in ((act, scores[:3]), (act[:, :, :6], scores), (act, scores[:, :0]), (act[0], scores), (np.zeros((4, 17, 17), np.float32), scores)):
        with pytest.raises(ValueError):
            masks.cam_combine(*args)
    with pytest.raises(ValueError):
        masks.cam_combine(act, scores, low0=np.zeros((3, 7, 7), np.float32))
    for g in (1, 17, 2.5, True):
        with pytest.raises(ValueError):
            masks.cam_axis(g)
    with pytest.raises(ValueError):
        masks.cam_upsample(np.zeros((3, 7, 6), np.float32))
