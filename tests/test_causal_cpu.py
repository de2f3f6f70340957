"""CPU-side checks of the deletion / insertion curves (csrc/mpx_rankmask.h): the two C-ABI entries exist and are bound, and the numpy
restatements the device is held to (masks.saliency_rank, curve_thresholds, rank_masks_apply, gaussian_taps, blur_fill, curve_auc) have the
properties the device tests lean on; masks.blur_fill sits within the bound derived from its written order (causal_ref) of torch's own
conv2d in fp64.  No GPU anywhere in this file."""
import os
import re

import numpy as np
import pytest

from network_interpretation_imagenet_amd import _lib, masks
import causal_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mpx_rank_apply", "mpx_blur_fill")
HW = causal_ref.HW


def test_entries_exported_and_bound(mpx_lib):
    blob = open(_lib.LIB_PATH, "rb").read()
    header = open(os.path.join(ROOT, "include", "mpx.h")).read()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and getattr(mpx_lib, name) is not None and name.encode() in blob, name
        assert re.search(r"^int %s\(mpx_engine\* h," % name, header, re.M), name
    assert len(_lib.SIGNATURES["mpx_rank_apply"][1]) == 13 and len(_lib.SIGNATURES["mpx_blur_fill"][1]) == 9
    kernel = open(os.path.join(ROOT, "network_interpretation_imagenet_amd", "csrc", "mpx_rankmask.h")).read()
    stage = open(os.path.join(ROOT, "network_interpretation_imagenet_amd", "csrc", "mpx_stage.h")).read()
    assert "STAGE_MT" in kernel and int(re.search(r"constexpr int STAGE_MT = (\d+);", stage).group(1)) == _lib.RANKMASK_TILE == _lib.SOFTMASK_TILE
    assert int(re.search(r"constexpr int BF_KMAX = (\d+);", kernel).group(1)) == _lib.BLUR_KLEN_MAX == masks.BLUR_KLEN_MAX


# ---- saliency_rank ----------------------------------------------------------------------------------------------------------------
def test_saliency_rank_is_a_permutation_by_falling_saliency():
    sal = np.random.default_rng(1).standard_normal((224, 224)).astype(np.float32)
    rank = masks.saliency_rank(sal)
    assert rank.dtype == np.int32 and rank.shape == (224, 224)
    assert (np.sort(rank.ravel()) == np.arange(HW)).all()
    by_rank = np.empty(HW, dtype=np.float32)
    by_rank[rank.ravel()] = sal.ravel()
    assert (np.diff(by_rank) <= 0).all() and rank.ravel()[np.argmax(sal)] == 0


def test_saliency_rank_ties_go_to_raster_order():
    sal = causal_ref.superpixel_saliency()
    rank = masks.saliency_rank(sal)
    assert (rank == causal_ref.tied_rank_reference(sal)).all()
    flat, r = sal.ravel(), rank.ravel()
    for v in np.unique(flat):
        at = np.flatnonzero(flat == v)                  # rising pixel index ...
        assert (np.diff(r[at]) == 1).all()              # ... takes consecutive rising ranks
    assert (masks.saliency_rank(np.zeros((224, 224), np.float32)).ravel() == np.arange(HW)).all()


def test_saliency_rank_signed_zeros_are_tied():
    sal = np.zeros((224, 224), dtype=np.float32)
    sal.ravel()[::2] = -0.0
    sal[5, 7] = 1.0
    rank = masks.saliency_rank(sal).ravel()
    p = 5 * 224 + 7
    rest = np.delete(np.arange(HW), p)
    assert rank[p] == 0 and (rank[rest] == np.arange(1, HW)).all()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_saliency_rank_refuses_non_finite(bad):
    sal = np.zeros((224, 224), dtype=np.float32)
    sal[100, 3] = bad
    with pytest.raises(ValueError):
        masks.saliency_rank(sal)
    with pytest.raises(ValueError):
        masks.saliency_rank(np.zeros((224, 223), np.float32))


# ---- curve_thresholds -------------------------------------------------------------------------------------------------------------
def test_curve_thresholds():
    t = masks.curve_thresholds(224 * 8)
    assert t.dtype == np.int32 and t.shape == (29,) and t[0] == 0 and t[-1] == HW and (np.diff(t) == 1792).all()
    assert (t == masks.curve_thresholds(masks.CURVE_STEP)).all()
    t = masks.curve_thresholds(20000)                   # does not divide 50176: the last step is short
    assert t.tolist() == [0, 20000, 40000, HW]
    assert masks.curve_thresholds(HW).tolist() == [0, HW]
    assert masks.curve_thresholds(HW + 5).tolist() == [0, HW]
    assert masks.curve_thresholds(3, hw=7).tolist() == [0, 3, 6, 7]
    for bad in (0, -1792):
        with pytest.raises(ValueError):
            masks.curve_thresholds(bad)


# ---- rank_masks_apply -------------------------------------------------------------------------------------------------------------
def test_rank_masks_apply_rows():
    x, fill = causal_ref.noise_chw(2), causal_ref.noise_chw(3)
    rank = masks.saliency_rank(causal_ref.superpixel_saliency())
    thresh = masks.curve_thresholds(224 * 56)           # 5 rows
    dele = masks.rank_masks_apply(x, rank, thresh, fill, keep_top=False)
    ins = masks.rank_masks_apply(x, rank, thresh, fill, keep_top=True)
    assert dele.dtype == np.float32 and dele.shape == (5, 3, 224, 224) == ins.shape
    bits = lambda a: np.asarray(a).view(np.int32)
    from_x = bits(dele) == bits(x)[None]
    assert not (bits(x) == bits(fill)).any()            # so that `from_x` says which source a pixel came from
    # deletion rows are nested: what row i replaced stays replaced in row i + 1, and exactly thresh[i] pixels are replaced
    assert (from_x[1:] <= from_x[:-1]).all()
    assert (np.logical_not(from_x).sum(axis=(2, 3)) == thresh[:, None]).all()
    # insertion row i and deletion row i partition the pixels between the two sources
    assert ((bits(ins) == bits(x)[None]) != from_x).all()
    assert ((bits(ins) == bits(fill)[None]) == from_x).all()
    # the ends are the pure images
    assert (bits(dele[0]) == bits(x)).all() and (bits(dele[-1]) == bits(fill)).all()
    assert (bits(ins[0]) == bits(fill)).all() and (bits(ins[-1]) == bits(x)).all()


def test_rank_masks_apply_without_fill_is_the_binary_masks_removed_pixel():
    x = causal_ref.noise_chw(2)
    rank = masks.saliency_rank(causal_ref.superpixel_saliency())
    thresh = np.array([0, 1, 25000, HW], dtype=np.int32)
    got = masks.rank_masks_apply(x, rank, thresh, None, keep_top=False)
    keep = (rank[None] >= thresh[:, None, None]).astype(np.float32)
    want = x[None] * keep[:, None]                      # K0's x * mask, -0.0 under a removed negative pixel
    assert (got.view(np.int32) == want.view(np.int32)).all()
    assert (got[-1].view(np.int32) == np.int32(-2 ** 31)).any()
    with pytest.raises(ValueError):
        masks.rank_masks_apply(x, rank.astype(np.int64), thresh)
    with pytest.raises(ValueError):
        masks.rank_masks_apply(x, rank, thresh, fill=x[:2])


# ---- curve_auc --------------------------------------------------------------------------------------------------------------------
def test_curve_auc_known_answers():
    assert masks.curve_auc(np.full(29, 0.75, np.float32)) == 0.75
    assert masks.curve_auc(np.linspace(0.0, 1.0, 29)) == pytest.approx(0.5, abs=1e-15)
    assert masks.curve_auc([0.25, 0.75]) == 0.5
    assert masks.curve_auc([1.0, 0.0, 0.0]) == 0.25
    with pytest.raises(ValueError):
        masks.curve_auc([1.0])


# ---- taps and blur ----------------------------------------------------------------------------------------------------------------
def test_gaussian_taps():
    t = masks.gaussian_taps()
    assert t.dtype == np.float32 and t.shape == (11,) and (t == t[::-1]).all() and t.argmax() == 5
    d = np.arange(11, dtype=np.float64) - 5
    g = np.exp(-d * d / 50.0)
    assert (t == (g / g.sum()).astype(np.float32)).all()
    assert abs(float(t.astype(np.float64).sum()) - 1.0) <= 11 * 2.0 ** -25
    assert masks.gaussian_taps(1, 2.0).tolist() == [1.0]
    for klen, sigma in ((0, 5.0), (10, 5.0), (33, 5.0), (11, 0.0)):
        with pytest.raises(ValueError):
            masks.gaussian_taps(klen, sigma)


def test_blur_fill_one_tap_is_the_identity():
    x = causal_ref.noise_chw(4)
    x[0, 0, 0] = -0.0
    got = masks.blur_fill(x, np.array([1.0], np.float32))
    x[0, 0, 0] = 0.0                                    # fl(+0.0 + fl(1 * -0.0)) = +0.0: the sum starts from +0.0
    assert (got.view(np.int32) == x.view(np.int32)).all()


def test_blur_fill_is_a_correlation():
    """An impulse at (10, 20) under the taps [0.5, 0.25, 0.125]: out[y][x] = t[y' - y + 1] t[x' - x + 1], so the LAST tap lands on the pixel
    before the impulse -- a convolution would put the first one there."""
    x = np.zeros((3, 224, 224), dtype=np.float32)
    x[:, 10, 20] = 1.0
    got = masks.blur_fill(x, causal_ref.ASYM_TAPS)
    t = causal_ref.ASYM_TAPS
    want = np.outer(t[::-1], t[::-1])                   # rows y = 9, 10, 11; columns x = 19, 20, 21
    assert (got[:, 9:12, 19:22] == want[None]).all()
    got[:, 9:12, 19:22] = 0
    assert not got.any()
    # the corner: the taps that fall outside the image are skipped, not wrapped
    x[:] = 0
    x[:, 0, 0] = 1.0
    got = masks.blur_fill(x, t)
    assert (got[:, :2, :2] == np.outer(t[1::-1], t[1::-1])[None]).all() and not got[:, 2:].any() and not got[:, :, 2:].any()
    for bad in (np.ones(2, np.float32), np.ones(33, np.float32), np.ones(3, np.float64), np.ones((3, 1), np.float32)):
        with pytest.raises(ValueError):
            masks.blur_fill(x, bad)


@pytest.mark.parametrize("klen", causal_ref.KLEN_CASES)
def test_blur_fill_within_derived_bound_of_fp64_conv2d(klen):
    """Against torch.nn.functional.conv2d in fp64 with the outer-product kernel and padding r, every element within
    causal_ref.blur_bound (2 K u (1 + 2 K u) B).  Measured maxima: 0 at klen 1, 1.7e-07 at 3, 6.6e-08 at 11, 6.3e-08 at 31; the
    largest error / bound of an element is 0.44, 0.07 and 0.02 -- a worst-case bound over 2 K roundings loosens as K grows."""
    x, taps = causal_ref.noise_chw(5), causal_ref.taps_for(klen)
    got = masks.blur_fill(x, taps)
    assert got.dtype == np.float32 and got.shape == (3, 224, 224)
    err = np.abs(got.astype(np.float64) - causal_ref.conv2d_64(x, taps))
    bound = causal_ref.blur_bound(x, taps)
    print("klen=%d max |blur_fill - fp64 conv2d| = %.3e, max bound %.3e, max err / bound %.3f"
          % (klen, err.max(), bound.max(), float((err / bound).max())))
    assert (err <= bound).all()
