"""CPU-side checks of the Sobol total-order path (csrc/mpx_softmask.h DesignWeights; Fel et al., NeurIPS 2021): the new entry in the header
and the ctypes table, the design's rows and cells against literal loops, the quasi-Monte-Carlo design, Jansen's estimator against known
answers, and the refusals of the host checks.  No GPU anywhere in this file."""
import os
import re
import warnings

import numpy as np
import pytest

from network_interpretation_imagenet_amd import _lib, masks
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine
import sobol_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG = 224


# ------------------------------------------------------------------------------------------------------------------------------------
# the entry
# ------------------------------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_exported_and_bound(mpx_lib):
    """mpx_sobol_apply is declared, exported and bound with as many arguments as the header declares: the 15 of the signature (the handle,
    two image pointers, A, B, N, d, row0, M, the fill, mean, std, slot0, out_f32, the stream)."""
    header = open(os.path.join(ROOT, "include", "mpx.h")).read()
    decl = re.search(r"^int mpx_sobol_apply\((.*?)\);", header, re.M | re.S).group(1)
    params = [p.strip() for p in decl.replace("\n", " ").split(",")]
    assert params[0] == "mpx_engine* h" and params[-1] == "void* stream" and len(params) == 15
    assert [p.split()[-1].split("[")[0].lstrip("*") for p in params] == ["h", "img_u8_hwc", "img_f32_chw", "A", "B", "N", "d", "row0", "M",
                                                                         "fill_f32_chw", "mean", "std", "slot0", "out_f32_nchw", "stream"]
    res, args = _lib.SIGNATURES["mpx_sobol_apply"]
    assert len(args) == len(params)
    assert getattr(mpx_lib, "mpx_sobol_apply").argtypes == args
    block = header[header.index("the rows of a Sobol total-order design"):header.index("int mpx_sobol_apply(")]
    assert "extends: mpx_softmask_apply" in block
    lo, hi = (int(re.search(r"#define MPX_SOBOL_GRID_%s (\d+)" % n, header).group(1)) for n in ("MIN", "MAX"))
    assert (_lib.SOBOL_GRID_MIN, _lib.SOBOL_GRID_MAX) == (lo, hi) == (masks.SOBOL_GRID_MIN, masks.SOBOL_GRID_MAX) == (2, 32)
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "mpx_softmask.h")).read()
    assert "constexpr int SOBOL_GRID_MIN = %d;" % lo in src and "constexpr int SOBOL_GRID_MAX = %d;" % hi in src
    assert hi * hi <= _lib.SURROGATE_S_MAX          # mpx_segment_paint paints the d * d indices


# ------------------------------------------------------------------------------------------------------------------------------------
# rows and cells
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n", [(2, 2), (3, 4), (32, 2)])
def test_row_cells_equal_a_literal_double_loop(d, n):
    A, B = sobol_ref.design(d, n)
    D = d * d
    rows = masks.sobol_rows(n, d)
    assert rows == n * (D + 1)
    want = sobol_ref.row_cells_loop(A, B)
    got = masks.sobol_row_cells(A, B, 0, rows)
    assert got.dtype == np.float32 and got.shape == (rows, D)
    assert (got.view(np.int32) == want.view(np.int32)).all()
    for row0, m in ((0, 0), (n - 1, 3), (rows - 1, 1), (n + D - 1, 2), (1, rows - 1)):          # any window of rows is that window
        assert (masks.sobol_row_cells(A, B, row0, m).view(np.int32) == want[row0:row0 + m].view(np.int32)).all()
    for row0, m in ((-1, 2), (0, rows + 1), (rows, 1), (0, -1)):
        with pytest.raises(ValueError):
            masks.sobol_row_cells(A, B, row0, m)


def test_cell_map_sizes():
    c3 = masks.sobol_cell_map(3)
    assert c3.dtype == np.int32 and c3.shape == (IMG, IMG)
    assert np.bincount(c3[:, 0] // 3).tolist() == [75, 75, 74] and np.bincount(c3[0, :]).tolist() == [75, 75, 74]
    c32 = masks.sobol_cell_map(32)
    assert (np.bincount(c32[:, 0] // 32) == 7).all() and (np.bincount(c32[0, :]) == 7).all()
    assert (np.bincount(c32.ravel(), minlength=1024) == 49).all()
    for d in (2, 3, 7, 13, 32):
        c = masks.sobol_cell_map(d)
        assert c.min() == 0 and c.max() == d * d - 1 and len(np.unique(c)) == d * d
        y, x = np.divmod(np.arange(IMG * IMG), IMG)
        assert (c.ravel() == ((y * d) // IMG) * d + (x * d) // IMG).all()


@pytest.mark.parametrize("d,n,row0,m", [(3, 4, 0, 40), (3, 4, 2, 33), (2, 2, 2, 8), (32, 2, 1023, 8), (13, 3, 100, 7)])
def test_weights_are_the_cells_gathered(d, n, row0, m):
    A, B = sobol_ref.design(d, n)
    w = masks.sobol_weights(A, B, d, row0, m)
    assert w.dtype == np.float32 and w.shape == (m, IMG, IMG) and w.flags["C_CONTIGUOUS"]
    want = masks.sobol_row_cells(A, B, row0, m)[:, masks.sobol_cell_map(d)]
    assert (w.view(np.int32) == want.view(np.int32)).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# the design
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n", [(2, 2), (8, 32), (3, 5), (32, 4)])
def test_design_shape_range_and_seed(d, n):
    A, B = masks.sobol_design(n, d, seed=3)
    for t in (A, B):
        assert t.dtype == np.float32 and t.shape == (n, d * d) and t.flags["C_CONTIGUOUS"]
        assert np.isfinite(t).all() and t.min() >= 0.0 and t.max() <= 1.0
    A2, B2 = masks.sobol_design(n, d, seed=3)
    assert (A == A2).all() and (B == B2).all()
    A3, _B3 = masks.sobol_design(n, d, seed=4)
    assert (A != A3).any() and (A != B).any()
    assert masks.check_sobol(A, B, d)[0].shape == A.shape


# ------------------------------------------------------------------------------------------------------------------------------------
# the estimator
# ------------------------------------------------------------------------------------------------------------------------------------
def _scores_of(f, A, B):
    """f32[R, 1]: f evaluated in fp64 on every row's cells, rounded to fp32 as a class score is."""
    cells = masks.sobol_row_cells(A, B, 0, masks.sobol_rows(A.shape[0], int(round(A.shape[1] ** 0.5)))).astype(np.float64)
    return f(cells).astype(np.float32)[:, None]


def test_a_score_of_one_cell_gives_exact_zeros_elsewhere():
    A, B = masks.sobol_design(16, 3, seed=1)
    st = masks.sobol_total_order(_scores_of(lambda c: np.sin(3.0 * c[:, 0]), A, B), 16)
    assert st.dtype == np.float64 and st.shape == (1, 9)
    assert st[0, 0] > 0.5 and (st[0, 1:] == 0.0).all()


def test_a_constant_score_gives_zeros_without_a_warning():
    A, B = masks.sobol_design(8, 2, seed=0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        st = masks.sobol_total_order(np.full((8 * 5, 3), 0.25, dtype=np.float32), 8)
    assert st.shape == (3, 4) and (st == 0.0).all() and not np.isnan(st).any()
    mixed = np.concatenate([np.full((40, 1), 0.25, np.float32), _scores_of(lambda c: c[:, 1], A, B)], axis=1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        st = masks.sobol_total_order(mixed, 8)
    assert (st[0] == 0.0).all() and st[1, 1] > 0 and (st[1, [0, 2, 3]] == 0.0).all()


def test_a_product_of_two_cells():
    """f = x0 * x1: the cells 2.. never enter (ST exactly 0); ST0 = ST1 = 4/7 analytically (V = 1/9 - 1/16 = 7/144, E[Var(f | x1)] =
    E[x1^2] / 12 = 1/36).  Only the sign is asserted of those two: their error is the sampling error of 64 designs."""
    A, B = masks.sobol_design(64, 3, seed=2)
    st = masks.sobol_total_order(_scores_of(lambda c: c[:, 0] * c[:, 1], A, B), 64)[0]
    print("ST0 %.4f ST1 %.4f (4/7 = %.4f)" % (st[0], st[1], 4 / 7))
    assert st[0] > 0 and st[1] > 0 and (st[2:] == 0.0).all()


def test_a_linear_score_converges_to_its_variance_shares():
    """f = sum (i + 1) x_i at D = 9, N = 1024, seeds 0..7: ST_i = (i + 1)^2 / sum (i + 1)^2 up to the sampling error of the design.  The
    bound 0.005 is ten times the 0.0005 measured with these exact inputs: the error is a sampling error, not a rounding error."""
    want = np.arange(1, 10) ** 2 / float((np.arange(1, 10) ** 2).sum())
    worst = 0.0
    for seed in range(8):
        A, B = masks.sobol_design(1024, 3, seed=seed)
        st = masks.sobol_total_order(_scores_of(lambda c: (c * np.arange(1, 10)).sum(axis=1), A, B), 1024)[0]
        worst = max(worst, float(np.abs(st - want).max()))
    print("max |ST_i - (i+1)^2 / sum| over seeds 0..7: %.6f" % worst)
    assert worst <= 0.005


def test_estimator_against_a_loop_restatement_and_column_independence():
    rng = np.random.default_rng(5)
    for n, D, K in ((2, 4, 1), (5, 9, 3), (32, 64, 5)):
        scores = rng.random((n * (D + 1), K), dtype=np.float32)
        st = masks.sobol_total_order(scores, n)
        assert st.shape == (K, D) and st.dtype == np.float64
        want = sobol_ref.total_order_loop(scores, n)
        assert (np.abs(st - want) <= 1e-12 * np.abs(want)).all()
        for k in range(K):
            one = masks.sobol_total_order(scores[:, k:k + 1], n)
            assert (one[0].view(np.int64) == st[k].view(np.int64)).all()
            assert (masks.sobol_total_order(np.ascontiguousarray(scores[:, k]), n)[0].view(np.int64) == st[k].view(np.int64)).all()
    for bad_scores, n in ((np.zeros((10, 1), np.float32), 3), (np.zeros((10, 1), np.float32), 1), (np.zeros((4, 1), np.float32), 4),
                          (np.zeros((2, 5, 1), np.float32), 2)):
        with pytest.raises(ValueError):
            masks.sobol_total_order(bad_scores, n)


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals, before anything touches a device
# ------------------------------------------------------------------------------------------------------------------------------------
def _bare_engine(small=False):
    """An engine object with no device behind it: the drivers check their arguments before they touch one."""
    e = object.__new__(MaskedForwardEngine)
    e._h = None
    e.small = small
    e.arch = "mnist_net" if small else "resnet18"
    return e


def _bad_designs():
    A, B = sobol_ref.design(3, 4)
    yield "d = 1", np.zeros((4, 1), np.float32), np.zeros((4, 1), np.float32), 1
    yield "d = 33", np.zeros((2, 33 * 33), np.float32), np.zeros((2, 33 * 33), np.float32), 33
    yield "N = 1", A[:1], B[:1], 3
    yield "f64", A.astype(np.float64), B, 3
    yield "B f64", A, B.astype(np.float64), 3
    yield "wrong D", A[:, :8], B[:, :8], 3
    yield "A and B differ in N", A, B[:3], 3
    yield "3-D", A[None], B[None], 3
    yield "grid does not match", A, B, 4
    hot = A.copy()
    hot[2, 5] = 1.5
    yield "1.5", hot, B, 3
    neg = B.copy()
    neg[1, 1] = -0.25
    yield "negative", A, neg, 3
    nan = B.copy()
    nan[3, 8] = np.nan
    yield "NaN", A, nan, 3


def test_check_sobol_refuses():
    A, B = sobol_ref.design(3, 4)
    a, b = masks.check_sobol(A, B, 3)
    assert (a == A).all() and (b == B).all()
    for why, bad_a, bad_b, d in _bad_designs():
        with pytest.raises(ValueError):
            masks.check_sobol(bad_a, bad_b, d)
            pytest.fail("accepted: " + why)
    for n, d in ((1, 3), (4, 1), (4, 33), (2.5, 3)):
        with pytest.raises(ValueError):
            masks.sobol_design(n, d)
        with pytest.raises(ValueError):
            masks.sobol_rows(n, d)
    for d in (1, 33, 0):
        with pytest.raises(ValueError):
            masks.sobol_cell_map(d)


def test_drivers_refuse_before_the_device():
    img = np.zeros((IMG, IMG, 3), np.uint8)
    A, B = sobol_ref.design(3, 4)
    e = _bare_engine()
    for _why, bad_a, bad_b, d in _bad_designs():
        with pytest.raises(ValueError):
            e.score_sobol(img, bad_a, bad_b, d, 1)
        with pytest.raises(ValueError):
            e.score_sobol_classes(img, bad_a, bad_b, d, [1, 2])
    for fill in (np.zeros((3, IMG, 223), np.float32), np.zeros((IMG, IMG, 3), np.float32), np.zeros((3, IMG, IMG), np.float64), "mean"):
        with pytest.raises(ValueError):
            e.score_sobol(img, A, B, 3, 1, fill=fill)
        with pytest.raises(ValueError):
            e.score_sobol_classes(img, A, B, 3, [1], fill=fill)
        with pytest.raises(ValueError):
            e.sobol_attribution(img, classes=[1], grid=3, n_design=4, fill=fill)
    for kw in (dict(grid=1), dict(grid=33), dict(n_design=1), dict(classes=[1], top=2), dict(classes=[1000]), dict(classes=[]), dict(top=0)):
        with pytest.raises(ValueError):
            e.sobol_attribution(img, **({"classes": [1], "grid": 3, "n_design": 4} | kw))
    with pytest.raises(ValueError):
        e.score_sobol(img, A, B, 3, 1000)
    with pytest.raises(ValueError):
        e.score_sobol_classes(img, A, B, 3, [-1])
    small = _bare_engine(small=True)
    for call in (lambda: small.score_sobol(img, A, B, 3, 1), lambda: small.score_sobol_classes(img, A, B, 3, [1]),
                 lambda: small.sobol_attribution(img, classes=[1], grid=3, n_design=4)):
        with pytest.raises(ValueError):
            call()
