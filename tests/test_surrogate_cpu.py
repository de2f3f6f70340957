"""CPU-side checks of the linear-surrogate path (csrc/mpx_surrogate.h; LIME and KernelSHAP on superpixels): the two new entries in the
header, the ctypes table and the built library; the samplers and weights of masks.py; the two fp64 solves against sklearn's Ridge and
against brute-force Shapley values; the numpy restatement of the moment sums against an extended-precision matrix product; and the recorded
reason why the sums are fp64.  No GPU anywhere in this file.  Every bound is computed in the test that uses it, from the roundings named
in its docstring."""
import itertools
import math
import os

import numpy as np
import pytest

from network_interpretation_imagenet_amd import _lib, masks
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine

NEW_ENTRIES = ("mpx_surrogate_accumulate", "mpx_segment_paint")
U32, U64 = 2.0 ** -24, 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def ztilde(onoff):
    return np.concatenate([np.ones((onoff.shape[0], 1)), (onoff != 0).astype(np.float64)], axis=1)


def zero_moments(s, k):
    return np.zeros((s + 1, s + 1)), np.zeros((s + 1, k))


# ------------------------------------------------------------------------------------------------------------------------------------
# the entries
# ------------------------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_exported_and_bound(mpx_lib):
    header = open(os.path.join(ROOT, "include", "mpx.h")).read()
    for name in NEW_ENTRIES:
        assert "int %s(mpx_engine* h" % name in header
        assert name in _lib.SIGNATURES
        assert getattr(mpx_lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "extends: mpx_heatmap_accumulate" in header[header.index("a linear surrogate over on/off superpixel rows"):]
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "mpx_surrogate.h")).read()
    assert "constexpr int SUR_S_MAX = %d;" % _lib.SURROGATE_S_MAX in src          # the Python copies of the kernel's limit
    assert masks.SURROGATE_S_MAX == _lib.SURROGATE_S_MAX


def _bare_engine(small=False):
    """An engine object with no device behind it: lime and kernel_shap check their arguments before they touch one."""
    e = object.__new__(MaskedForwardEngine)
    e._h = None
    e.small = small
    e.arch = "mnist_net" if small else "resnet18"
    return e


def test_python_methods_refuse_before_the_device():
    img = np.zeros((224, 224, 3), np.uint8)
    seg = np.repeat(np.repeat(np.arange(16, dtype=np.int32).reshape(4, 4), 56, axis=0), 56, axis=1)        # S = 16
    one = np.zeros((224, 224), np.int32)                                                                    # S = 1
    small = _bare_engine(small=True)
    for call in (lambda: small.lime(img, seg, classes=[1]), lambda: small.kernel_shap(img, seg, classes=[1]),
                 lambda: small.score_masks_classes(img, seg, np.ones((2, 16), np.uint8), [1])):
        with pytest.raises(ValueError):
            call()
    e = _bare_engine()
    for kw in (dict(n_samples=14), dict(n_samples=33), dict(classes=[1, 2], top=3), dict(classes=[1000])):
        with pytest.raises(ValueError):
            e.kernel_shap(img, seg, **({"classes": [1]} | kw))
    with pytest.raises(ValueError):
        e.kernel_shap(img, one, classes=[1], n_samples=4)                                                   # S < 2
    for kw in (dict(n_samples=0), dict(lam=-1.0), dict(kernel_width=0.0), dict(classes=[]), dict(top=0)):
        with pytest.raises(ValueError):
            e.lime(img, seg, **({"classes": [1]} | kw))


# ------------------------------------------------------------------------------------------------------------------------------------
# samplers and weights
# ------------------------------------------------------------------------------------------------------------------------------------
def test_lime_onoff_is_seeded_and_starts_with_the_whole_image():
    a, b, c = masks.lime_onoff(50, 33, seed=4), masks.lime_onoff(50, 33, seed=4), masks.lime_onoff(50, 33, seed=5)
    assert a.dtype == np.uint8 and a.shape == (50, 33) and (a == b).all() and (a != c).any()
    assert (a[0] == 1).all() and set(np.unique(a)) == {0, 1}
    assert 0.4 < a[1:].mean() < 0.6
    with pytest.raises(ValueError):
        masks.lime_onoff(0, 5)


def test_shap_onoff_pairs_and_sizes():
    s = 10
    a, b = masks.shap_onoff(40000, s, seed=2), masks.shap_onoff(40000, s, seed=2)
    assert a.dtype == np.uint8 and a.shape == (40000, s) and (a == b).all() and (a != masks.shap_onoff(40000, s, seed=3)).any()
    assert (a[0::2] + a[1::2] == 1).all()                       # complementary pairs
    sizes = a[0::2].sum(axis=1)
    assert sizes.min() >= 1 and sizes.max() <= s - 1
    n = sizes.size                                              # 20 000 draws of the size
    p = masks.shap_size_pmf(s)
    assert abs(p.sum() - 1) < 1e-15 and np.allclose(p * np.arange(1, s) * (s - np.arange(1, s)), p[0] * (s - 1))
    count = np.bincount(sizes, minlength=s)[1:]
    sd = np.sqrt(n * p * (1 - p))
    assert (np.abs(count - n * p) <= 5 * sd).all(), (count, n * p, sd)
    # every superpixel is in the first row of a pair about half the time (the kernel is symmetric in k and S - k)
    assert (np.abs(a[0::2].mean(axis=0) - 0.5) < 5 * 0.5 / math.sqrt(n)).all()
    for bad in ((3, 5), (4, 1), (-2, 5)):
        with pytest.raises(ValueError):
            masks.shap_onoff(*bad)
    assert masks.shap_onoff(0, 5).shape == (0, 5)


def test_shapley_kernel_enumeration():
    onoff, w = masks.shapley_kernel_onoff(5)
    assert onoff.shape == (30, 5) and w.dtype == np.float32 and len({tuple(r) for r in onoff}) == 30
    k = onoff.sum(axis=1)
    assert k.min() == 1 and k.max() == 4
    want = np.array([4 / (math.comb(5, int(v)) * v * (5 - v)) for v in k])
    assert (w == want.astype(np.float32)).all()
    for bad in (1, 13):
        with pytest.raises(ValueError):
            masks.shapley_kernel_onoff(bad)


def test_lime_weights():
    s = 16
    onoff = np.zeros((s + 1, s), np.uint8)
    for k in range(s + 1):
        onoff[k, :k] = 7                                        # k superpixels on, by a byte other than 1
    w = masks.lime_weights(onoff)
    assert w.dtype == np.float32 and w[s] == 1.0 and w[0] == np.float32(math.exp(-8.0))
    assert (np.diff(w.astype(np.float64)) > 0).all()           # monotone in k
    d = 1 - math.sqrt(4 / 16)
    assert w[4] == np.float32(math.sqrt(math.exp(-d * d / 0.0625)))
    assert masks.lime_weights(onoff, kernel_width=0.5)[0] == np.float32(math.exp(-2.0))
    with pytest.raises(ValueError):
        masks.lime_weights(onoff.astype(np.int32))


# ------------------------------------------------------------------------------------------------------------------------------------
# the moment sums
# ------------------------------------------------------------------------------------------------------------------------------------
def _job(m, s, k, seed):
    rng = np.random.default_rng(seed)
    onoff = masks.lime_onoff(m, s, seed)
    return onoff, masks.lime_weights(onoff), rng.uniform(0, 1, size=(m, k)).astype(np.float32), rng


def _exact_moments(onoff, w, sc):
    """Z~^T W Z~ and Z~^T W Y in x87 extended precision (64 significant bits: its own error is 2^-11 of an fp64 rounding per term)."""
    z = ztilde(onoff).astype(np.longdouble)
    zw = z * w.astype(np.longdouble)[:, None]
    return zw.T @ z, zw.T @ sc.astype(np.longdouble)


def test_surrogate_sums_against_the_matrix_product():
    """M sequential fp64 additions of exact terms err by at most (M - 1) 2^-53 sum|terms| (each partial sum is bounded by sum|terms|);
    the reference product is taken in extended precision, whose own error fits in the remaining 2^-53 sum|terms|.  So per element
    |got - product| <= M 2^-53 sum|terms|, with sum|terms| the same product over the absolute values."""
    m, s, k = 257, 33, 5
    onoff, w, sc, rng = _job(m, s, k, 3)
    sc -= 0.5                                                   # both signs: cancellation in B
    a0, b0 = rng.standard_normal((s + 1, s + 1)), rng.standard_normal((s + 1, k))
    A, B = masks.surrogate_sums(a0, b0, onoff, w, sc)
    assert A.dtype == np.float64 and B.dtype == np.float64 and (a0 != A).any()         # not accumulated in place
    ea, eb = _exact_moments(onoff, w, sc)
    ta, tb = _exact_moments(onoff, w, np.abs(sc))
    da = np.abs((A - a0).astype(np.longdouble) - ea).astype(np.float64)
    db = np.abs((B - b0).astype(np.longdouble) - eb).astype(np.float64)
    # a0 / b0 are part of every partial sum: they enter the bound as one more term
    bound_a = (m + 1) * U64 * (np.abs(a0) + ta.astype(np.float64))
    bound_b = (m + 1) * U64 * (np.abs(b0) + tb.astype(np.float64))
    print("sums: max dA / bound %.3f, max dB / bound %.3f" % ((da / bound_a).max(), (db / bound_b).max()))
    assert (da <= bound_a).all() and (db <= bound_b).all()
    A0, _ = masks.surrogate_sums(*zero_moments(s, k), onoff, w, sc)
    assert (A0 == A0.T).all() and A0[0, 0] == np.cumsum(w.astype(np.float64))[-1]     # both triangles, and the sequential sum of the weights


def test_surrogate_sums_cut_into_calls_bytes_and_nan():
    m, s, k = 65, 7, 3
    onoff, w, sc, rng = _job(m, s, k, 8)
    a0, b0 = rng.standard_normal((s + 1, s + 1)), rng.standard_normal((s + 1, k))
    A, B = masks.surrogate_sums(a0, b0, onoff, w, sc)
    a, b = a0, b0
    for lo, hi in ((0, 1), (1, 30), (30, 65)):
        a, b = masks.surrogate_sums(a, b, onoff[lo:hi], w[lo:hi], sc[lo:hi])
    assert (bits64(a) == bits64(A)).all() and (bits64(b) == bits64(B)).all()
    other = onoff.copy()
    other[onoff != 0] = rng.choice(np.array([2, 128, 255], np.uint8), size=int((onoff != 0).sum()))
    a, b = masks.surrogate_sums(a0, b0, other, w, sc)
    assert (bits64(a) == bits64(A)).all() and (bits64(b) == bits64(B)).all()
    # a NaN weight and score on an all-off row reach only row 0 / column 0 of that row's z~ = (1, 0, .., 0): A[0][0] and B[0][:]
    o2, w2, s2 = onoff.copy(), w.copy(), sc.copy()
    o2[9] = 0
    base_a, base_b = masks.surrogate_sums(a0, b0, o2, w2, s2)
    s2[9, 1] = np.nan
    a, b = masks.surrogate_sums(a0, b0, o2, w2, s2)
    assert (bits64(a) == bits64(base_a)).all()
    hit = np.isnan(b)
    assert hit[0, 1] and hit.sum() == 1 and (bits64(b)[~hit] == bits64(base_b)[~hit]).all()
    # a NaN score on a row with superpixels {2, 5} on: column 1 of rows 0, 3 and 6, nothing else
    o3, s3 = onoff.copy(), sc.copy()
    o3[11] = 0
    o3[11, [2, 5]] = 1
    base_a, base_b = masks.surrogate_sums(a0, b0, o3, w, s3)
    s3[11, 1] = np.nan
    a, b = masks.surrogate_sums(a0, b0, o3, w, s3)
    hit = np.isnan(b)
    assert (bits64(a) == bits64(base_a)).all() and sorted(zip(*np.nonzero(hit))) == [(0, 1), (3, 1), (6, 1)]
    assert (bits64(b)[~hit] == bits64(base_b)[~hit]).all()
    with pytest.raises(ValueError):
        masks.surrogate_sums(a0, b0, onoff, w.astype(np.float64), sc)
    with pytest.raises(ValueError):
        masks.surrogate_sums(a0, b0[:, :2], onoff, w, sc)


def test_segment_paint():
    seg = np.array([[0, 3, 2], [5, -1, 1]], dtype=np.int32)
    value = np.array([[1, 2, 3, -4], [5, 6, 7, 8]], dtype=np.float32)
    got = masks.segment_paint(seg, value)
    assert got.dtype == np.float32 and got.shape == (2, 2, 3)
    assert (got[0] == np.array([[1, -4, 3], [0, 0, 2]], np.float32)).all() and (got[1] == np.array([[5, 8, 7], [0, 0, 6]])).all()
    assert not np.signbit(got[0, 1, 0])
    with pytest.raises(ValueError):
        masks.segment_paint(seg, value.astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------------------------
# the solves
# ------------------------------------------------------------------------------------------------------------------------------------
def test_lime_solve_against_sklearn_ridge():
    """Tolerance: 100 x the difference of sklearn's Ridge from an fp64 lstsq on the augmented rows (sqrt(w) z~ over sqrt(lam) e_j with a zero
    target), both measured here."""
    linear_model = pytest.importorskip("sklearn.linear_model")
    m, s, k, lam = 400, 40, 3, 1.0
    onoff, w, sc, _ = _job(m, s, k, 12)
    A, B = masks.surrogate_sums(*zero_moments(s, k), onoff, w, sc)
    c0, c = masks.lime_solve(A, B, lam)
    assert c0.shape == (k,) and c.shape == (k, s) and c0.dtype == np.float64 and c.dtype == np.float64
    w64, y = w.astype(np.float64), sc.astype(np.float64)
    ridge = linear_model.Ridge(alpha=lam, fit_intercept=True).fit((onoff != 0).astype(np.float64), y, sample_weight=w64)
    rows = np.concatenate([np.sqrt(w64)[:, None] * ztilde(onoff), math.sqrt(lam) * np.eye(s + 1)[1:]])
    beta = np.linalg.lstsq(rows, np.concatenate([np.sqrt(w64)[:, None] * y, np.zeros((s, k))]), rcond=None)[0]
    ref = max(np.abs(ridge.coef_ - beta[1:].T).max(), np.abs(ridge.intercept_ - beta[0]).max())
    got = max(np.abs(ridge.coef_ - c).max(), np.abs(ridge.intercept_ - c0).max())
    print("lime_solve: |ours - sklearn| %.3e, |sklearn - lstsq| %.3e" % (got, ref))
    assert got <= 100 * ref


def test_lime_solve_recovers_a_linear_set_function_without_a_penalty():
    """Coefficients that are multiples of 1/16 below 4: every score is exact in fp32, so only the fp64 solve rounds.  A backward-stable
    solve of an n x n system errs by about n 2^-53 cond(A) max|beta|; the weights' sums in A and B add M 2^-53 relative: the bound is
    (n + M) 2^-52 cond(A) max|beta|."""
    m, s = 300, 24
    rng = np.random.default_rng(5)
    onoff = masks.lime_onoff(m, s, 5)
    coef = rng.integers(-63, 64, size=(2, s)) / 16.0
    icpt = np.array([0.25, -1.5])
    sc = (icpt[None, :] + (onoff != 0).astype(np.float64) @ coef.T).astype(np.float32)
    assert (sc.astype(np.float64) == icpt[None, :] + onoff.astype(np.float64) @ coef.T).all()
    A, B = masks.surrogate_sums(*zero_moments(s, 2), onoff, masks.lime_weights(onoff), sc)
    c0, c = masks.lime_solve(A, B, lam=0.0)
    bound = (s + 1 + m) * 2.0 ** -52 * np.linalg.cond(A) * 4.0
    err = max(np.abs(c - coef).max(), np.abs(c0 - icpt).max())
    print("lime_solve, lam = 0: max error %.3e, bound %.3e" % (err, bound))
    assert err <= bound


def test_solves_refuse_singular_systems():
    s = 6
    onoff = masks.lime_onoff(4, s, 1)                           # 4 rows for 7 unknowns
    sc = np.ones((4, 1), np.float32)
    A, B = masks.surrogate_sums(*zero_moments(s, 1), onoff, np.ones(4, np.float32), sc)
    with pytest.raises(ValueError):
        masks.lime_solve(A, B, lam=0.0)
    masks.lime_solve(A, B, lam=1.0)                             # the penalty makes it regular
    dup = masks.lime_onoff(60, s, 2)
    dup[:, 1] = dup[:, 0]                                       # two dependent columns
    A, B = masks.surrogate_sums(*zero_moments(s, 1), dup, np.ones(60, np.float32), np.ones((60, 1), np.float32))
    with pytest.raises(ValueError):
        masks.lime_solve(A, B, lam=0.0)
    few = masks.shap_onoff(2, s, 0)                             # one pair for 5 unknowns
    A, B = masks.surrogate_sums(*zero_moments(s, 1), few, np.ones(2, np.float32), np.ones((2, 1), np.float32))
    with pytest.raises(ValueError):
        masks.shap_solve(A, B, [0.0], [1.0])
    with pytest.raises(ValueError):
        masks.shap_solve(np.eye(2), np.zeros((2, 1)), [0.0], [1.0])         # S = 1
    with pytest.raises(ValueError):
        masks.lime_solve(np.eye(3), np.zeros((4, 1)))


def _set_function(s):
    """A non-linear set function on {0, 1}^s with two output columns, in fp64."""
    a = np.arange(1, s + 1) * 0.3

    def f(z):
        z = np.asarray(z, dtype=np.float64)
        return np.array([math.tanh(z @ a / s) + 0.5 * z[0] * z[3] - 0.2 * z[1] * z[2] * z[s - 1], math.exp(-(z @ a) / s) + z[1] * z[2]])

    return f


def _brute_force_shapley(f, s):
    phi = np.zeros((2, s))
    for j in range(s):
        others = [i for i in range(s) if i != j]
        for k in range(s):
            c = math.factorial(k) * math.factorial(s - k - 1) / math.factorial(s)
            for sub in itertools.combinations(others, k):
                z = np.zeros(s)
                z[list(sub)] = 1
                without = f(z)
                z[j] = 1
                phi[:, j] += c * (f(z) - without)
    return phi


@pytest.mark.parametrize("s", [4, 6])
def test_shap_solve_gives_exact_shapley_values_on_the_full_enumeration(s):
    """With exact weights w and scores y the Shapley values phi solve G phi = b exactly (Lundberg & Lee, theorem 2).  The inputs here are
    rounded to fp32: w^ = w (1 + e), y^ = y + d, f0^ and f1^ likewise, |e| <= u, |d| <= u |y|, u = 2^-24.  With d_m = (z_mj - z_mL)_j,
    r_m = y_m - f0 - (f1 - f0) z_mL:  G = sum_m w_m d_m d_m^T,  b = sum_m w_m d_m r_m  and  sum_m w_m d_m (r_m - d_m^T phi) = 0, so
      phi^ - phi = G^^-1 sum_m d_m [ w^_m (r^_m - r_m) + (w^_m - w_m) (r_m - d_m^T phi) ],     |d_m|_inf <= 1,
      |phi^ - phi|_inf <= |G^^-1|_inf u sum_m w^_m ( |y_m| + 2 |f0| + |f1| + |r_m - d_m^T phi| ) (1 + u)        =: bound
    for the s - 1 free values; the eliminated one is (f1^ - f0^) - sum of them: (s - 1) bound + u (|f0| + |f1|).  The fp64 roundings of
    the sums and of the solve are 2^-29 of these and are covered by the factor 1.01.  sum(phi) = f1 - f0 holds to the fp64 rounding of
    that one subtraction and of the test's own sum: s 2^-52 sum|phi|."""
    f = _set_function(s)
    onoff, w = masks.shapley_kernel_onoff(s)
    y = np.array([f(r) for r in onoff])
    sc = y.astype(np.float32)
    f0, f1 = f(np.zeros(s)).astype(np.float32).astype(np.float64), f(np.ones(s)).astype(np.float32).astype(np.float64)
    A, B = masks.surrogate_sums(*zero_moments(s, 2), onoff, w, sc)
    phi = masks.shap_solve(A, B, f0, f1)
    want = _brute_force_shapley(f, s)
    assert phi.shape == (2, s) and phi.dtype == np.float64
    z = onoff.astype(np.float64)
    d = z[:, :s - 1] - z[:, s - 1:]
    g_inv = np.abs(np.linalg.inv(A[1:s, 1:s] - A[1:s, s:] - A[s:, 1:s] + A[s, s])).sum(axis=1).max()
    for k in range(2):
        r = y[:, k] - f0[k] - (f1[k] - f0[k]) * z[:, s - 1]
        res = np.abs(r - d @ want[k, :s - 1])
        bound = 1.01 * g_inv * U32 * (1 + U32) * float((w.astype(np.float64) * (np.abs(y[:, k]) + 2 * abs(f0[k]) + abs(f1[k]) + res)).sum())
        last = (s - 1) * bound + U32 * (abs(f0[k]) + abs(f1[k]))
        err = np.abs(phi[k] - want[k])
        print("shap_solve S=%d column %d: max error %.3e (bound %.3e), eliminated %.3e (bound %.3e)"
              % (s, k, err[:s - 1].max(), bound, err[s - 1], last))
        assert (err[:s - 1] <= bound).all() and err[s - 1] <= last
        assert abs(phi[k].sum() - (f1[k] - f0[k])) <= s * 2.0 ** -52 * np.abs(phi[k]).sum()


def test_shap_solve_recovers_a_linear_set_function_from_sampled_rows():
    """Coefficients that are multiples of 1/16: every score is exact in fp32 and the sampled rows carry weight 1, so only fp64 rounds:
    (n + M) 2^-52 cond(G) max|phi| as for lime_solve."""
    m, s = 200, 9
    coef = np.random.default_rng(9).integers(-63, 64, size=(2, s)) / 16.0
    icpt = np.array([0.5, -2.0])
    onoff = masks.shap_onoff(m, s, 4)
    sc = (icpt[None, :] + onoff.astype(np.float64) @ coef.T).astype(np.float32)
    A, B = masks.surrogate_sums(*zero_moments(s, 2), onoff, np.ones(m, np.float32), sc)
    phi = masks.shap_solve(A, B, icpt, icpt + coef.sum(axis=1))
    G = A[1:s, 1:s] - A[1:s, s:] - A[s:, 1:s] + A[s, s]
    bound = (s + m) * 2.0 ** -52 * np.linalg.cond(G) * 4.0
    err = np.abs(phi - coef).max()
    print("shap_solve, linear: max error %.3e, bound %.3e" % (err, s * bound))
    assert err <= s * bound                                     # the eliminated value sums the others' errors


# ------------------------------------------------------------------------------------------------------------------------------------
# why fp64
# ------------------------------------------------------------------------------------------------------------------------------------
def test_fp32_sums_move_the_coefficients_a_hundred_times_more_than_fp64_sums():
    """S = 64, M = 512, LIME's weights: the same sequential sums taken in fp32 (a rounded product, a rounded sum) against the fp64 sums,
    both through lime_solve and compared with lime_solve of the extended-precision product.  Only the ratio is asserted."""
    m, s, k = 512, 64, 2
    onoff, w, sc, _ = _job(m, s, k, 21)
    z = np.concatenate([np.ones((m, 1), dtype=bool), onoff != 0], axis=1)
    a32, b32 = np.zeros((s + 1, s + 1), np.float32), np.zeros((s + 1, k), np.float32)
    for i in range(m):
        a32 = np.where(z[i][:, None] & z[i][None, :], a32 + w[i], a32)
        b32 = np.where(z[i][:, None], b32 + (w[i] * sc[i])[None, :], b32)
    assert a32.dtype == np.float32 and b32.dtype == np.float32
    A, B = masks.surrogate_sums(*zero_moments(s, k), onoff, w, sc)
    ea, eb = _exact_moments(onoff, w, sc)
    ref = masks.lime_solve(ea.astype(np.float64), eb.astype(np.float64))[1]
    d64 = np.abs(masks.lime_solve(A, B)[1] - ref).max()
    d32 = np.abs(masks.lime_solve(a32, b32)[1] - ref).max()
    print("fp32 sums move the coefficients by %.3e, fp64 sums by %.3e (scale %.3e)" % (d32, d64, np.abs(ref).max()))
    assert d32 > 100 * d64
