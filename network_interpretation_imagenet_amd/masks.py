"""Mask construction (host logic; the superpixel mask-vectors are integer only).

A mask-vector is onoff in {0,1}^S over the S distinct superpixel labels in np.unique(segments)
order; the reference only ever uses contiguous windows of k = int(0.4*S) labels
(generate_gp_training_data_imagenet.py:223-230, bayesian_active_learning_imagenet.py:173-178).

The second convention, real-valued per-pixel masks, has its host side here too: RISE's draws (rise_cells, rise_shifts, rise_masks) and
rise_weights, the numpy fp32 restatement of the weights csrc/mpx_softmask.h synthesises on the device.

The deletion / insertion curves that score a saliency map (saliency_rank, curve_thresholds, rank_masks_apply, gaussian_taps, blur_fill,
curve_auc) restate csrc/mpx_rankmask.h the same way.

Back on the superpixel side, the linear surrogates LIME and KernelSHAP: their samplers and weights (lime_onoff, lime_weights, shap_onoff,
shapley_kernel_onoff), surrogate_sums, the fp64 restatement of csrc/mpx_surrogate.h's moment sums, the two host solves (lime_solve,
shap_solve) and segment_paint.
"""
import random

import numpy as np

SUPERPIXEL_FRACTION = 0.4   # generate_gp_training_data_imagenet.py:224
BO_UPPER_FRACTION = 0.6     # bayesian_active_learning_imagenet.py:467


def window_size(num_segments):
    """num_conse_superpixels = int(0.4*total_num_segments)."""
    return int(SUPERPIXEL_FRACTION * num_segments)


def bo_upper_bound(num_segments):
    """ub of the BO domain firstIndex in [0, ub] (bayesian_active_learning_imagenet.py:467,478)."""
    return int(BO_UPPER_FRACTION * num_segments)


def window_onoff(num_segments, first_index):
    """u8[S]: 1 on [first_index, first_index+k).  Like the reference's slice
    `np.unique(segments)[firstIndex:firstIndex+k]` a window running off the end truncates and a
    negative first_index follows Python slice semantics."""
    row = np.zeros(num_segments, dtype=np.uint8)
    k = window_size(num_segments)
    row[int(first_index):int(first_index) + k] = 1
    return row


def windows_onoff(num_segments, first_indices):
    """u8[M,S] for a list of window starts."""
    idx = list(first_indices)
    out = np.zeros((len(idx), num_segments), dtype=np.uint8)
    for i, f in enumerate(idx):
        out[i] = window_onoff(num_segments, f)
    return out


def draw_first_indices(num_segments, count, rng=None):
    """firstIndex = randint(1, S-k), both ends inclusive
    (generate_gp_training_data_imagenet.py:227).  rng: random.Random (the reference uses the
    unseeded module-level generator)."""
    rng = rng or random
    k = window_size(num_segments)
    if num_segments - k < 1:
        raise ValueError("too few superpixels (%d) to draw a window start" % num_segments)
    return [rng.randint(1, num_segments - k) for _ in range(count)]


def expand_pixel_mask(seg_rank, onoff_row):
    """u8[H,W] in {0,1}: mask[y,x] = onoff[seg[y,x]] (host mirror of what K0 does on the device;
    used for the PNG wire format and heat-map reduction)."""
    return np.asarray(onoff_row, dtype=np.uint8)[seg_rank]


# ---- RISE: real-valued masks from random grids (Petsiuk, Das, Saenko, BMVC 2018) -----------------------------------------
RISE_IMG = 224
RISE_S_MIN, RISE_S_MAX = 2, 32      # csrc/mpx_softmask.h SM_S_MIN / SM_S_MAX (a mask's s x s cells are staged in at most 1 KB of LDS); the one Python copy


def rise_geometry(s):
    """(cell, U) of an s x s grid: cell = ceil(224 / s) pixels per cell, U = (s + 1) * cell the side of the upsampled grid the 224 x 224
    mask is cropped from.  s = 2, 7, 13, 32 -> (112, 336), (32, 256), (18, 252), (7, 231)."""
    s = int(s)
    if not RISE_S_MIN <= s <= RISE_S_MAX:
        raise ValueError("s=%r outside [%d, %d]" % (s, RISE_S_MIN, RISE_S_MAX))
    cell = -(-RISE_IMG // s)
    return cell, (s + 1) * cell


def _rise_rng(rng):
    return rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)


def rise_cells(M, s, p1=0.5, rng=None):
    """u8[M,s,s]: each cell is kept (1) with probability p1 (RISE's binary grids).  rng: a numpy Generator, a seed, or None."""
    rise_geometry(s)
    if int(M) < 0 or not 0.0 <= float(p1) <= 1.0:
        raise ValueError("M >= 0 and p1 in [0, 1], got M=%r p1=%r" % (M, p1))
    return (_rise_rng(rng).random((int(M), int(s), int(s))) < float(p1)).astype(np.uint8)


def rise_shifts(M, s, rng=None):
    """i32[M,2]: (dy, dx) uniform in [0, cell)^2, where the 224 x 224 mask is cropped from the upsampled grid."""
    cell, _ = rise_geometry(s)
    if int(M) < 0:
        raise ValueError("M >= 0, got %r" % (M,))
    return _rise_rng(rng).integers(0, cell, size=(int(M), 2), dtype=np.int32)


def rise_masks(M, s, p1=0.5, seed=0):
    """(cells u8[M,s,s], shifts i32[M,2]) of one seeded job: the cells, then the shifts, from ONE np.random.default_rng(seed) -- the draws
    MaskedForwardEngine.rise_saliency makes, so that a caller can restate its sum."""
    rng = np.random.default_rng(seed)
    return rise_cells(M, s, p1, rng), rise_shifts(M, s, rng)


def check_rise(cells, shifts, s):
    """What the device entries leave to the caller (include/mpx.h: a shift outside [0, cell) is undefined there): cells u8[M,s,s], shifts
    i32[M,2] in [0, cell), 2 <= s <= 32.  -> (cells, shifts) as contiguous arrays; ValueError otherwise."""
    cell, _ = rise_geometry(s)
    cells, shifts = np.asarray(cells), np.asarray(shifts)
    if cells.dtype != np.uint8 or cells.ndim != 3 or cells.shape[1:] != (int(s), int(s)):
        raise ValueError("cells must be uint8[M,%d,%d], got %s%s" % (s, s, cells.dtype, cells.shape))
    if shifts.dtype != np.int32 or shifts.shape != (cells.shape[0], 2):
        raise ValueError("shifts must be int32[%d,2], got %s%s" % (cells.shape[0], shifts.dtype, shifts.shape))
    if shifts.size and (shifts.min() < 0 or shifts.max() >= cell):
        raise ValueError("shifts must lie in [0, cell=%d) for s=%d, got [%d, %d]" % (cell, s, shifts.min(), shifts.max()))
    return np.ascontiguousarray(cells), np.ascontiguousarray(shifts)


def _rise_axis(Y, s, U):
    """One axis of the upsampling at the shifted coordinates Y (int64): (i0, i1, f) -- integers up to the ONE fp32 division r / 2U."""
    t = np.maximum((2 * Y + 1) * s - U, 0)
    i0 = t // (2 * U)
    r = t - i0 * (2 * U)
    f = r.astype(np.float32) / np.float32(2 * U)
    return i0, np.minimum(i0 + 1, s - 1), f


def rise_weights(cells, shifts, s):
    """f32[M,224,224]: the weight of every pixel under every mask, the numpy fp32 restatement of csrc/mpx_softmask.h (the device is held to it
    bit for bit): the s x s grid upsampled bilinearly to U x U with half-pixel centres -- torch.nn.functional.interpolate(size=(U, U),
    mode="bilinear", align_corners=False) --, cropped at (dy, dx).  i0, i1 and the remainder r are integers, f = fl(r / 2U) is one fp32
    division per axis, and  w = fl(fl(fl(1 - fy) * top) + fl(fy * bot))  with  top = fl(fl(fl(1 - fx) * g[i0][j0]) + fl(fx * g[i0][j1])),
    bot the same on row i1: every product and sum rounded on its own, products before their sum, no FMA."""
    cells, shifts = check_rise(cells, shifts, s)
    s = int(s)
    _, U = rise_geometry(s)
    m_all = cells.shape[0]
    out = np.empty((m_all, RISE_IMG, RISE_IMG), dtype=np.float32)
    pix = np.arange(RISE_IMG, dtype=np.int64)
    one = np.float32(1.0)
    for a in range(0, m_all, 64):       # in blocks: the gathers below hold four [M,224,224] temporaries
        b = min(m_all, a + 64)
        g = (cells[a:b] != 0).astype(np.float32)
        i0, i1, fy = _rise_axis(pix[None, :] + shifts[a:b, 0:1].astype(np.int64), s, U)
        j0, j1, fx = _rise_axis(pix[None, :] + shifts[a:b, 1:2].astype(np.int64), s, U)
        mi = np.arange(b - a)[:, None, None]
        i0, i1, fy = i0[:, :, None], i1[:, :, None], fy[:, :, None]
        j0, j1, fx = j0[:, None, :], j1[:, None, :], fx[:, None, :]
        omx, omy = one - fx, one - fy
        top = omx * g[mi, i0, j0] + fx * g[mi, i0, j1]
        bot = omx * g[mi, i1, j0] + fx * g[mi, i1, j1]
        out[a:b] = omy * top + fy * bot
    return out


def saliency_sum_classes(sal0, scores, w):
    """f32[K,224,224]: the class-tiled saliency sum in numpy fp32, the restatement csrc/mpx_saliency_classes.h is held to bit for bit:
    sal[k] <- fl(sal[k] + fl(scores[m][k] * w[m])) for m ascending, from sal0 -- a rounded product and a rounded sum, no FMA.
    sal0 f32[K,H,W], scores f32[M,K], w f32[M,H,W].  Column k is the single-class sum with weight[m] = scores[m][k]."""
    acc = np.array(sal0, dtype=np.float32, copy=True)
    scores, w = np.asarray(scores, dtype=np.float32), np.asarray(w, dtype=np.float32)
    if acc.ndim != 3 or scores.ndim != 2 or w.ndim != 3 or scores.shape != (w.shape[0], acc.shape[0]) or w.shape[1:] != acc.shape[1:]:
        raise ValueError("sal0 [K,H,W], scores [M,K], w [M,H,W]; got %s, %s, %s" % (acc.shape, scores.shape, w.shape))
    for m in range(scores.shape[0]):
        prod = scores[m][:, None, None] * w[m][None]
        acc = acc + prod
    return acc


def class_selection(classes, top, num_classes=1000):
    """The classes a many-class call names: at most one of `classes` (a non-empty sequence of indices in [0, num_classes)) and `top` (an int
    in [1, num_classes]: that many of the largest logits) -> (i32[K] or None, top or None); (None, None) means all num_classes classes.
    ValueError otherwise -- checked on the host before anything is uploaded."""
    if classes is not None and top is not None:
        raise ValueError("give classes or top, not both")
    if top is not None:
        if isinstance(top, bool) or int(top) != top or not 0 < int(top) <= num_classes:
            raise ValueError("top=%r outside [1, %d]" % (top, num_classes))
        return None, int(top)
    if classes is None:
        return None, None
    cls = np.asarray(classes)
    if cls.ndim != 1 or cls.size == 0 or cls.dtype.kind not in "iu":
        raise ValueError("classes must be a non-empty sequence of integers, got %s%s" % (cls.dtype, cls.shape))
    if cls.min() < 0 or cls.max() >= num_classes:
        raise ValueError("classes outside [0,%d): [%d, %d]" % (num_classes, cls.min(), cls.max()))
    return np.ascontiguousarray(cls, dtype=np.int32), None


def top_classes(logits, k):
    """i32[k]: the classes of the k largest logits, ties to the lower index (a stable sort of the negated logits)."""
    logits = np.asarray(logits).reshape(-1)
    k = int(k)
    if not 0 < k <= logits.size:
        raise ValueError("top=%r outside [1, %d]" % (k, logits.size))
    return np.argsort(-logits, kind="stable")[:k].astype(np.int32)


# ---- a linear surrogate over on/off superpixel rows: LIME (Ribeiro et al., KDD 2016) and KernelSHAP (Lundberg & Lee, NeurIPS 2017) ----
# Both fit  score ~ c0 + sum_j c_j * z_j  to random coalitions z in {0, 1}^S.  The samplers, the weights, the numpy fp64 restatement of the
# moment sums csrc/mpx_surrogate.h accumulates (the device is held to it bit for bit) and the two fp64 solves, which stay on the host.
SURROGATE_S_MAX = 1024              # csrc/mpx_surrogate.h SUR_S_MAX
SHAPLEY_ENUM_S_MAX = 12             # shapley_kernel_onoff enumerates 2^S - 2 rows


def _check_onoff(onoff):
    onoff = np.asarray(onoff)
    if onoff.dtype != np.uint8 or onoff.ndim != 2 or onoff.shape[1] < 1:
        raise ValueError("onoff must be uint8[M,S] with S >= 1, got %s%s" % (onoff.dtype, onoff.shape))
    return onoff


def lime_onoff(M, S, seed=0):
    """u8[M,S]: lime_image's rows -- every superpixel on with probability 1/2 (its randint(0, 2)), row 0 all on (its data[0, :] = 1),
    from ONE np.random.default_rng(seed)."""
    M, S = int(M), int(S)
    if M < 1 or S < 1:
        raise ValueError("M >= 1 and S >= 1, got M=%r S=%r" % (M, S))
    out = np.random.default_rng(seed).integers(0, 2, size=(M, S), dtype=np.uint8)
    out[0] = 1
    return out


def lime_weights(onoff, kernel_width=0.25):
    """f32[M]: LIME's kernel sqrt(exp(-d^2 / kernel_width^2)) of the cosine distance d = 1 - sqrt(k / S) of a row with k superpixels on to
    the all-on row (d = 1 for k = 0), computed in fp64 and rounded once.  1 for an all-on row, exp(-8) for an all-off row at 0.25."""
    onoff = _check_onoff(onoff)
    if not float(kernel_width) > 0.0:
        raise ValueError("kernel_width > 0, got %r" % (kernel_width,))
    k = np.count_nonzero(onoff, axis=1).astype(np.float64)
    d = 1.0 - np.sqrt(k / float(onoff.shape[1]))
    return np.sqrt(np.exp(-(d * d) / float(kernel_width) ** 2)).astype(np.float32)


def shap_size_pmf(S):
    """f64[S-1]: the Shapley kernel's mass on the coalition sizes 1 .. S-1, p(k) proportional to (S - 1) / (k * (S - k))."""
    S = int(S)
    if S < 2:
        raise ValueError("S >= 2, got %r" % (S,))
    k = np.arange(1, S, dtype=np.float64)
    p = (S - 1) / (k * (S - k))
    return p / p.sum()


def shap_onoff(M, S, seed=0):
    """u8[M,S]: KernelSHAP's paired sampling from ONE np.random.default_rng(seed) -- M / 2 sizes drawn from shap_size_pmf(S), then per pair
    row 2t = the first k of a random permutation switched on and row 2t + 1 = its complement.  Rows drawn from the kernel carry weight 1."""
    M, S = int(M), int(S)
    if M < 0 or M % 2 or S < 2:
        raise ValueError("M even and >= 0, S >= 2, got M=%r S=%r" % (M, S))
    rng = np.random.default_rng(seed)
    sizes = rng.choice(np.arange(1, S), size=M // 2, p=shap_size_pmf(S))
    out = np.zeros((M, S), dtype=np.uint8)
    for t, k in enumerate(sizes):
        out[2 * t, rng.permutation(S)[:int(k)]] = 1
        out[2 * t + 1] = 1 - out[2 * t]
    return out


def shapley_kernel_onoff(S):
    """(onoff u8[2^S - 2, S], weight f32[2^S - 2]): every coalition but the empty and the full one, row r - 1 = the bits of r (bit j =
    superpixel j), with the Shapley kernel (S - 1) / (C(S, k) * k * (S - k)).  2 <= S <= 12.  shap_solve on these rows gives the exact
    Shapley values."""
    from math import comb
    S = int(S)
    if not 2 <= S <= SHAPLEY_ENUM_S_MAX:
        raise ValueError("S=%r outside [2, %d]" % (S, SHAPLEY_ENUM_S_MAX))
    r = np.arange(1, 2 ** S - 1, dtype=np.int64)
    onoff = ((r[:, None] >> np.arange(S)[None, :]) & 1).astype(np.uint8)
    k = onoff.sum(axis=1).astype(np.int64)
    binom = np.array([comb(S, int(v)) for v in k], dtype=np.float64)
    return onoff, ((S - 1) / (binom * k * (S - k))).astype(np.float32)


def surrogate_sums(A0, B0, onoff, weight, scores):
    """(A f64[S+1,S+1], B f64[S+1,K]): the moment sums of csrc/mpx_surrogate.h in numpy fp64, the restatement the device is held to bit
    for bit.  With z~_m = (1, onoff[m] != 0), for m ascending from A0 and B0:  A[i][j] <- A[i][j] + w_m where z~_mi and z~_mj are on,
    B[i][k] <- B[i][k] + w_m * scores[m][k] where z~_mi is on (the product of two fp32 numbers is exact in fp64: one rounding per step);
    an element whose condition is off is not touched.  onoff u8[M,S], weight f32[M], scores f32[M,K]."""
    onoff = _check_onoff(onoff)
    m_all, s = onoff.shape
    A = np.array(A0, dtype=np.float64, copy=True)
    B = np.array(B0, dtype=np.float64, copy=True)
    weight, scores = np.asarray(weight), np.asarray(scores)
    if weight.dtype != np.float32 or scores.dtype != np.float32:
        raise ValueError("weight and scores must be float32, got %s and %s" % (weight.dtype, scores.dtype))
    if (A.shape != (s + 1, s + 1) or B.ndim != 2 or B.shape[0] != s + 1 or weight.shape != (m_all,)
            or scores.shape != (m_all, B.shape[1])):
        raise ValueError("A [S+1,S+1], B [S+1,K], onoff [M,S], weight [M], scores [M,K]; got %s, %s, %s, %s, %s"
                         % (A.shape, B.shape, onoff.shape, weight.shape, scores.shape))
    z = np.concatenate([np.ones((m_all, 1), dtype=bool), onoff != 0], axis=1)
    w, sc = weight.astype(np.float64), scores.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(m_all):
            A = np.where(z[m][:, None] & z[m][None, :], A + w[m], A)
            B = np.where(z[m][:, None], B + (w[m] * sc[m])[None, :], B)
    return A, B


def _solve_sym(G, b, what):
    """solve(G, b) in fp64 for a symmetric G; ValueError where G holds a non-finite value or is singular by numpy.linalg.matrix_rank's
    rule, smallest |eigenvalue| <= largest * n * eps (a symmetric matrix's singular values are its |eigenvalues|; eigvalsh reads one
    triangle and costs 5 ms at S = 330 where the SVD behind matrix_rank costs 13)."""
    if not (np.isfinite(G).all() and np.isfinite(b).all()):
        raise ValueError("%s: the system holds a NaN or an infinity" % what)
    ev = np.abs(np.linalg.eigvalsh(G))
    if ev.min() <= ev.max() * G.shape[0] * np.finfo(np.float64).eps:
        raise ValueError("%s: the system is singular (too few rows, or dependent columns without a penalty)" % what)
    try:
        return np.linalg.solve(G, b)
    except np.linalg.LinAlgError as e:
        raise ValueError("%s: %s" % (what, e))


def _check_moments(A, B):
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    if A.ndim != 2 or A.shape[0] != A.shape[1] or A.shape[0] < 2 or B.ndim != 2 or B.shape[0] != A.shape[0]:
        raise ValueError("A must be [S+1,S+1] and B [S+1,K], got %s and %s" % (A.shape, B.shape))
    return A, B


def lime_solve(A, B, lam=1.0):
    """(intercept f64[K], coef f64[K,S]): the weighted ridge regression of LIME from its moment sums -- (A + lam * diag(0, 1, .., 1)) beta
    = B in fp64, the intercept not penalised (sklearn.linear_model.Ridge(alpha=lam, fit_intercept=True, sample_weight=w) on the rows).
    ValueError on a singular system."""
    A, B = _check_moments(A, B)
    if not float(lam) >= 0.0:
        raise ValueError("lam >= 0, got %r" % (lam,))
    pen = np.full(A.shape[0], float(lam))
    pen[0] = 0.0
    beta = _solve_sym(A + np.diag(pen), B, "lime_solve")
    return beta[0].copy(), np.ascontiguousarray(beta[1:].T)


def shap_solve(A, B, f0, f1):
    """phi f64[K,S]: KernelSHAP's constrained fit from the moment sums of rows weighted by the Shapley kernel.  phi_0 = f0 (the score of
    the all-off row) and sum_j phi_j = f1 - f0 (f1 the all-on row's) are imposed by eliminating the last superpixel L, as shap's
    KernelExplainer does: with A's and B's indices shifted by one for the intercept,
      G[j][l] = A[j][l] - A[j][L] - A[L][l] + A[L][L],   b[j] = (B[j] - B[L]) - f0 * (A[0][j] - A[0][L]) - (f1 - f0) * (A[j][L] - A[L][L])
    for j, l < L; phi = solve(G, b), phi_L = (f1 - f0) - sum(phi).  f0, f1: f64[K].  ValueError on a singular system or S < 2."""
    A, B = _check_moments(A, B)
    n, K = A.shape[0], B.shape[1]
    s = n - 1
    if s < 2:
        raise ValueError("S >= 2, got %d" % s)
    f0 = np.asarray(f0, dtype=np.float64).reshape(-1)
    f1 = np.asarray(f1, dtype=np.float64).reshape(-1)
    if f0.shape != (K,) or f1.shape != (K,):
        raise ValueError("f0 and f1 must be [K=%d], got %s and %s" % (K, f0.shape, f1.shape))
    L = s                                   # the last superpixel's index in A and B
    delta = f1 - f0
    G = A[1:L, 1:L] - A[1:L, L:L + 1] - A[L:L + 1, 1:L] + A[L, L]
    b = ((B[1:L] - B[L:L + 1]) - f0[None, :] * (A[0, 1:L] - A[0, L])[:, None]
         - delta[None, :] * (A[1:L, L] - A[L, L])[:, None])
    phi = np.empty((K, s), dtype=np.float64)
    phi[:, :s - 1] = _solve_sym(G, b, "shap_solve").T
    phi[:, s - 1] = delta - phi[:, :s - 1].sum(axis=1)
    return phi


def segment_paint(seg, value):
    """f32[K,H,W]: out[k][p] = value[k][seg[p]], +0.0 where seg[p] lies outside [0, S) -- what mpx_segment_paint writes.  seg: an integer
    [H,W] map of ranks; value: f32[K,S]."""
    seg, value = np.asarray(seg), np.asarray(value)
    if seg.ndim != 2 or not np.issubdtype(seg.dtype, np.integer):
        raise ValueError("seg must be an integer [H,W] map, got %s%s" % (seg.dtype, seg.shape))
    if value.dtype != np.float32 or value.ndim != 2 or value.shape[1] < 1:
        raise ValueError("value must be float32[K,S], got %s%s" % (value.dtype, value.shape))
    inside = (seg >= 0) & (seg < value.shape[1])
    return np.where(inside[None], value[:, np.where(inside, seg, 0)], np.float32(0.0)).astype(np.float32)


# ---- Sobol total-order indices over a grid of cells (Fel, Cadene, Chalvidal, Cord, Vigouroux, Serre, NeurIPS 2021) --------------------
# The design, its rows as csrc/mpx_softmask.h (DesignWeights) gathers them -- the device is held to sobol_weights bit for bit -- and
# Jansen's total-order estimator, which stays on the host in fp64.
SOBOL_GRID_MIN, SOBOL_GRID_MAX = 2, 32      # include/mpx.h MPX_SOBOL_GRID_MIN / _MAX: D = d * d <= 1024 cells, segment_paint's limit


def _sobol_sizes(n_design, grid):
    """(N, d, D) of a design, checked: N >= 2 designs over a d x d grid, 2 <= d <= 32."""
    for name, v in (("n_design", n_design), ("grid", grid)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("%s must be an integer, got %r" % (name, v))
    n, d = int(n_design), int(grid)
    if not SOBOL_GRID_MIN <= d <= SOBOL_GRID_MAX:
        raise ValueError("grid=%r outside [%d, %d]" % (grid, SOBOL_GRID_MIN, SOBOL_GRID_MAX))
    if n < 2:
        raise ValueError("n_design=%r: the variance of the score needs at least 2 designs" % (n_design,))
    if n * (d * d + 1) > 2 ** 31 - 1:
        raise ValueError("n_design=%r over %d cells: more rows than an int holds" % (n_design, d * d))
    return n, d, d * d


def sobol_rows(n_design, grid):
    """R = N * (D + 1): the rows (forwards) of a total-order design of N designs over a grid x grid grid, D = grid * grid."""
    n, _d, D = _sobol_sizes(n_design, grid)
    return n * (D + 1)


def sobol_design(n_design, grid, seed=0):
    """(A, B), each f32[N, D] in [0, 1): the first N points of ONE scrambled Sobol sequence of dimension 2 D
    (torch.quasirandom.SobolEngine(2 * D, scramble=True, seed=seed).draw(N)); columns [:D] are A, columns [D:] are B.  Any N >= 2 is taken;
    a power of two keeps the sequence balanced.  The rows scored are A[j] and, for every cell i, A[j] with cell i taken from B[j]
    (sobol_row_cells): B itself is never a row.  Jansen's total-order estimator (sobol_total_order) does not read f(B), so the N forwards a
    Saltelli layout spends on it are not run."""
    import torch
    n, _d, D = _sobol_sizes(n_design, grid)
    pts = torch.quasirandom.SobolEngine(dimension=2 * D, scramble=True, seed=int(seed)).draw(n).numpy().astype(np.float32, copy=False)
    return np.ascontiguousarray(pts[:, :D]), np.ascontiguousarray(pts[:, D:])


def check_sobol(A, B, grid):
    """What mpx_sobol_apply leaves to the caller: A, B float32[N, grid * grid], finite, within [0, 1], N >= 2, 2 <= grid <= 32.
    -> (A, B) as contiguous arrays; ValueError otherwise."""
    A, B = np.asarray(A), np.asarray(B)
    for name, t in (("A", A), ("B", B)):
        if t.dtype != np.float32 or t.ndim != 2:
            raise ValueError("%s must be float32[N, grid * grid], got %s%s" % (name, t.dtype, t.shape))
    _n, d, D = _sobol_sizes(A.shape[0], grid)
    if A.shape[1] != D or B.shape != A.shape:
        raise ValueError("A and B must both be float32[N, %d] for grid=%d, got %s and %s" % (D, d, A.shape, B.shape))
    for name, t in (("A", A), ("B", B)):
        if not np.isfinite(t).all() or t.min() < 0.0 or t.max() > 1.0:
            raise ValueError("%s must be finite and within [0, 1]" % name)
    return np.ascontiguousarray(A), np.ascontiguousarray(B)


def sobol_cell_map(grid):
    """i32[224,224]: the cell of every pixel, c = ((y * d) // 224) * d + (x * d) // 224 -- piecewise constant cells, as in the paper.  Where
    d does not divide 224 the cells differ by one pixel (d = 3: 75, 75 and 74 pixels along each axis)."""
    _n, d, _D = _sobol_sizes(2, grid)
    a = (np.arange(RISE_IMG, dtype=np.int32) * d) // RISE_IMG
    return np.ascontiguousarray(a[:, None] * d + a[None, :], dtype=np.int32)


def sobol_row_cells(A, B, row0, m):
    """f32[m, D]: the cells of rows [row0, row0 + m) of the design.  Row r < N is A[r]; row r >= N, with q = r - N, j = q // D and
    i = q - j * D, is A[j] with cell i taken from B[j] (j-major: the D rows of one A[j] are adjacent)."""
    A, B = np.asarray(A), np.asarray(B)
    n, D = A.shape
    row0, m = int(row0), int(m)
    if m < 0 or row0 < 0 or row0 + m > n * (D + 1):
        raise ValueError("rows [%d, %d) outside the design's [0, %d)" % (row0, row0 + m, n * (D + 1)))
    r = np.arange(row0, row0 + m)
    q = np.maximum(r - n, 0)
    j = np.where(r < n, r, q // D)
    out = A[j].astype(np.float32)           # a copy: fancy indexing
    sub = np.nonzero(r >= n)[0]
    i = (q - (q // D) * D)[sub]
    out[sub, i] = B[j[sub], i]
    return out


def sobol_weights(A, B, grid, row0, m):
    """f32[m,224,224]: the weight of every pixel under rows [row0, row0 + m), sobol_row_cells(...)[:, sobol_cell_map(grid)] -- a pure gather,
    the numpy restatement of what mpx_sobol_apply's kernel reads."""
    A, B = check_sobol(A, B, grid)
    return np.ascontiguousarray(sobol_row_cells(A, B, row0, m)[:, sobol_cell_map(grid)])


def sobol_total_order(scores, n_design):
    """f64[K, D]: Jansen's total-order indices of D cells from the scores of a design's R = N * (D + 1) rows (f32[R, K], widened to fp64;
    f32[R] is one class).  With fA = scores[:N] and fC[j][i] = scores[N + j * D + i]:
        V[k]     = sum_j (fA[j][k] - mean_j fA[.][k])^2 / (N - 1)
        ST[k][i] = sum_j (fA[j][k] - fC[j][i][k])^2 / (2 N V[k]),     ST[k][.] = 0 where V[k] == 0
    Every sum runs over j in ascending order, so a class's indices do not depend on which other classes share the call."""
    s = np.asarray(scores)
    if s.ndim == 1:
        s = s[:, None]
    n = int(n_design)
    if s.ndim != 2 or n < 2 or s.shape[0] % n or s.shape[0] // n < 2 or s.shape[1] < 1:
        raise ValueError("scores must be [N * (D + 1), K] with N = n_design >= 2 and D >= 1, got %s for n_design=%r" % (s.shape, n_design))
    s = s.astype(np.float64)
    D, K = s.shape[0] // n - 1, s.shape[1]
    fA, fC = s[:n], s[n:].reshape(n, D, K)
    total = np.zeros(K)
    for j in range(n):
        total = total + fA[j]
    mean = total / n
    var, num = np.zeros(K), np.zeros((D, K))
    for j in range(n):
        dev = fA[j] - mean
        var = var + dev * dev
        diff = fA[j][None, :] - fC[j]
        num = num + diff * diff
    var = var / (n - 1)
    st = np.zeros((K, D))
    live = var != 0.0
    st[live] = (num[:, live] / (2.0 * n * var[live])).T
    return st


# ---- occlusion sensitivity: a sliding box (Zeiler, Fergus, ECCV 2014; Captum's Occlusion; MATLAB's occlusionSensitivity) ----------------
# The boxes, their weights as csrc/mpx_softmask.h (BoxWeights) synthesises them, and the overlap mean of the score drops as
# csrc/mpx_occlusion.h accumulates it -- the device is held to box_weights, occlusion_sums and occlusion_mean bit for bit.  (The window_*
# names at the top of this module are superpixel index windows of the Bayesian-optimisation loop: another thing.)
def _occlusion_axes(value, name):
    """An int, or an (h, w) pair of ints -> (h, w)."""
    pair = tuple(value) if isinstance(value, (tuple, list, np.ndarray)) else (value, value)
    if len(pair) != 2 or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in pair):
        raise ValueError("%s must be an int or an (h, w) pair of ints, got %r" % (name, value))
    return int(pair[0]), int(pair[1])


def _occlusion_starts(win, stride):
    """The starts of a window of `win` pixels sliding by `stride` over 224: n = ceil((224 - win) / stride) + 1 of them, the i-th at
    min(i * stride, 224 - win) -- the last box is clipped back inside the image, not hung over its edge, so every pixel is covered."""
    if not 1 <= win <= RISE_IMG:
        raise ValueError("window %r outside [1, %d]" % (win, RISE_IMG))
    if stride < 1:
        raise ValueError("stride %r < 1" % (stride,))
    n = -(-(RISE_IMG - win) // stride) + 1
    return [min(i * stride, RISE_IMG - win) for i in range(n)]


def occlusion_boxes(window=32, stride=16):
    """i32[R,4]: the boxes (y0, x0, y1, x1), half-open, of a window sliding over the 224 x 224 image in row-major order.  window, stride:
    ints or (h, w) pairs; per axis there are ceil((224 - win) / stride) + 1 starts, the last clipped back to 224 - win, so that every pixel
    is covered by at least one box.  window may also be a LIST of (window, stride) pairs: the boxes of those scales, concatenated (stride is
    not read then).  ValueError for a window outside [1, 224] or a stride < 1."""
    if isinstance(window, list):
        if not window:
            raise ValueError("an empty list of (window, stride) scales")
        for scale in window:
            if not isinstance(scale, (tuple, list)) or len(scale) != 2:
                raise ValueError("a list of scales holds (window, stride) pairs, got %r" % (scale,))
        return np.ascontiguousarray(np.concatenate([occlusion_boxes(tuple(w) if isinstance(w, list) else w, s) for w, s in window]))
    wh, ww = _occlusion_axes(window, "window")
    sh, sw = _occlusion_axes(stride, "stride")
    ys, xs = _occlusion_starts(wh, sh), _occlusion_starts(ww, sw)
    return np.array([(y, x, y + wh, x + ww) for y in ys for x in xs], dtype=np.int32).reshape(-1, 4)


def check_boxes(boxes):
    """What mpx_box_apply leaves to the caller: boxes integer [M,4] = (y0, x0, y1, x1) with 0 <= y0 <= y1 <= 224 and 0 <= x0 <= x1 <= 224
    (an empty box is legal: it covers nothing).  -> a contiguous i32[M,4]; ValueError otherwise."""
    b = np.asarray(boxes)
    if b.ndim != 2 or b.shape[1] != 4 or b.dtype.kind not in "iu":
        raise ValueError("boxes must be integer [M,4] = (y0, x0, y1, x1), got %s%s" % (b.dtype, b.shape))
    if b.size and not ((0 <= b[:, :2]).all() and (b[:, :2] <= b[:, 2:]).all() and (b[:, 2:] <= RISE_IMG).all()):
        raise ValueError("boxes must satisfy 0 <= y0 <= y1 <= %d and 0 <= x0 <= x1 <= %d" % (RISE_IMG, RISE_IMG))
    return np.ascontiguousarray(b, dtype=np.int32)


def box_weights(boxes):
    """f32[M,224,224]: 0.0 inside box m, 1.0 outside -- literal slicing, the numpy restatement of what mpx_box_apply's kernel compares."""
    b = check_boxes(boxes)
    w = np.ones((b.shape[0], RISE_IMG, RISE_IMG), dtype=np.float32)
    for m, (y0, x0, y1, x1) in enumerate(b):
        w[m, y0:y1, x0:x1] = 0.0
    return w


def occlusion_sums(sum0, cnt0, boxes, scores, base):
    """(sum f32[K,224,224], cnt i32[224,224]): the restatement csrc/mpx_occlusion.h is held to bit for bit.  From sum0 / cnt0, for m
    ascending, on the pixels box m covers: sum[k] <- fl(sum[k] + fl(base[k] - scores[m][k])) -- one rounded subtraction, one rounded
    addition -- and cnt <- cnt + 1; every other pixel keeps its bits.  scores f32[M,K], base f32[K]."""
    acc = np.array(sum0, dtype=np.float32, copy=True)
    cnt = np.array(cnt0, dtype=np.int32, copy=True)
    b = check_boxes(boxes)
    scores, base = np.asarray(scores, dtype=np.float32), np.asarray(base, dtype=np.float32)
    if (acc.ndim != 3 or acc.shape[1:] != (RISE_IMG, RISE_IMG) or cnt.shape != (RISE_IMG, RISE_IMG)
            or scores.shape != (b.shape[0], acc.shape[0]) or base.shape != (acc.shape[0],)):
        raise ValueError("sum0 [K,224,224], cnt0 [224,224], boxes [M,4], scores [M,K], base [K]; got %s, %s, %s, %s, %s"
                         % (acc.shape, cnt.shape, b.shape, scores.shape, base.shape))
    for m, (y0, x0, y1, x1) in enumerate(b):
        drop = base - scores[m]                     # fp32: one rounding
        acc[:, y0:y1, x0:x1] = acc[:, y0:y1, x0:x1] + drop[:, None, None]
        cnt[y0:y1, x0:x1] += 1
    return acc, cnt


def occlusion_mean(sum, cnt):
    """f32[K,224,224]: sum[k][p] / float32(cnt[p]) where cnt[p] > 0 (one correctly rounded fp32 division), 0.0 where no box covered p."""
    sum, cnt = np.asarray(sum, dtype=np.float32), np.asarray(cnt)
    if sum.ndim != 3 or cnt.shape != sum.shape[1:] or cnt.dtype.kind not in "iu":
        raise ValueError("sum [K,H,W] and integer cnt [H,W]; got %s and %s%s" % (sum.shape, cnt.dtype, cnt.shape))
    out = np.zeros_like(sum)
    np.divide(sum, cnt.astype(np.float32)[None], out=out, where=(cnt > 0)[None])
    return out


# ---- Score-CAM: the network's own activation maps as masks (Wang et al., CVPR-W 2020; ScoreCAM in pytorch-grad-cam) ---------------------
# The numpy fp32 restatements csrc/mpx_cam.h and csrc/mpx_softmask.h (MapWeights) are held to bit for bit: the upsampling g -> 224, the
# normalised cells of every channel, the weight of a row, the score-weighted sum at layer resolution and its upsampling.
CAM_GRID_MIN, CAM_GRID_MAX = 2, 16  # include/mpx.h MPX_CAM_GRID_MIN / _MAX


def _cam_grid(g):
    if isinstance(g, (bool, np.bool_)) or int(g) != g or not CAM_GRID_MIN <= int(g) <= CAM_GRID_MAX:
        raise ValueError("g=%r outside [%d, %d]" % (g, CAM_GRID_MIN, CAM_GRID_MAX))
    return int(g)


def cam_axis(g):
    """(i0 i64[224], i1 i64[224], f f32[224]): one axis of the bilinear upsampling g -> 224 with half-pixel centres, from integers --
    t = max((2y + 1) g - 224, 0), i0 = t // 448, r = t - 448 i0, f = fl(float(r) / 448.0f) (ONE fp32 division), i1 = min(i0 + 1, g - 1):
    RISE's axis (_rise_axis) with no shift and U = 224."""
    g = _cam_grid(g)
    i0, i1, f = _rise_axis(np.arange(RISE_IMG, dtype=np.int64), g, RISE_IMG)
    return i0, i1, f


def cam_upsample(G):
    """f32[..., 224, 224] = up(G) of G f32[..., g, g]: top = fl(fl(fl(1 - fx) G[i0][j0]) + fl(fx G[i0][j1])), bot the same on row i1,
    up = fl(fl(fl(1 - fy) top) + fl(fy bot)) -- every product and sum rounded on its own, products before their sum, no FMA;
    torch.nn.functional.interpolate(G, size=(224, 224), mode="bilinear", align_corners=False) up to rounding."""
    G = np.asarray(G, dtype=np.float32)
    if G.ndim < 2 or G.shape[-1] != G.shape[-2]:
        raise ValueError("G must be [..., g, g], got %s" % (G.shape,))
    i0, i1, f = cam_axis(G.shape[-1])
    one = np.float32(1.0)
    fy, fx = f[:, None], f[None, :]
    omy, omx = one - fy, one - fx
    r0, r1 = G[..., i0, :], G[..., i1, :]                   # [..., 224, g]
    top = omx * r0[..., i0] + fx * r0[..., i1]
    bot = omx * r1[..., i0] + fx * r1[..., i1]
    return omy * top + fy * bot


def check_activations(act):
    """What the Score-CAM driver refuses before anything is uploaded: act f32[C, g, g], finite, 2 <= g <= 16, C >= 1.  -> contiguous."""
    a = np.asarray(act)
    if a.dtype != np.float32 or a.ndim != 3 or a.shape[1] != a.shape[2] or a.shape[0] < 1:
        raise ValueError("activations must be float32[C,g,g] with C >= 1, got %s%s" % (a.dtype, a.shape))
    _cam_grid(a.shape[1])
    if not np.isfinite(a).all():
        raise ValueError("activations must be finite")
    return np.ascontiguousarray(a)


def cam_cells(act):
    """(cells f32[C,g,g], lo f32[C], hi f32[C], valid u8[C]) of act f32[C,g,g]: lo_c / hi_c = min / max over the 224 x 224 values of
    cam_upsample(act_c) (the published code normalises the UPSAMPLED map; its extremes are not the cells'), valid_c = (max cell > min cell)
    and (hi_c > lo_c), cells_c = fl(fl(act_c - lo_c) / fl(hi_c - lo_c)) where valid and +0.0 elsewhere.  The cells lie slightly outside
    [0, 1] where an interior extreme is reached by no pixel centre."""
    act = check_activations(act)
    c = act.shape[0]
    lo, hi = np.empty(c, dtype=np.float32), np.empty(c, dtype=np.float32)
    for a in range(0, c, 64):           # in blocks: cam_upsample holds a few [C,224,224] temporaries
        up = cam_upsample(act[a:a + 64]).reshape(-1, RISE_IMG * RISE_IMG)
        lo[a:a + 64], hi[a:a + 64] = up.min(axis=1), up.max(axis=1)
    flat = act.reshape(c, -1)
    valid = (flat.max(axis=1) > flat.min(axis=1)) & (hi > lo)
    cells = np.zeros_like(act)
    num = act[valid] - lo[valid][:, None, None]
    cells[valid] = num / (hi[valid] - lo[valid])[:, None, None]
    return cells, lo, hi, valid.astype(np.uint8)


def cam_weights(cells):
    """f32[M,224,224]: w = min(max(cam_upsample(cells_m), 0), 1), as two selects (v > 0 ? v : +0.0, then w < 1 ? w : 1) -- what
    mpx_cam_apply's kernel multiplies the image by.  The unclamped value leaves [0, 1] by rounding only."""
    v = cam_upsample(cells)
    w = np.where(v > 0, v, np.float32(0.0))
    return np.where(w < 1, w, np.float32(1.0)).astype(np.float32)


def cam_combine(act, scores, low0=None):
    """(low f32[K,g,g], sal f32[K,224,224]): low[k] starts at +0.0 (or low0: the sum of the rows before these) and takes
    low[k] <- fl(low[k] + fl(scores[r][k] * act_r)) for r ascending -- a rounded product and a rounded sum, no FMA, the RAW activations as
    published --, sal[k] = v > 0 ? v : +0.0 with v = cam_upsample(low[k]).  act f32[R,g,g], scores f32[R,K]; R = 0 gives zero maps."""
    act, scores = np.asarray(act, dtype=np.float32), np.asarray(scores, dtype=np.float32)
    if act.ndim != 3 or act.shape[1] != act.shape[2] or scores.ndim != 2 or scores.shape[0] != act.shape[0] or scores.shape[1] < 1:
        raise ValueError("act [R,g,g] and scores [R,K] with K >= 1; got %s and %s" % (act.shape, scores.shape))
    g = _cam_grid(act.shape[1])
    k = scores.shape[1]
    low = np.zeros((k, g, g), dtype=np.float32) if low0 is None else np.array(low0, dtype=np.float32, copy=True)
    if low.shape != (k, g, g):
        raise ValueError("low0 must be [%d,%d,%d], got %s" % (k, g, g, low.shape))
    for r in range(act.shape[0]):
        prod = scores[r][:, None, None] * act[r][None]
        low = low + prod
    v = cam_upsample(low)
    return low, np.where(v > 0, v, np.float32(0.0)).astype(np.float32)


# ---- deletion / insertion curves of a saliency map (Petsiuk, Das, Saenko, BMVC 2018, section 4.1) ---------------------------------
# The numpy restatements csrc/mpx_rankmask.h is held to bit for bit: a rank per pixel, a threshold per row, a fill image.
BLUR_KLEN_MAX = 31                  # csrc/mpx_rankmask.h BF_KMAX
CURVE_STEP = RISE_IMG * 8           # RISE's default: 8 image rows' worth of pixels per step, 29 rows per curve


def saliency_rank(sal):
    """i32[224,224]: rank[p] = the position of pixel p when the pixels are sorted by falling saliency -- order = argsort(-sal.ravel(),
    kind="stable"), rank[order[k]] = k.  Ties, +0.0 against -0.0 included, go to the lower pixel index (raster order).  A map with a NaN or
    an infinity has no such order: ValueError."""
    sal = np.asarray(sal)
    if sal.shape != (RISE_IMG, RISE_IMG) or not np.issubdtype(sal.dtype, np.floating):
        raise ValueError("saliency must be a floating-point [224,224] map, got %s%s" % (sal.dtype, sal.shape))
    if not np.isfinite(sal).all():
        raise ValueError("saliency holds a NaN or an infinity: its pixels have no order")
    order = np.argsort(-sal.ravel(), kind="stable")
    rank = np.empty(order.size, dtype=np.int32)
    rank[order] = np.arange(order.size, dtype=np.int32)
    return rank.reshape(RISE_IMG, RISE_IMG)


def curve_thresholds(step, hw=RISE_IMG * RISE_IMG):
    """i32[n_steps + 1]: n_i = min(i * step, hw) pixels are replaced (deletion) or revealed (insertion) in row i, n_steps = ceil(hw / step).
    step = 224 * 8 -> 29 rows, 0 .. 50176."""
    step, hw = int(step), int(hw)
    if step <= 0 or hw <= 0:
        raise ValueError("step and hw must be positive, got step=%r hw=%r" % (step, hw))
    n_steps = -(-hw // step)
    return np.minimum(np.arange(n_steps + 1, dtype=np.int64) * step, hw).astype(np.int32)


def rank_masks_apply(x, rank, thresh, fill=None, keep_top=False):
    """f32[M,3,224,224], what mpx_rank_apply stages (bit for bit): row m takes pixel p from x where (rank[p] < thresh[m]) == keep_top and
    from the fill image elsewhere.  fill None: x * 0.0f, the removed pixel of the binary masks (-0.0 under a negative pixel).
    keep_top False = a deletion curve's rows, True = an insertion curve's."""
    x = np.asarray(x)
    rank, thresh = np.asarray(rank), np.asarray(thresh)
    if x.dtype != np.float32 or x.shape != (3, RISE_IMG, RISE_IMG):
        raise ValueError("x must be float32[3,224,224], got %s%s" % (x.dtype, x.shape))
    if rank.dtype != np.int32 or rank.shape != (RISE_IMG, RISE_IMG):
        raise ValueError("rank must be int32[224,224], got %s%s" % (rank.dtype, rank.shape))
    if thresh.dtype != np.int32 or thresh.ndim != 1:
        raise ValueError("thresh must be int32[M], got %s%s" % (thresh.dtype, thresh.shape))
    if fill is None:
        fill = x * np.float32(0.0)
    else:
        fill = np.asarray(fill)
        if fill.dtype != np.float32 or fill.shape != x.shape:
            raise ValueError("fill must be float32[3,224,224], got %s%s" % (fill.dtype, fill.shape))
    top = (rank[None] < thresh[:, None, None])[:, None]
    return np.where(top, x[None], fill[None]) if keep_top else np.where(top, fill[None], x[None])


def _check_taps(taps):
    taps = np.asarray(taps)
    if taps.dtype != np.float32 or taps.ndim != 1 or not 1 <= taps.size <= BLUR_KLEN_MAX or taps.size % 2 == 0:
        raise ValueError("taps must be float32[klen], klen odd in [1, %d], got %s%s" % (BLUR_KLEN_MAX, taps.dtype, taps.shape))
    return np.ascontiguousarray(taps)


def gaussian_taps(klen=11, sigma=5.0):
    """f32[klen]: the sampled Gaussian exp(-(k - r)^2 / (2 sigma^2)), r = klen // 2, normalised to sum 1 in fp64, then rounded to fp32.
    The outer product of these taps with themselves is a normalised sampled 2-D Gaussian.  (RISE's own `gkern` filters an impulse with
    scipy's gaussian_filter instead; it is separable too, and a caller who wants it passes its 1-D profile as `taps`.)"""
    klen = int(klen)
    if not 1 <= klen <= BLUR_KLEN_MAX or klen % 2 == 0 or not float(sigma) > 0.0:
        raise ValueError("klen odd in [1, %d] and sigma > 0, got klen=%r sigma=%r" % (BLUR_KLEN_MAX, klen, sigma))
    d = np.arange(klen, dtype=np.float64) - (klen // 2)
    g = np.exp(-(d * d) / (2.0 * float(sigma) ** 2))
    return (g / g.sum()).astype(np.float32)


def _correlate_last(v, taps):
    """acc = fl(acc + fl(t[k] * v[.., x + k - r])) over the k whose pixel lies inside, k ascending, from +0.0, along the last axis."""
    n, klen = v.shape[-1], taps.size
    r = klen // 2
    acc = np.zeros_like(v)
    for k in range(klen):
        d = k - r
        lo, hi = max(0, -d), min(n, n - d)          # the x with 0 <= x + d < n
        if lo < hi:
            acc[..., lo:hi] = acc[..., lo:hi] + taps[k] * v[..., lo + d:hi + d]
    return acc


def blur_fill(x, taps):
    """f32[3,224,224], what mpx_blur_fill writes (bit for bit): the separable correlation of x with taps, zero padding, in fp32 in the written
    order -- the row pass h, then the same along y over h; every product and every sum rounded on its own.  With gaussian_taps() this is
    RISE's insertion substrate, its Conv2d(3, 3, klen, padding=klen // 2) applied to the normalised image."""
    x = np.asarray(x)
    if x.dtype != np.float32 or x.shape != (3, RISE_IMG, RISE_IMG):
        raise ValueError("x must be float32[3,224,224], got %s%s" % (x.dtype, x.shape))
    taps = _check_taps(taps)
    h = _correlate_last(x, taps)
    return np.ascontiguousarray(_correlate_last(h.transpose(0, 2, 1), taps).transpose(0, 2, 1))


def curve_auc(scores):
    """(sum(s) - s[0] / 2 - s[-1] / 2) / (len(s) - 1) in fp64: the trapezoid rule on a unit interval, RISE's `auc`."""
    s = np.asarray(scores, dtype=np.float64)
    if s.ndim != 1 or s.size < 2:
        raise ValueError("a curve needs at least two scores, got shape %s" % (s.shape,))
    return float((s.sum() - s[0] / 2 - s[-1] / 2) / (s.size - 1))


# ---- the small networks' sampler ------------------------------------------------------------------------
def draw_removed_sets(uniq, k, count, rng=None, burn_window_draw=False):
    """The CIFAR / MNIST scorers' draw: `random.sample(range(np.unique(segments)[0], np.unique(segments)[-1]), k)` per mask
    (generate_gp_training_data_cifar.py:308 with k = 5, generate_gp_training_data_mnist.py:215 with k = 1) -> `count` lists of k
    superpixel LABEL VALUES to switch off.  The population is range(first, last): the LAST superpixel can never be drawn, and with
    gaps in the labels a drawn value may name no superpixel (then `mask[segments == v] = 0` removes nothing).  Like
    random.sample it raises ValueError when k exceeds the population.  burn_window_draw: the MNIST script first draws an unused
    `firstIndex = randint(1, S - 1)` per mask (:210) -- consume it too, so that a seeded generator stays in step with upstream.
    rng: random.Random (the reference uses the unseeded module-level generator)."""
    rng = rng or random
    uniq = np.asarray(uniq)
    lo, hi = int(uniq[0]), int(uniq[-1])
    out = []
    for _ in range(int(count)):
        if burn_window_draw:
            rng.randint(1, len(uniq) - 1)
        out.append(rng.sample(range(lo, hi), int(k)))
    return out


def removed_onoff(uniq, removed_sets):
    """u8[M,S]: removed[m][s] = 1 when the s-th label of np.unique(segments) is in removed_sets[m] (the layout
    MaskedForwardEngine.score_masks_removed / mpx_mask_apply_minmax take)."""
    uniq = np.asarray(uniq)
    out = np.zeros((len(removed_sets), len(uniq)), dtype=np.uint8)
    for m, vals in enumerate(removed_sets):
        if len(vals):
            out[m] = np.isin(uniq, np.asarray(list(vals)))
    return out


def removed_mask_u8(segments, removed_set):
    """u8[H,W] in {0,255}: `mask.fill(255); mask[segments == segVal] = 0` for the drawn values
    (generate_gp_training_data_cifar.py:310-313) -- the picture the scorers write as mask_{i}_{label}.png."""
    seg = np.asarray(segments)
    mask = np.full(seg.shape, 255, dtype=np.uint8)
    if len(removed_set):
        mask[np.isin(seg, np.asarray(list(removed_set)))] = 0
    return mask
