"""What the Sobol tests share (test infrastructure only): literal loop restatements of the design's rows and of Jansen's estimator, the
numpy fp32 restatement of the fill blend, the apply cases of the GPU tests with their seeded designs, and the sentinel check of staged
planes against arbitrary expected values.

The fill blend, in the order csrc/mpx_softmask.h writes it (every operation one fp32 rounding, no FMA -- numpy has none):
    o = fl( fl(v * w) + fl( F * fl(1 - w) ) )
For w = 1 that is fl(v + F * 0) = v as a value (F finite), for w = 0 it is fl(v * 0 + F) = F as a value: `binary_design` draws rows
whose cells are all 0.0 or 1.0, where the blend is a select."""
import numpy as np

from gpu_common import PLANE_IMG, PLANE_SENTINEL
import rise_ref

IMG = 224

# (d, N, row0, M, slot0, engine max_batch): the apply cases of tests/test_gpu_sobol.py
#   (3, 4, 0, 8, 0, 8)      the A -> replacement boundary at row 4 inside a call; uneven cells (75 / 75 / 74)
#   (3, 4, 2, 33, 5, 40)    that boundary, j changing three times, a second tile of one row, slot0 > 0
#   (2, 2, 2, 8, 0, 8)      the smallest grid and design; the design's last row (row 9 of 10)
#   (32, 2, 1023, 8, 0, 8)  D = 1024: i = 1021, 1022, 1023 of j = 0, then i = 0 .. 4 of j = 1 -- the last and the first 7 x 7 cell
#   (7, 4, 0, 5, 2, 8)      u8 and f32 image, out_f32 given
APPLY_CASES = ((3, 4, 0, 8, 0, 8), (3, 4, 2, 33, 5, 40), (2, 2, 2, 8, 0, 8), (32, 2, 1023, 8, 0, 8), (7, 4, 0, 5, 2, 8))


def design(d, n, seed=0):
    """(A, B) f32[n, d * d] random in [0, 1) with an exact 0.0 and an exact 1.0 planted in both."""
    rng = np.random.default_rng(1000 * d + 10 * n + seed)
    A, B = rng.random((n, d * d), dtype=np.float32), rng.random((n, d * d), dtype=np.float32)
    A[0, 1], A[n - 1, 0] = 0.0, 1.0
    B[0, 0], B[n - 1, 1] = 1.0, 0.0
    return A, B


def binary_design(d, n, seed=0):
    """(A, B) f32[n, d * d] in {0.0, 1.0}: every row of the design is a select between the image and the fill."""
    rng = np.random.default_rng(77 + seed)
    return ((rng.random((n, d * d)) < 0.5).astype(np.float32), (rng.random((n, d * d)) < 0.5).astype(np.float32))


def row_cells_loop(A, B):
    """f32[N * (D + 1), D]: every row of the design by a literal double loop -- the N rows of A, then for j, for i: A[j] with cell i from B[j]."""
    n, D = A.shape
    rows = [A[r].copy() for r in range(n)]
    for j in range(n):
        for i in range(D):
            row = A[j].copy()
            row[i] = B[j][i]
            rows.append(row)
    return np.stack(rows).astype(np.float32)


def total_order_loop(scores, n):
    """Jansen's estimator by scalar loops in Python floats (fp64): ST[k][i] = sum_j (fA[j][k] - fC[j][i][k])^2 / (2 N V[k])."""
    s = np.asarray(scores, dtype=np.float64)
    D, K = s.shape[0] // n - 1, s.shape[1]
    st = np.zeros((K, D))
    for k in range(K):
        fa = [float(s[j, k]) for j in range(n)]
        mean = sum(fa) / n
        var = sum((v - mean) ** 2 for v in fa) / (n - 1)
        if var == 0.0:
            continue
        for i in range(D):
            st[k, i] = sum((fa[j] - float(s[n + j * D + i, k])) ** 2 for j in range(n)) / (2.0 * n * var)
    return st


def blend(x, w, F):
    """f32[M,3,224,224]: fl(fl(v * w) + fl(F * fl(1 - w))), the four operations in their written order.  x, F: f32[3,224,224]; w: f32[M,224,224]."""
    x, w, F = np.asarray(x, np.float32), np.asarray(w, np.float32), np.asarray(F, np.float32)
    omw = np.float32(1.0) - w[:, None]
    a = x[None] * w[:, None]
    b = F[None] * omw
    out = a + b
    assert out.dtype == np.float32
    return out


def check_planes_values(planes, want, slot0, out=None):
    """gpu_common.check_planes for arbitrary expected values want f32[M,3,224,224]: slots [slot0, slot0 + M) hold split(want[m]) bit for bit in
    channels 0..2 and +0.0 in channel 3; their 3-pixel border and every other slot still hold the sentinel; out holds want bit for bit."""
    hi, lo = planes.read()
    m = len(want)
    whi, wlo = rise_ref.split16(want.transpose(0, 2, 3, 1))
    for name, got, exp in (("hi", hi, whi), ("lo", lo, wlo)):
        inner = got[slot0:slot0 + m, 3:3 + PLANE_IMG, 3:3 + PLANE_IMG]
        assert (inner[..., :3] == exp).all(), "%s plane differs from the split of the blend at %d elements" % (name, int((inner[..., :3] != exp).sum()))
        assert (inner[..., 3] == 0).all(), "%s: channel 3 is not +0.0" % name
        border = got[slot0:slot0 + m].copy()
        border[:, 3:3 + PLANE_IMG, 3:3 + PLANE_IMG] = PLANE_SENTINEL
        assert (border == PLANE_SENTINEL).all(), "%s: the 3-pixel border was written" % name
        assert (got[:slot0] == PLANE_SENTINEL).all() and (got[slot0 + m:] == PLANE_SENTINEL).all(), "%s: a slot outside [slot0, slot0 + M) was written" % name
    if out is not None:
        assert (out.cpu().numpy().view(np.int32) == want.view(np.int32)).all(), "out_f32_nchw differs from the blend"
