"""The draws and bounds of the shared pool / head kernels' tests, in one place: tests/test_gpu_shared_kernels.py runs them through the
kernels, tests/test_shared_kernel_bounds_cpu.py through a numpy fp32 emulation of the kernels' arithmetic, and the two cannot drift.

Bounds.  u = 2^-24 is one fp32 rounding relative to the rounded value; the re-split into (hi, lo) is 2^-22 = 4 u relative with half of
lo's fp16 subnormal step, 2^-25 <= 2^-24, as the absolute floor.
  Global average pool, per element, against the fp64 mean of the merged planes: ((hw + 1) u + 2^-22) mean|x| + 2^-24 -- hw - 1 serial fp32
  adds (each within u of a partial sum that is at most hw mean|x|, so u mean|x| after the division), the division, the re-split.
  DownsampleB (avgpool2_pad), per real element, against the fp64 mean of the four taps: (3 u + 2^-22) mean|x| + 2^-24 -- 0 + x is exact,
  three adds, the division by 4 is exact, the re-split.  Channels [cin_p, cout_p) are exact zeros.
  Head, per row, with a = row - max(row) and p = softmax(row) in fp64:
      (|a_label| + sum_i p_i |a_i| + ceil(ncls / 64) + 11) u want + 2^-149
  -- the fp32 subtraction in the exponent perturbs exp by |a| u relative (the numerator, and p-weighted every term of the denominator);
  expf within 1 ulp is 2 u on the numerator and 2 u on the denominator; a lane's chain of ceil(ncls / 64) adds and the 6 folds; the
  division; 2^-149 is fp32's subnormal step.  Rows whose fp64 score is under HEAD_FLOOR = 1e-37 (expf's result leaves the normal range at
  1.18e-38) are checked for 0 <= got <= HEAD_FLOOR only; head_cases draws so that they stay under a tenth of the rows.
  Max pool and heat map: exact."""
import math

import numpy as np
import torch

U = 2.0 ** -24
HEAD_FLOOR = 1e-37
HEAD_BATCHES = (1, 4, 5, 9)         # the last workgroup of 4 waves has 1, 4, 1 and 1 live waves
HEAD_SPREADS = (0.01, 4.0, 25.0)

MAXPOOL_CASES = [
    # B, hin, c
    (1, 2, 8),              # one output pixel, its window clipped on two sides
    (2, 4, 8),
    (3, 6, 16),             # a batch index > 0
    (2, 14, 24),            # c / 8 not a power of two
]
AVGPOOL_CASES = [
    # B, hw, c
    (1, 1, 8),              # a single pixel
    (3, 49, 24),
    (2, 169, 1000),
    (5, 12544, 8),          # the longest serial sum any caller could ask for (112 x 112)
    (33, 49, 2048),         # 8448 threads: 33 blocks, the last one ragged
]
AVGPAD_CASES = [(1, 2, 8, 8), (3, 16, 16, 32), (2, 8, 32, 64), (2, 6, 8, 24)]       # B, hin, cin_p, cout_p


def valid_pairs(x):
    """fp32 -> the fp32 values hi + lo of split(x): what a pair of split-fp16 planes can hold."""
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    return hi.float() + lo.float()


def planes(shape, seed, sign=0):
    """fp32 [..., c] as the newer kernel tests draw their planes: exact zeros, both signs, values beyond +-10, a channel band scaled by
    1e-3 (lo in fp16's subnormals); every value a valid (hi, lo) pair.  sign < 0: strictly negative everywhere (no zeros)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * 3.0
    zero = torch.rand(shape, generator=g) < 0.15
    x[torch.rand(shape, generator=g) < 0.10] *= 4.0
    if sign < 0:
        x = -(x.abs() + 0.01)
    else:
        x[zero] = 0.0
    x[..., : max(1, shape[-1] // 4)] *= 1e-3
    out = valid_pairs(x)
    if sign < 0:
        assert (out < 0).all()
    return out


def planes_are_rich(x):
    """The properties a draw of planes() has once it is large enough to show them."""
    band = x[..., : max(1, x.shape[-1] // 4)]
    return bool((x == 0).any() and (x > 10).any() and (x < -10).any() and ((band != 0) & (band.abs() < 6e-3)).any())


def avgpool_bound(x64):
    """x64: fp64 [B][hw][c] merged planes -> (fp64 mean [B][c], bound [B][c])."""
    hw = x64.shape[1]
    return x64.mean(1), ((hw + 1) * U + 2.0 ** -22) * x64.abs().mean(1) + 2.0 ** -24


def avgpad_bound(x64, cin_p):
    """x64: fp64 [B][hin][hin][cin_p] -> (fp64 mean of the four taps [B][ho][ho][cin_p], bound)."""
    b, hin = x64.shape[0], x64.shape[1]
    t = x64.view(b, hin // 2, 2, hin // 2, 2, cin_p)
    return t.mean((2, 4)), (3 * U + 2.0 ** -22) * t.abs().mean((2, 4)) + 2.0 ** -24


# ------------------------------------------------------------------------------------------------
# head
# ------------------------------------------------------------------------------------------------
def head_cases(ncls, seed=0):
    """[(name, rows f32[B][ncls], label i32[B])] for B in HEAD_BATCHES x spread in HEAD_SPREADS.  Every third row (counted through the
    case's phase) is offset by +1e4, where fp32's step is 2^-10: at spread 0.01 such a row has a few dozen distinct values, so it is full
    of tied maxima.  Labels cycle through 0, ncls - 1, the row's argmax and its argmin.  At spread 25 columns 0 and ncls - 1 are lifted by
    60 (2.4 spreads): their softmax is then a deep tail that lies above HEAD_FLOOR and is checked rather than skipped, and the rows under
    the floor are the argmin ones, 5 of the 57 for 1000 classes."""
    rng = np.random.default_rng(1000 * ncls + seed)
    out = []
    k = 0
    for b in HEAD_BATCHES:
        for spread in HEAD_SPREADS:
            rows = (rng.standard_normal((b, ncls)) * spread).astype(np.float32)
            if spread >= 25.0:
                rows[:, 0] += 60.0
                rows[:, ncls - 1] += 60.0
            label = np.zeros(b, dtype=np.int32)
            for r in range(b):
                if (r + k) % 3 == 0:
                    rows[r] += np.float32(1e4)
                kind = (r + k) % 4
                label[r] = (0, ncls - 1, int(rows[r].argmax()), int(rows[r].argmin()))[kind]
            out.append(("B %d spread %g" % (b, spread), rows, label))
            k += 1
    return out


def head_tie_rows(ncls, seed=0):
    """(rows f32[n][ncls], label i32[n], what [n]): the maximum duplicated at i and i + 64 (the same lane; only where ncls > 64), at i and
    i + 1 (neighbouring lanes), at 0 and ncls - 1, and a row of all-equal logits.  The wanted argmax is the first maximum, as torch.argmax
    and numpy's give it."""
    rng = np.random.default_rng(77 * ncls + seed)
    rows, label, what = [], [], []

    def add(at, name):
        row = (rng.standard_normal(ncls) * 4.0).astype(np.float32)
        row[list(at)] = row.max() + np.float32(1.0)
        rows.append(row)
        label.append(at[-1])                    # the score is asked for at the LATER of the tied classes
        what.append(name)

    for i in ([5, 63, ncls - 65] if ncls > 64 else []):
        add((i, i + 64), "max at %d and %d (one lane)" % (i, i + 64))
    for i in ([0, 31, 63, ncls - 2] if ncls > 64 else [0, 4, ncls - 2]):
        add((i, i + 1), "max at %d and %d (neighbouring lanes)" % (i, i + 1))
    add((0, ncls - 1), "max at 0 and %d" % (ncls - 1))
    rows.append(np.full(ncls, 0.7, dtype=np.float32))
    label.append(ncls // 2)
    what.append("all equal")
    return np.stack(rows), np.asarray(label, dtype=np.int32), what


def head_want(rows, label):
    """fp64 softmax score of the label, the bound, the first argmax.  rows f32[B][ncls], label in [0, ncls)."""
    ncls = rows.shape[1]
    r = rows.astype(np.float64)
    a = r - r.max(1, keepdims=True)
    e = np.exp(a)
    p = e / e.sum(1, keepdims=True)
    idx = np.arange(rows.shape[0])
    want = p[idx, label]
    bound = (np.abs(a[idx, label]) + (p * np.abs(a)).sum(1) + math.ceil(ncls / 64) + 11) * U * want + 2.0 ** -149
    return want, bound, rows.argmax(1)


def head_check(name, got_score, got_pred, rows, label):
    """Asserts the head's contract on one batch of rows; -> (worst err / bound over the rows above the floor, rows under the floor)."""
    want, bound, arg = head_want(rows, label)
    assert np.array_equal(np.asarray(got_pred, dtype=np.int64), arg), (name, got_pred, arg)
    got = np.asarray(got_score, dtype=np.float64)
    low = want < HEAD_FLOOR
    assert ((got[low] >= 0) & (got[low] <= HEAD_FLOOR)).all(), (name, got[low])
    ratio = np.abs(got[~low] - want[~low]) / bound[~low]
    worst = float(ratio.max()) if ratio.size else 0.0
    print("head %s: %d rows (%d under the 1e-37 floor), scores %.3e .. %.3e, worst err / bound %.3f" % (name, len(want), int(low.sum()), want.min(), want.max(), worst))
    assert worst <= 1.0, (name, worst)
    return worst, int(low.sum())
