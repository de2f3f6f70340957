"""The rounding-count bounds of tests/test_gpu_shared_kernels.py speak for the kernels only if the arithmetic they describe stays inside
them: a numpy fp32 emulation of the head's order (lane l sums i = l, l + 64, ..., then six xor folds; numpy's exp for expf) and of the
average pools' serial sum + division + re-split, run on the very draws the GPU tests use (tests/shared_kernel_draws.py), against fp64.
No GPU.  Worst err / bound with numpy 2: head 0.61 (1000 classes) and 0.35 (10), global pool 0.45, DownsampleB 0.50."""
import numpy as np
import pytest
import torch

import shared_kernel_draws as draws

F32 = np.float32


def _split_merge(v):
    hi = v.astype(np.float16)
    lo = (v - hi.astype(F32)).astype(np.float16)
    return hi.astype(F32) + lo.astype(F32)


def emulate_head(rows, label):
    """mpx_head_softmax_gather's arithmetic for rows f32[B][ncls]."""
    b, ncls = rows.shape
    score = np.zeros(b, dtype=F32)
    pred = np.zeros(b, dtype=np.int32)
    lanes = np.arange(64)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for n in range(b):
            row = rows[n]
            mx = np.full(64, -np.inf, dtype=F32)
            arg = np.zeros(64, dtype=np.int64)
            for i in range(ncls):
                l = i & 63
                if row[i] > mx[l]:
                    mx[l], arg[l] = row[i], i
            for off in (32, 16, 8, 4, 2, 1):
                omx, oarg = mx[lanes ^ off], arg[lanes ^ off]
                take = (omx > mx) | ((omx == mx) & (oarg < arg))
                mx, arg = np.where(take, omx, mx), np.where(take, oarg, arg)
            assert (mx == mx[0]).all() and (arg == arg[0]).all()            # every lane ends with the same pair
            m = mx[0]
            s = np.zeros(64, dtype=F32)
            for i in range(ncls):
                s[i & 63] = F32(s[i & 63] + np.exp(F32(row[i] - m)))
            for off in (32, 16, 8, 4, 2, 1):
                s = (s + s[lanes ^ off]).astype(F32)
            lb = int(label[n])
            score[n] = F32(np.exp(F32(row[lb] - m)) / s[0]) if 0 <= lb < ncls else F32(0)
            pred[n] = arg[0]
    return score, pred


@pytest.mark.parametrize("ncls", [1000, 10])
def test_head_order_stays_inside_its_bound(ncls):
    worst, low, total = 0.0, 0, 0
    for name, rows, label in draws.head_cases(ncls):
        score, pred = emulate_head(rows, label)
        w, n_low = draws.head_check("ncls %d %s" % (ncls, name), score, pred, rows, label)
        worst, low, total = max(worst, w), low + n_low, total + len(label)
        assert (rows.max(1) > 9e3).any() or len(label) < 3              # the +1e4 rows are there
    print("head ncls %d: %d rows, %d under the floor, worst err / bound %.3f" % (ncls, total, low, worst))
    assert total == 3 * sum(draws.HEAD_BATCHES) and low < 0.10 * total
    if ncls == 1000:
        assert low >= 1                                                  # a spread at which expf underflows is in the draw


@pytest.mark.parametrize("ncls", [1000, 10])
def test_head_ties_and_bad_labels(ncls):
    rows, label, what = draws.head_tie_rows(ncls)
    score, pred = emulate_head(rows, label)
    draws.head_check("ncls %d ties" % ncls, score, pred, rows, label)
    assert pred[-1] == 0 and abs(float(score[-1]) - 1.0 / ncls) <= draws.head_want(rows[-1:], label[-1:])[1][0]
    for bad in (-1, ncls, 2 ** 31 - 1):
        s, p = emulate_head(rows, np.full(len(label), bad, dtype=np.int64))
        assert (s == 0).all() and np.array_equal(p, pred)
    nan_rows = np.full((2, ncls), np.nan, dtype=F32)
    s, p = emulate_head(nan_rows, np.zeros(2, dtype=np.int32))
    assert np.isnan(s).all() and (p == 0).all()
    assert int(torch.argmax(torch.from_numpy(nan_rows), 1)[0]) == 0      # what the reference's argmax gives on such a row


def emulate_avgpool(x):
    """mpx_global_avgpool's arithmetic for merged planes f32[B][hw][c]: serial fp32 sum in pixel order, one division, the re-split."""
    s = np.zeros((x.shape[0], x.shape[2]), dtype=F32)
    for i in range(x.shape[1]):
        s = (s + x[:, i, :]).astype(F32)
    return _split_merge((s / F32(x.shape[1])).astype(F32))


@pytest.mark.parametrize("b,hw,c", draws.AVGPOOL_CASES)
def test_avgpool_order_stays_inside_its_bound(b, hw, c):
    x = draws.planes((b, hw, c), seed=100 * hw + c)
    want, bound = draws.avgpool_bound(x.double())
    got = torch.from_numpy(emulate_avgpool(x.numpy())).double()
    worst = ((got - want).abs() / bound).max().item()
    print("global pool %d x %d x %d: worst err / bound %.3f" % (b, hw, c, worst))
    assert worst <= 1.0
    if hw >= 49:
        assert draws.planes_are_rich(x)
        assert (want.abs() < 0.1 * x.double().abs().mean(1)).any()       # cancellation: a mean far below the mean magnitude


@pytest.mark.parametrize("b,hin,cin_p,cout_p", draws.AVGPAD_CASES)
def test_avgpad_order_stays_inside_its_bound(b, hin, cin_p, cout_p):
    x = draws.planes((b, hin, hin, cin_p), seed=10 * hin + cin_p)
    want, bound = draws.avgpad_bound(x.double(), cin_p)
    v = x.numpy().reshape(b, hin // 2, 2, hin // 2, 2, cin_p)
    acc = np.zeros((b, hin // 2, hin // 2, cin_p), dtype=F32)
    for dy in range(2):
        for dx in range(2):
            acc = (acc + v[:, :, dy, :, dx, :]).astype(F32)
    got = torch.from_numpy(_split_merge((acc / F32(4)).astype(F32))).double()
    worst = ((got - want).abs() / bound).max().item()
    print("avgpool2_pad %d x %d x %d: worst err / bound %.3f" % (b, hin, cin_p, worst))
    assert worst <= 1.0


def test_the_draws_are_what_they_claim():
    x = draws.planes((2, 14, 14, 24), seed=3)
    assert draws.planes_are_rich(x) and torch.equal(draws.valid_pairs(x), x)
    neg = draws.planes((2, 6, 6, 16), seed=4, sign=-1)
    assert (neg < 0).all() and torch.equal(draws.valid_pairs(neg), neg)
    rows, label, what = draws.head_tie_rows(1000)
    assert len(what) == 3 + 4 + 1 + 1 and all((r == r.max()).sum() >= 2 for r in rows)
    assert len(draws.head_tie_rows(10)[2]) == 3 + 1 + 1
