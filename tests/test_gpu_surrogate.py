"""GPU tests of the linear-surrogate path (csrc/mpx_surrogate.h), through ctypes as the other GPU tests.

  sums    mpx_surrogate_accumulate against the numpy fp64 restatement (masks.surrogate_sums), BIT FOR BIT on the fp64 bits, at the edges
          of the row block (64), the column tile (32) and the mask stage (64), with A and B pre-loaded, fenced on both sides, NaN in the
          padding of the score rows, all-off and all-on rows and on-bytes other than 1; the rows cut into three calls; one NaN score;
  paint   mpx_segment_paint against masks.segment_paint, exactly;
  whole   score_masks_classes against score_masks per class, bit for bit, on both stagings; lime and kernel_shap against lime_solve /
          shap_solve of surrogate_sums over score_masks_classes' scores, bit for bit in fp64, and LIME's coefficients against those from
          the CPU oracle's scores within the bound the fit's own operator norm gives the project's score tolerance.

There are no tolerances here beyond the project's SCORE_TOL, that derived bound and the fp64 rounding of sum(phi).
Measured on one MI355X: every bit comparison exact; sum(phi) - (f1 - f0) = 0 on both jobs; the device scores at most 1.3e-6 from the CPU
oracle's, LIME's coefficients at most 1.4e-7 apart against the bound 2.2e-4; the 35 tests take 3 s."""
import functools

import numpy as np
import pytest
import torch

from gpu_common import Fenced, SCORE_TOL, dev, ptr as _p  # noqa: F401  (dev is a fixture)
from network_interpretation_imagenet_amd import masks, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine
from oracle import scorer

pytestmark = pytest.mark.gpu

IMG = 224
NCLS = 1000
MPX_E_ARG = -1
SEED = 3


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def sd18():
    return synth.make_state_dict("resnet18")


@pytest.fixture(scope="module")
def eng(mpx_lib, dev, sd18):
    """resnet18, max_batch = 32: 40 rows run as 32 + 8, 300 rows as 9 x 32 + 12."""
    e = MaskedForwardEngine("resnet18", max_batch=32, device=0).load_state_dict(sd18)
    yield e
    e.close()


@pytest.fixture(scope="module")
def picture():
    img = synth.make_images(2, kind="noise")[1]
    return img, scorer.to_tensor_normalize(img)


# ------------------------------------------------------------------------------------------------------------------------------------
# the moment sums
# ------------------------------------------------------------------------------------------------------------------------------------
class Fenced64:
    """rows x cols fp64 elements inside a gpu_common.Fenced buffer of twice as many fp32 elements, pre-loaded with `start`."""

    def __init__(self, start, dev):
        rows, cols = start.shape
        self.f = Fenced(rows, 2 * cols, dev, f32=True)
        self.view = self.f.payload.view(torch.float64)
        assert tuple(self.view.shape) == (rows, cols) and self.view.is_contiguous()
        self.view.copy_(torch.from_numpy(np.array(start, dtype=np.float64)))

    def result(self):
        torch.cuda.synchronize()
        assert self.f.problems() == [], "; ".join(self.f.problems())
        return self.view.cpu().numpy()


@functools.lru_cache(maxsize=None)
def sums_case(m, s, k):
    """onoff u8[m, s] with an all-off row, an all-on row and the on-bytes 2 and 255, weights of both signs with a zero, scores with both
    zeros, and non-zero starting values of A and B; computed once and never written."""
    rng = np.random.default_rng(1000 * s + 10 * k + m)
    onoff = rng.integers(0, 2, size=(m, s), dtype=np.uint8)
    onoff[onoff != 0] = rng.choice(np.array([1, 2, 255], np.uint8), size=int((onoff != 0).sum()))
    if m > 2:
        onoff[1], onoff[m - 1] = 0, 255
    w = rng.uniform(-0.5, 1.5, size=m).astype(np.float32)
    sc = rng.standard_normal((m, k)).astype(np.float32)
    if m > 3:
        w[3] = 0.0
        sc[2, 0], sc[3, k - 1] = 0.0, -0.0
    a0, b0 = rng.standard_normal((s + 1, s + 1)), rng.standard_normal((s + 1, k))
    for a in (onoff, w, sc, a0, b0):
        a.setflags(write=False)
    return onoff, w, sc, a0, b0


def run_sums(eng, dev, onoff, w, sc, a0, b0, pad, cuts=None):
    """One launch (or one per (lo, hi) of cuts) of mpx_surrogate_accumulate -> (A, B) host fp64.  The score rows lie K + pad apart with NaN
    in the padding; A and B start from a0 and b0 between fences, which are checked."""
    m, k = sc.shape
    pitch = k + pad
    rows = np.full((m, pitch), np.nan, dtype=np.float32)
    rows[:, :k] = sc
    sc_d, onoff_d, w_d = torch.from_numpy(rows).to(dev), torch.from_numpy(onoff.copy()).to(dev), torch.from_numpy(w.copy()).to(dev)
    fa, fb = Fenced64(a0, dev), Fenced64(b0, dev)
    for lo, hi in cuts or [(0, m)]:
        rc = eng._lib.mpx_surrogate_accumulate(eng._h, _p(onoff_d[lo:hi]), _p(w_d[lo:hi]), _p(sc_d[lo:hi]), pitch, hi - lo,
                                               onoff.shape[1], k, _p(fa.view), _p(fb.view), None)
        assert rc == 0, eng._lib.mpx_last_error(eng._h)
    return fa.result(), fb.result()


# (S, K, M, padding): every S of {1, 7, 33, 64, 65}, every K of {1, 31, 32, 33}, every M of {1, 63, 64, 65, 257}, both pitches;
# S = 63 / 64 put S + 1 on the row block's edge (64 / 65 rows), and K = 1000 with S = 5, M = 9
SUM_SHAPES = [(1, 1, 1, 0), (1, 32, 63, 3), (1, 33, 257, 0), (7, 1, 64, 3), (7, 31, 65, 0), (7, 33, 1, 3), (7, 32, 257, 3),
              (33, 1, 257, 0), (33, 31, 63, 3), (33, 32, 64, 0), (33, 33, 65, 3), (63, 33, 65, 0), (64, 1, 65, 3), (64, 31, 1, 0),
              (64, 32, 257, 3), (64, 33, 63, 0), (65, 1, 63, 0), (65, 31, 64, 3), (65, 32, 65, 0), (65, 33, 257, 3), (5, 1000, 9, 3)]


@pytest.mark.parametrize("s,k,m,pad", SUM_SHAPES)
def test_accumulate_against_restatement(eng, dev, s, k, m, pad):
    onoff, w, sc, a0, b0 = sums_case(m, s, k)
    want_a, want_b = masks.surrogate_sums(a0, b0, onoff, w, sc)
    got_a, got_b = run_sums(eng, dev, onoff, w, sc, a0, b0, pad)
    bad_a, bad_b = bits64(got_a) != bits64(want_a), bits64(got_b) != bits64(want_b)
    assert not bad_a.any(), "A differs at %d elements, the first at %s" % (int(bad_a.sum()), np.argwhere(bad_a)[0])
    assert not bad_b.any(), "B differs at %d elements, the first at %s" % (int(bad_b.sum()), np.argwhere(bad_b)[0])


def test_accumulate_rows_cut_into_calls(eng, dev):
    """257 rows as 1 + 99 + 157 (no cut on a stage of 64) leave the bits of one call, and of the restatement."""
    onoff, w, sc, a0, b0 = sums_case(257, 65, 33)
    whole = run_sums(eng, dev, onoff, w, sc, a0, b0, 3)
    parts = run_sums(eng, dev, onoff, w, sc, a0, b0, 3, cuts=[(0, 1), (1, 100), (100, 257)])
    want = masks.surrogate_sums(a0, b0, onoff, w, sc)
    for g, p, t in zip(whole, parts, want):
        assert (bits64(g) == bits64(p)).all() and (bits64(g) == bits64(t)).all()


@pytest.mark.parametrize("k0", [3, 31, 32])
def test_one_nan_score(eng, dev, k0):
    """A NaN at scores[m0][k0] of a row with superpixels {2, 40} on reaches B[0][k0], B[3][k0] and B[41][k0] and nothing else -- in the first
    tile, at its last class and in the one-class tail tile.  On a row whose superpixels are all off it reaches B[0][k0] alone: z~_0 = 1, the
    intercept's element, is on for every row, and no other element sees that row."""
    m, s, k, m0 = 70, 65, 33, 66
    onoff, w, sc, a0, b0 = (a.copy() for a in sums_case(m, s, k))
    onoff[m0] = 0
    onoff[m0, [2, 40]] = 1
    clean_a, clean_b = run_sums(eng, dev, onoff, w, sc, a0, b0, 3)
    sc[m0, k0] = np.nan
    got_a, got_b = run_sums(eng, dev, onoff, w, sc, a0, b0, 3)
    want_a, want_b = masks.surrogate_sums(a0, b0, onoff, w, sc)
    hit = np.isnan(got_b)
    assert sorted(map(tuple, np.argwhere(hit))) == [(0, k0), (3, k0), (41, k0)]
    assert (bits64(got_a) == bits64(clean_a)).all() and (bits64(got_b)[~hit] == bits64(clean_b)[~hit]).all()
    assert (bits64(got_a) == bits64(want_a)).all() and (bits64(got_b)[~hit] == bits64(want_b)[~hit]).all() and np.isnan(want_b[hit]).all()
    # the same NaN on a row whose superpixels are all off: only the intercept's row sees that row at all
    onoff[m0] = 0
    got_a, got_b = run_sums(eng, dev, onoff, w, sc, a0, b0, 3)
    sc[m0, k0] = 0.5
    clean_a, clean_b = run_sums(eng, dev, onoff, w, sc, a0, b0, 3)
    hit = np.isnan(got_b)
    assert list(map(tuple, np.argwhere(hit))) == [(0, k0)]
    assert (bits64(got_a) == bits64(clean_a)).all() and (bits64(got_b)[~hit] == bits64(clean_b)[~hit]).all()


def test_off_row_reaches_nothing_beyond_the_intercept(eng, dev):
    """An all-off row with a NaN weight and NaN scores: A[0][0] and B[0][:] turn NaN (z~_0 is on for every row), every other element keeps
    the bits of the run without that row."""
    m, s, k = 10, 7, 5
    onoff, w, sc, a0, b0 = (a.copy() for a in sums_case(m, s, k))
    keep = np.arange(m) != 4
    clean_a, clean_b = run_sums(eng, dev, onoff[keep], w[keep], sc[keep], a0, b0, 0)
    onoff[4], w[4], sc[4] = 0, np.nan, np.nan
    got_a, got_b = run_sums(eng, dev, onoff, w, sc, a0, b0, 0)
    assert np.isnan(got_a[0, 0]) and np.isnan(got_b[0]).all()
    got_a[0, 0], clean_a[0, 0] = 0, 0
    assert (bits64(got_a) == bits64(clean_a)).all() and (bits64(got_b[1:]) == bits64(clean_b[1:])).all()


def test_refusals_launch_nothing(eng, dev):
    lib, h = eng._lib, eng._h
    onoff, w, sc, a0, b0 = sums_case(9, 7, 3)
    onoff_d, w_d, sc_d = torch.from_numpy(onoff.copy()).to(dev), torch.from_numpy(w.copy()).to(dev), torch.from_numpy(sc.copy()).to(dev)
    fa, fb = Fenced64(a0, dev), Fenced64(b0, dev)
    seg_d = torch.zeros(IMG, IMG, dtype=torch.int32, device=dev)
    val_d = torch.ones(3, 7, dtype=torch.float32, device=dev)
    out = Fenced(3 * IMG, IMG, dev, f32=True)

    def refused(rc, entry, why):
        msg = lib.mpx_last_error(h)
        assert rc == MPX_E_ARG and msg.startswith(entry + b": ") and why in msg, (rc, msg)

    def acc(o=onoff_d, ww=w_d, s_=sc_d, pitch=3, m=9, s=7, k=3, a=fa.view, b=fb.view):
        return lib.mpx_surrogate_accumulate(h, _p(o), _p(ww), _p(s_), pitch, m, s, k, _p(a), _p(b), None)

    def paint(sg=seg_d, v=val_d, pitch=7, s=7, k=3, o=out.payload):
        return lib.mpx_segment_paint(h, _p(sg), _p(v), pitch, s, k, _p(o), None)

    for kw in (dict(o=None), dict(ww=None), dict(s_=None), dict(a=None), dict(b=None)):
        refused(acc(**kw), b"surrogate_accumulate", b"null pointer")
    refused(acc(m=-1), b"surrogate_accumulate", b"M=-1")
    for k in (0, -2):
        refused(acc(k=k), b"surrogate_accumulate", b"K=%d" % k)
    for s in (0, -1, 1025):
        refused(acc(s=s), b"surrogate_accumulate", b"S=%d outside" % s)
        refused(paint(s=s), b"segment_paint", b"S=%d outside" % s)
    refused(acc(pitch=2), b"surrogate_accumulate", b"score_pitch=2 < K=3")
    for kw in (dict(sg=None), dict(v=None), dict(o=None)):
        refused(paint(**kw), b"segment_paint", b"null pointer")
    refused(paint(k=0), b"segment_paint", b"K=0")
    refused(paint(pitch=6), b"segment_paint", b"value_pitch=6 < S=7")
    assert acc(m=0) == 0                                        # M == 0 succeeds and writes nothing
    got_a, got_b = fa.result(), fb.result()
    assert (bits64(got_a) == bits64(a0)).all() and (bits64(got_b) == bits64(b0)).all()
    assert (out.bits == out.sentinel).all()
    # the Python layer
    A, B = torch.zeros(8, 8, dtype=torch.float64, device=dev), torch.zeros(8, 3, dtype=torch.float64, device=dev)
    eng.surrogate_accumulate(onoff_d, w_d, sc_d, A, B)
    want = masks.surrogate_sums(np.zeros((8, 8)), np.zeros((8, 3)), onoff, w, sc)
    assert (bits64(A.cpu().numpy()) == bits64(want[0])).all() and (bits64(B.cpu().numpy()) == bits64(want[1])).all()
    for bad in (lambda: eng.surrogate_accumulate(onoff_d, w_d[:8], sc_d, A, B),
                lambda: eng.surrogate_accumulate(onoff_d, w_d, sc_d, A.float(), B),
                lambda: eng.surrogate_accumulate(onoff_d, w_d, sc_d, A[:7], B),
                lambda: eng.surrogate_accumulate(onoff_d, w_d, sc_d[:, :2], A, B),
                lambda: eng.surrogate_accumulate(onoff_d.int(), w_d, sc_d, A, B),
                lambda: eng.segment_paint(seg_d.long(), val_d),
                lambda: eng.segment_paint(seg_d, val_d, out=torch.empty(2, IMG, IMG, dtype=torch.float32, device=dev)),
                lambda: eng.lime(np.zeros((IMG, IMG, 3), np.uint8), np.zeros((IMG, IMG), np.int32), classes=[1], n_samples=4,
                                 out=torch.empty(2, IMG, IMG, dtype=torch.float32, device=dev))):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------------------------------------------
# the paint
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,s,pad", [(1, 1, 0), (3, 7, 3), (33, 196, 0)])
def test_segment_paint_against_restatement(eng, dev, k, s, pad):
    rng = np.random.default_rng(40 + s)
    seg = rng.integers(0, s, size=(IMG, IMG), dtype=np.int32)
    seg[0, 0], seg[0, 1], seg[IMG - 1, IMG - 1], seg[5, 5] = -1, s, s + 1000, np.iinfo(np.int32).min     # outside [0, S): +0.0
    value = rng.standard_normal((k, s)).astype(np.float32)
    value[0, 0] = -0.0
    rows = np.full((k, s + pad), np.nan, dtype=np.float32)
    rows[:, :s] = value
    out = Fenced(k * IMG, IMG, dev, f32=True)
    seg_d, rows_d = torch.from_numpy(seg).to(dev), torch.from_numpy(rows).to(dev)       # named: they live until the launch is done
    rc = eng._lib.mpx_segment_paint(eng._h, _p(seg_d), _p(rows_d), s + pad, s, k, _p(out.payload), None)
    assert rc == 0, eng._lib.mpx_last_error(eng._h)
    torch.cuda.synchronize()
    assert out.problems() == [], "; ".join(out.problems())
    got = out.payload.cpu().numpy().reshape(k, IMG, IMG)
    assert (bits32(got) == bits32(masks.segment_paint(seg, value))).all()
    assert bits32(got[0, 0, 0]) == 0 and bits32(got[0, 5, 5]) == 0
    # the Python wrapper on a column block of a wider tensor
    assert (bits32(eng.segment_paint(seg_d, rows_d[:, :s]).cpu().numpy()) == bits32(got)).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# the small networks
# ------------------------------------------------------------------------------------------------------------------------------------
def test_small_network_raw_entries_work_python_methods_refuse(mpx_lib, dev):
    e = MaskedForwardEngine("mnist_net", max_batch=4, device=0)
    try:
        onoff, w, sc, a0, b0 = sums_case(65, 33, 5)
        got = run_sums(e, dev, onoff, w, sc, a0, b0, 3)
        want = masks.surrogate_sums(a0, b0, onoff, w, sc)
        assert (bits64(got[0]) == bits64(want[0])).all() and (bits64(got[1]) == bits64(want[1])).all()
        h = e.image_size
        seg = np.random.default_rng(1).integers(-1, 6, size=(h, h), dtype=np.int32)
        value = np.random.default_rng(2).standard_normal((2, 5)).astype(np.float32)
        got = e.segment_paint(torch.from_numpy(seg).to(dev), torch.from_numpy(value).to(dev))
        assert tuple(got.shape) == (2, h, h) and (bits32(got.cpu().numpy()) == bits32(masks.segment_paint(seg, value))).all()
        img, seg224 = np.zeros((IMG, IMG, 3), np.uint8), block_segments(2, 3)
        for call in (lambda: e.lime(img, seg224, classes=[1], n_samples=8), lambda: e.kernel_shap(img, seg224, classes=[1], n_samples=8),
                     lambda: e.score_masks_classes(img, seg224, np.ones((2, 6), np.uint8), [1])):
            with pytest.raises(ValueError):
                call()
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------------------------
def block_segments(rows, cols):
    """i32[224,224]: rows x cols blocks, labelled in raster order."""
    r, c = np.arange(IMG) * rows // IMG, np.arange(IMG) * cols // IMG
    return (r[:, None] * cols + c[None, :]).astype(np.int32)


# (blocks, rows of the job, its staging): 40 rows stay below stem_table_min_rows, 300 rows take the stem table
WHOLE = {"conv": ((2, 3), 40), "table": ((3, 4), 300)}


def _three_classes(e, img):
    """The predicted class between two others: unsorted on purpose."""
    label, _ = e.predict(img)
    return [(label + 500) % NCLS, label, (label + 7) % NCLS]


@pytest.mark.parametrize("kind", sorted(WHOLE))
def test_score_masks_classes_equals_score_masks(eng, picture, kind):
    (br, bc), n = WHOLE[kind]
    img, seg, s = picture[0], block_segments(br, bc), br * bc
    assert eng.stem_for_rows(n) == kind
    classes = _three_classes(eng, img)
    onoff = masks.lime_onoff(n, s, SEED)
    scores, pred = eng.score_masks_classes(img, seg, onoff, classes)
    assert scores.shape == (n, 3) and scores.dtype == np.float32 and pred.shape == (n,) and pred.dtype == np.int32
    for i, c in enumerate(classes):
        _o, score1, pred1 = eng.score_masks(img, seg, onoff, c)
        assert (bits32(score1) == bits32(scores[:, i])).all() and (pred1 == pred).all(), "class %d" % c
    other = "conv" if kind == "table" else None                 # the caller's choice of staging is passed through
    if other:
        forced, _p2 = eng.score_masks_classes(img, seg, onoff[:40], classes, stem=other)
        _o, score1, _p1 = eng.score_masks(img, seg, onoff[:40], classes[1], stem=other)
        assert (bits32(score1) == bits32(forced[:, 1])).all()


@pytest.mark.parametrize("kind", sorted(WHOLE))
def test_lime_and_kernel_shap_whole_path(eng, dev, sd18, picture, kind):
    """eng.lime / eng.kernel_shap return exactly lime_solve / shap_solve of surrogate_sums over score_masks_classes' scores (fp64 bits); sal
    is the paint of the coefficients rounded to fp32; out= leaves the same bits on the device; sum(phi) = f1 - f0 to the fp64 rounding of
    the elimination (S 2^-52 sum|phi|).  On the 40-row job also against the CPU oracle: see the bound below."""
    (br, bc), n = WHOLE[kind]
    (img, x), seg, s = picture, block_segments(br, bc), br * bc
    classes = _three_classes(eng, img)
    # ---- LIME
    cls, icpt, coef, sal = eng.lime(img, seg, classes=classes, n_samples=n, seed=SEED)
    assert cls.dtype == np.int32 and cls.tolist() == classes
    assert icpt.shape == (3,) and coef.shape == (3, s) and icpt.dtype == np.float64 and coef.dtype == np.float64
    assert sal.shape == (3, IMG, IMG) and sal.dtype == np.float32
    onoff = masks.lime_onoff(n, s, SEED)
    w = masks.lime_weights(onoff)
    scores, _pred = eng.score_masks_classes(img, seg, onoff, classes)
    A, B = masks.surrogate_sums(np.zeros((s + 1, s + 1)), np.zeros((s + 1, 3)), onoff, w, scores)
    want_icpt, want_coef = masks.lime_solve(A, B, 1.0)
    assert (bits64(icpt) == bits64(want_icpt)).all() and (bits64(coef) == bits64(want_coef)).all()
    assert (bits32(sal) == bits32(masks.segment_paint(seg, coef.astype(np.float32)))).all()
    assert np.abs(coef).max() > 0
    out = torch.full((3, IMG, IMG), 7.0, dtype=torch.float32, device=dev)                   # out= is overwritten
    _c, icpt2, coef2, sal_d = eng.lime(img, seg, classes=classes, n_samples=n, seed=SEED, out=out)
    assert sal_d is out and (bits32(out.cpu().numpy()) == bits32(sal)).all()
    assert (bits64(icpt2) == bits64(icpt)).all() and (bits64(coef2) == bits64(coef)).all()
    # ---- KernelSHAP: n - 2 sampled rows behind the all-off and the all-on row
    cls, base, phi, sal = eng.kernel_shap(img, seg, classes=classes, n_samples=n - 2, seed=SEED)
    assert cls.tolist() == classes and base.shape == (3,) and phi.shape == (3, s) and phi.dtype == np.float64
    rows = np.concatenate([np.zeros((1, s), np.uint8), np.ones((1, s), np.uint8), masks.shap_onoff(n - 2, s, SEED)])
    wk = np.ones(n, np.float32)
    wk[:2] = 0
    sk, _pred = eng.score_masks_classes(img, seg, rows, classes)
    A, B = masks.surrogate_sums(np.zeros((s + 1, s + 1)), np.zeros((s + 1, 3)), rows, wk, sk)
    f0, f1 = sk[0].astype(np.float64), sk[1].astype(np.float64)
    want_phi = masks.shap_solve(A, B, f0, f1)
    assert (bits64(phi) == bits64(want_phi)).all() and (bits64(base) == bits64(f0)).all()
    assert (bits32(sal) == bits32(masks.segment_paint(seg, phi.astype(np.float32)))).all()
    gap = np.abs(phi.sum(axis=1) - (f1 - f0))
    print("%s: max |sum(phi) - (f1 - f0)| = %.3e" % (kind, gap.max()))
    assert (gap <= s * 2.0 ** -52 * np.abs(phi).sum(axis=1)).all()
    out.fill_(7.0)
    _c, _b, phi2, sal_d = eng.kernel_shap(img, seg, classes=classes, n_samples=n - 2, seed=SEED, out=out)
    assert sal_d is out and (bits32(out.cpu().numpy()) == bits32(sal)).all() and (bits64(phi2) == bits64(phi)).all()
    if kind != "conv":
        return
    # ---- the oracle's fp32 CPU loop on the same 40 rows.  beta = P y with P = (A + lam D)^-1 Z~^T W, so scores that differ by at most the
    # project's score tolerance move every coefficient by at most |P|_inf SCORE_TOL (the largest absolute row sum of P)
    _sc, _pr, logits = scorer.score_masks_reference_loop(sd18, "resnet18", x, seg, onoff, classes[0], return_logits=True)
    ref = torch.softmax(torch.from_numpy(np.asarray(logits, dtype=np.float32)), dim=1).numpy()[:, classes]
    d_score = np.abs(ref.astype(np.float64) - scores.astype(np.float64)).max()
    assert d_score <= SCORE_TOL
    A, _B = masks.surrogate_sums(np.zeros((s + 1, s + 1)), np.zeros((s + 1, 3)), onoff, w, scores)
    zt = np.concatenate([np.ones((n, 1)), (onoff != 0).astype(np.float64)], axis=1)
    P = np.linalg.solve(A + np.diag([0.0] + [1.0] * s), zt.T * w.astype(np.float64)[None, :])
    bound = np.abs(P).sum(axis=1).max() * SCORE_TOL
    ra, rb = masks.surrogate_sums(np.zeros((s + 1, s + 1)), np.zeros((s + 1, 3)), onoff, w, ref)
    ref_icpt, ref_coef = masks.lime_solve(ra, rb, 1.0)
    err = max(np.abs(ref_coef - coef).max(), np.abs(ref_icpt - icpt).max())
    print("oracle: max |d score| %.3e, max |d coefficient| %.3e, bound |P|_inf x %g = %.3e" % (d_score, err, SCORE_TOL, bound))
    assert err <= bound
