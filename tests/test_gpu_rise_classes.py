"""GPU tests of the many-class RISE path (csrc/mpx_saliency_classes.h), through ctypes as the other GPU tests.

  head   mpx_softmax_gather_classes against mpx_head_softmax_gather on the same logits, BIT FOR BIT, one call of the old head per class;
  sums   mpx_rise_saliency_classes / mpx_softmask_saliency_classes against the numpy fp32 restatement (masks.saliency_sum_classes) and against
         the single-class entries run once per class, BIT FOR BIT, at the edges of the class tile (_lib.SALIENCY_CLASS_TILE) and of the mask
         tile (32), with fences around sal and NaN in the padding of the score rows;
  whole  rise_saliency_classes / score_rise_classes against rise_saliency / score_rise per class, bit for bit, and against the CPU forward.

There are no tolerances here beyond the project's SCORE_TOL and the two bounds derived below (head_row_sum_bound, the all-classes sum).
Measured on one MI355X: every bit comparison exact; max |row sum - 1| 9.4e-8 against the bound 1.37e-6; the scores at most 6.6e-7 from the
CPU forward; the all-classes sum at most 0.07 of its bound; the 69 tests take 4 s."""
import functools

import numpy as np
import pytest
import torch

from gpu_common import dev, ptr as _p  # noqa: F401  (dev is a fixture)
from network_interpretation_imagenet_amd import _lib, masks, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine
from oracle import scorer
import rise_ref

pytestmark = pytest.mark.gpu

IMG = 224
T = _lib.SALIENCY_CLASS_TILE
NCLS = 1000
SCORE_TOL = 1e-4                    # the project's tolerance of a score against the CPU forward (tests/test_gpu_rise.py)
FENCE = np.float32(-12345.678)      # what the maps in front of and behind sal[0 .. K) hold
PAD = np.float32(777.25)            # what the padding [K, score_pitch) of the head's rows holds
MPX_E_ARG, MPX_E_STATE = -1, -2
M_MAX, K_MAX = 65, 2 * T + 1


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.fixture(scope="module")
def sd18():
    return synth.make_state_dict("resnet18")


@pytest.fixture(scope="module")
def eng(mpx_lib, dev, sd18):
    """resnet18, max_batch = 16: 40 masks run as 16 + 16 + 8."""
    e = MaskedForwardEngine("resnet18", max_batch=16, device=0).load_state_dict(sd18)
    yield e
    e.close()


@pytest.fixture(scope="module")
def picture():
    img = synth.make_images(2, kind="noise")[1]
    return img, scorer.to_tensor_normalize(img)


# ------------------------------------------------------------------------------------------------------------------------------------
# head
# ------------------------------------------------------------------------------------------------------------------------------------
def head_row_sum_bound():
    """|sum_k scores[b][k] - 1| for K = 1000, classes = NULL, the sum over k taken in fp64.  u = 2^-24.

    Every output is fl(e_k / S) with e_k = expf(row[k] - mx) THE SAME fp32 value that entered the sum S (one function, one argument), so the
    accuracy of expf cancels: sum_k e_k (1 + d_k) / S with |d_k| <= u (one correctly rounded division each).
    S: lane l adds its 16 (l < 40) or 15 terms one after the other from 0.0 -- the first add is exact, so at most 15 roundings --, then six
    xor-shuffle levels add one rounding each; every term is positive, so each passes through at most 15 + 6 = 21 roundings, counted as 22
    (16 sequential adds + 6 levels):  S = sum_k e_k (1 + t_k), |t_k| <= g = 22u / (1 - 22u).
    Hence sum_k e_k / S lies in [1 / (1 + g), 1 / (1 - g)] and, with the divisions, |sum - 1| <= (1 + u) / (1 - g) - 1.
    Absolute terms: a quotient below the normal range rounds with an absolute error <= 2^-150 (1000 of them), and the fp64 sum of the test
    itself adds at most 1000 * 2^-53 * 2."""
    u = rise_ref.U32
    g = 22 * u / (1 - 22 * u)
    return (1 + u) / (1 - g) - 1 + NCLS * 2.0 ** -150 + NCLS * 2.0 ** -52


@functools.lru_cache(maxsize=None)
def head_logits():
    """f32[5, 1000] with a spread of about +-20 (the softmax terms span e^-40 .. 1), a tie at the top of row 1 and a -0.0 / +0.0 pair."""
    z = (np.random.default_rng(11).uniform(-20.0, 20.0, size=(5, NCLS))).astype(np.float32)
    z[1, 900] = z[1, 17] = z[1].max()
    z[2, 3], z[2, 4] = 0.0, -0.0
    return z


def old_head(eng, logits_d, classes, b):
    """mpx_head_softmax_gather once per class: f32[b, K], 0-based rows of the same logits."""
    out = np.empty((b, len(classes)), dtype=np.float32)
    score = torch.empty(b, dtype=torch.float32, device=logits_d.device)
    pred = torch.empty(b, dtype=torch.int32, device=logits_d.device)
    for k, c in enumerate(classes):
        label = torch.full((b,), int(c), dtype=torch.int32, device=logits_d.device)
        assert eng._lib.mpx_head_softmax_gather(eng._h, _p(logits_d), _p(label), _p(score), _p(pred), b, None) == 0
        out[:, k] = score.cpu().numpy()
    return out


HEAD_CLASSES = {
    1: [417],
    3: [1000, 5, -1],
    6: [999, 3, -1, 3, 1000, 0],                                                # unsorted, a repeat, -1 and 1000
    70: list(np.random.default_rng(3).integers(0, NCLS, size=70)),             # more than one pass of the 64 lanes
}


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("b", [1, 4, 5])
@pytest.mark.parametrize("k", sorted(HEAD_CLASSES))
def test_head_equals_single_label_head(eng, dev, k, b, pad):
    classes = HEAD_CLASSES[k]
    logits_d = torch.from_numpy(head_logits()[:b].copy()).to(dev)
    want = old_head(eng, logits_d, classes, b)
    pitch = k + pad
    scores = torch.full((b + 1, pitch), float(PAD), dtype=torch.float32, device=dev)       # one row more: the row behind the last
    cls_d = torch.tensor(classes, dtype=torch.int32, device=dev)
    assert eng._lib.mpx_softmax_gather_classes(eng._h, _p(logits_d), _p(cls_d), k, _p(scores), pitch, b, None) == 0
    got = scores.cpu().numpy()
    assert (bits(got[:b, :k]) == bits(want)).all()
    assert (got[:b, k:] == PAD).all() and (got[b] == PAD).all()
    for j, c in enumerate(classes):
        if not 0 <= c < NCLS:
            assert (bits(got[:b, j]) == 0).all()                                            # exactly +0.0
    assert (got[:b, :k][:, [0 <= c < NCLS for c in classes]] > 0).all()


def test_head_all_classes(eng, dev):
    """K = 1000, classes = NULL, B = 5: every entry is the old head's, and each row sums to 1 within head_row_sum_bound()."""
    z = head_logits()
    logits_d = torch.from_numpy(z.copy()).to(dev)
    want = old_head(eng, logits_d, range(NCLS), 5)
    for pad in (0, 3):
        scores = torch.full((5, NCLS + pad), float(PAD), dtype=torch.float32, device=dev)
        assert eng._lib.mpx_softmax_gather_classes(eng._h, _p(logits_d), None, NCLS, _p(scores), NCLS + pad, 5, None) == 0
        got = scores.cpu().numpy()
        assert (bits(got[:, :NCLS]) == bits(want)).all()
        assert (got[:, NCLS:] == PAD).all()
    row_sum = got[:, :NCLS].astype(np.float64).sum(1)
    bound = head_row_sum_bound()
    print("head: max |row sum - 1| = %.3e, bound %.3e" % (float(np.abs(row_sum - 1).max()), bound))
    assert (np.abs(row_sum - 1) <= bound).all()
    # the Python wrapper: the same numbers from forward()'s kind of tensor
    assert (bits(eng.class_scores(logits_d).cpu().numpy()) == bits(want)).all()
    sub = eng.class_scores(logits_d, [5, 2, 5])
    assert (bits(sub.cpu().numpy()) == bits(want[:, [5, 2, 5]])).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# saliency sums
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rise_case(s):
    """M_MAX masks of grid s (the first three at the corner shifts), their weights, K_MAX columns of scores and K_MAX nonzero starting maps;
    computed once and never written."""
    cells, shifts = rise_ref.draws(s, M_MAX, seed=100 + s)
    assert (shifts[:3] == rise_ref.corner_shifts(s)).all()
    w = masks.rise_weights(cells, shifts, s)
    rng = np.random.default_rng(200 + s)
    scores = rng.standard_normal((M_MAX, K_MAX)).astype(np.float32)
    scores[0, 0], scores[0, 1], scores[1, 0] = 0.0, -0.0, 3.0e4
    sal0 = rng.standard_normal((K_MAX, IMG, IMG)).astype(np.float32)
    assert (sal0 != 0).all()
    for a in (cells, shifts, w, scores, sal0):
        a.setflags(write=False)
    return cells, shifts, w, scores, sal0


def run_classes(eng, dev, source, s, scores, sal0, pad, cuts=None, cells=None, shifts=None, w=None):
    """One launch (or one per (a, b) of cuts) of the class-tiled entry on masks [0, M) of rise_case(s) -> f32[K,224,224].  The score rows
    lie K + pad apart with NaN in the padding (a padding value that reached a map would show); sal is map 1 .. K of K + 2 maps whose first
    and last hold FENCE, and both are checked."""
    m, k = scores.shape
    pitch = k + pad
    sc = np.full((m, pitch), np.nan, dtype=np.float32)
    sc[:, :k] = scores
    sc_d = torch.from_numpy(sc).to(dev)
    buf = torch.full((k + 2, IMG, IMG), float(FENCE), dtype=torch.float32, device=dev)
    buf[1:k + 1] = torch.from_numpy(np.ascontiguousarray(sal0)).to(dev)
    sal = buf[1:k + 1]
    if source == "rise":
        cells_d, shifts_d = torch.from_numpy(cells[:m].copy()).to(dev), torch.from_numpy(shifts[:m].copy()).to(dev)
    else:
        w_d = torch.from_numpy(w[:m].copy()).to(dev)
    for a, b in cuts or [(0, m)]:
        if source == "rise":
            rc = eng._lib.mpx_rise_saliency_classes(eng._h, _p(cells_d[a:b]), _p(shifts_d[a:b]), _p(sc_d[a:b]), pitch, b - a, k, s, _p(sal), None)
        else:
            rc = eng._lib.mpx_softmask_saliency_classes(eng._h, _p(w_d[a:b]), _p(sc_d[a:b]), pitch, b - a, k, _p(sal), None)
        assert rc == 0, eng._lib.mpx_last_error(eng._h)
    out = buf.cpu().numpy()
    assert (out[0] == FENCE).all() and (out[k + 1] == FENCE).all(), "a map outside sal[0 .. K) was written"
    return out[1:k + 1]


# (K, M, padding of the score rows): every K of {1, T-1, T, T+1, 2T+1}, every M of {1, 32, 33, 65}, both pitches
SUM_SHAPES = [(1, 1, 0), (1, 33, 3), (T - 1, 32, 3), (T, 33, 0), (T + 1, 65, 3), (2 * T + 1, 32, 0), (2 * T + 1, 1, 3)]


@pytest.mark.parametrize("k,m,pad", SUM_SHAPES)
@pytest.mark.parametrize("s", rise_ref.S_CASES)
def test_rise_classes_against_restatement(eng, dev, s, k, m, pad):
    """(a), (e): the RISE source is masks.saliency_sum_classes over masks.rise_weights bit for bit; the fences survive."""
    cells, shifts, w, scores, sal0 = rise_case(s)
    want = masks.saliency_sum_classes(sal0[:k], scores[:m, :k], w[:m])
    got = run_classes(eng, dev, "rise", s, scores[:m, :k], sal0[:k], pad, cells=cells, shifts=shifts)
    bad = bits(got) != bits(want)
    assert not bad.any(), "differs from the restatement at %d elements, maps %s" % (int(bad.sum()), np.unique(np.nonzero(bad)[0])[:8])


@pytest.mark.parametrize("s", rise_ref.S_CASES)
def test_classes_equal_single_class_entries(eng, dev, s):
    """(b), (c) at K = T + 1, M = 33, pitch K + 3: map k is mpx_rise_saliency run with weight = scores[:, k]; the explicit source fed
    masks.rise_weights gives the RISE source's bits, and its map k is mpx_softmask_saliency's (first tile, tile edge, tail)."""
    k, m = T + 1, 33
    cells, shifts, w, scores, sal0 = rise_case(s)
    got = run_classes(eng, dev, "rise", s, scores[:m, :k], sal0[:k], 3, cells=cells, shifts=shifts)
    cells_d, shifts_d = torch.from_numpy(cells[:m].copy()).to(dev), torch.from_numpy(shifts[:m].copy()).to(dev)
    for j in range(k):
        one = torch.from_numpy(sal0[j].copy()).to(dev)
        eng.rise_saliency_accumulate(cells_d, shifts_d, s, torch.from_numpy(scores[:m, j].copy()).to(dev), one)
        assert (bits(one.cpu().numpy()) == bits(got[j])).all(), "map %d differs from mpx_rise_saliency" % j
    ex = run_classes(eng, dev, "explicit", s, scores[:m, :k], sal0[:k], 3, w=w)
    assert (bits(ex) == bits(got)).all()
    w_d = torch.from_numpy(w[:m].copy()).to(dev)
    for j in (0, T - 1, T):
        one = torch.from_numpy(sal0[j].copy()).to(dev)
        eng.soft_saliency_accumulate(w_d, torch.from_numpy(scores[:m, j].copy()).to(dev), one)
        assert (bits(one.cpu().numpy()) == bits(got[j])).all(), "map %d differs from mpx_softmask_saliency" % j


@pytest.mark.parametrize("source", ["rise", "explicit"])
def test_classes_rows_cut_into_calls(eng, dev, source):
    """(d): 2 rows then 3 rows in two calls leave what 5 rows in one call leave."""
    k, s = T + 1, 7
    cells, shifts, w, scores, sal0 = rise_case(s)
    kw = dict(cells=cells, shifts=shifts, w=w)
    whole = run_classes(eng, dev, source, s, scores[:5, :k], sal0[:k], 0, **kw)
    parts = run_classes(eng, dev, source, s, scores[:5, :k], sal0[:k], 0, cuts=[(0, 2), (2, 5)], **kw)
    assert (bits(whole) == bits(parts)).all()
    assert (bits(whole) == bits(masks.saliency_sum_classes(sal0[:k], scores[:5, :k], w[:5]))).all()


@pytest.mark.parametrize("k0", [3, T - 1, T])
def test_one_nan_score_reaches_one_map(eng, dev, k0):
    """(f): NaN at scores[m0][k0] makes map k0 NaN exactly where the restatement says (NaN * w is NaN for every w, 0 included: the whole
    map) and leaves every other map the bits of the run without it: no class reads another class's score -- in the first tile, at its
    last class, and in the one-class tail tile whose clamped score index repeats."""
    k, m, s, m0 = T + 1, 5, 13, 2
    cells, shifts, w, scores, sal0 = rise_case(s)
    clean = run_classes(eng, dev, "rise", s, scores[:m, :k], sal0[:k], 3, cells=cells, shifts=shifts)
    dirty_scores = scores[:m, :k].copy()
    dirty_scores[m0, k0] = np.nan
    want = masks.saliency_sum_classes(sal0[:k], dirty_scores, w[:m])
    got = run_classes(eng, dev, "rise", s, dirty_scores, sal0[:k], 3, cells=cells, shifts=shifts)
    assert (np.isnan(got) == np.isnan(want)).all() and np.isnan(got[k0]).all()
    others = np.arange(k) != k0
    assert not np.isnan(got[others]).any()
    assert (bits(got[others]) == bits(clean[others])).all()


def test_all_classes_against_restatement(eng, dev):
    """(g): K = 1000 (31 full tiles and a tail of 8) at M = 4."""
    s, m = 7, 4
    cells, shifts, w, _scores, _sal0 = rise_case(s)
    rng = np.random.default_rng(9)
    scores = rng.standard_normal((m, NCLS)).astype(np.float32)
    sal0 = rng.standard_normal((NCLS, IMG, IMG)).astype(np.float32)
    want = masks.saliency_sum_classes(sal0, scores, w[:m])
    got = run_classes(eng, dev, "rise", s, scores, sal0, 3, cells=cells, shifts=shifts)
    assert (bits(got) == bits(want)).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# error paths
# ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(eng, dev):
    lib, h = eng._lib, eng._h
    cells, shifts, w, _s, _s0 = rise_case(7)
    cells_d, shifts_d = torch.from_numpy(cells[:2].copy()).to(dev), torch.from_numpy(shifts[:2].copy()).to(dev)
    w_d = torch.from_numpy(w[:2].copy()).to(dev)
    logits_d = torch.from_numpy(head_logits()[:2].copy()).to(dev)
    cls_d = torch.tensor([1, 2, 3], dtype=torch.int32, device=dev)
    sc_d = torch.full((2, 6), float(PAD), dtype=torch.float32, device=dev)
    big = torch.full((2, NCLS), float(PAD), dtype=torch.float32, device=dev)
    sal = torch.full((3, IMG, IMG), float(FENCE), dtype=torch.float32, device=dev)

    def refused(rc, entry, why):
        msg = lib.mpx_last_error(h)
        assert rc == MPX_E_ARG and msg.startswith(entry + b": ") and why in msg, (rc, msg)

    head = lambda lg, cl, k, sc, pitch, b: lib.mpx_softmax_gather_classes(h, _p(lg), _p(cl), k, _p(sc), pitch, b, None)
    rise = lambda c, sh, sc, pitch, m, k, s, out: lib.mpx_rise_saliency_classes(h, _p(c), _p(sh), _p(sc), pitch, m, k, s, _p(out), None)
    soft = lambda ww, sc, pitch, m, k, out: lib.mpx_softmask_saliency_classes(h, _p(ww), _p(sc), pitch, m, k, _p(out), None)

    refused(head(None, cls_d, 3, sc_d, 6, 2), b"softmax_gather_classes", b"null pointer")
    refused(head(logits_d, cls_d, 3, None, 6, 2), b"softmax_gather_classes", b"null pointer")
    for b in (0, -1):
        refused(head(logits_d, cls_d, 3, sc_d, 6, b), b"softmax_gather_classes", b"B=%d" % b)
    for k in (0, -2):
        refused(head(logits_d, cls_d, k, sc_d, 6, 2), b"softmax_gather_classes", b"K=%d" % k)
    refused(head(logits_d, cls_d, 3, sc_d, 2, 2), b"softmax_gather_classes", b"score_pitch=2 < K=3")
    refused(head(logits_d, None, 3, sc_d, 6, 2), b"softmax_gather_classes", b"classes == NULL")
    refused(head(logits_d, None, NCLS - 1, big, NCLS, 2), b"softmax_gather_classes", b"classes == NULL")

    refused(rise(None, shifts_d, sc_d, 6, 2, 3, 7, sal), b"rise_saliency_classes", b"null pointer")
    refused(rise(cells_d, None, sc_d, 6, 2, 3, 7, sal), b"rise_saliency_classes", b"null pointer")
    refused(rise(cells_d, shifts_d, None, 6, 2, 3, 7, sal), b"rise_saliency_classes", b"null pointer")
    refused(rise(cells_d, shifts_d, sc_d, 6, 2, 3, 7, None), b"rise_saliency_classes", b"null pointer")
    refused(soft(None, sc_d, 6, 2, 3, sal), b"softmask_saliency_classes", b"null pointer")
    refused(soft(w_d, None, 6, 2, 3, sal), b"softmask_saliency_classes", b"null pointer")
    refused(soft(w_d, sc_d, 6, 2, 3, None), b"softmask_saliency_classes", b"null pointer")
    for m in (0, -1):
        refused(rise(cells_d, shifts_d, sc_d, 6, m, 3, 7, sal), b"rise_saliency_classes", b"M=%d" % m)
        refused(soft(w_d, sc_d, 6, m, 3, sal), b"softmask_saliency_classes", b"M=%d" % m)
    for k in (0, -1):
        refused(rise(cells_d, shifts_d, sc_d, 6, 2, k, 7, sal), b"rise_saliency_classes", b"K=%d" % k)
        refused(soft(w_d, sc_d, 6, 2, k, sal), b"softmask_saliency_classes", b"K=%d" % k)
    refused(rise(cells_d, shifts_d, sc_d, 2, 2, 3, 7, sal), b"rise_saliency_classes", b"score_pitch=2 < K=3")
    refused(soft(w_d, sc_d, 2, 2, 3, sal), b"softmask_saliency_classes", b"score_pitch=2 < K=3")
    for s in (1, 33, 0, -3):
        refused(rise(cells_d, shifts_d, sc_d, 6, 2, 3, s, sal), b"rise_saliency_classes", b"s=%d outside" % s)
    torch.cuda.synchronize()
    assert (sal.cpu().numpy() == FENCE).all() and (sc_d.cpu().numpy() == PAD).all() and (big.cpu().numpy() == PAD).all()
    # the Python layer
    with pytest.raises(ValueError):
        eng.class_scores(logits_d[:, :999])
    with pytest.raises(ValueError):
        eng.class_scores(logits_d, out=torch.empty(2, 4, dtype=torch.float32, device=dev))         # K = 1000
    with pytest.raises(ValueError):
        eng.rise_saliency_accumulate_classes(cells_d, shifts_d, 7, sc_d[:, :3], sal[:2])            # K of scores and sal differ
    with pytest.raises(ValueError):
        eng.soft_saliency_accumulate_classes(w_d, sc_d[:1, :3], sal)                                # M of weights and scores differ
    with pytest.raises(ValueError):
        eng.rise_saliency_classes(np.zeros((IMG, IMG, 3), np.uint8), classes=[1], n_masks=4,
                                  out=torch.empty(2, IMG, IMG, dtype=torch.float32, device=dev))    # out holds another K


def test_small_network_is_refused(mpx_lib, dev):
    e = MaskedForwardEngine("mnist_net", max_batch=4, device=0)
    try:
        lib, h = e._lib, e._h
        cells, shifts, w, _s, _s0 = rise_case(7)
        cells_d, shifts_d = torch.from_numpy(cells[:2].copy()).to(dev), torch.from_numpy(shifts[:2].copy()).to(dev)
        w_d = torch.from_numpy(w[:2].copy()).to(dev)
        logits_d = torch.zeros(2, NCLS, dtype=torch.float32, device=dev)
        cls_d = torch.tensor([1, 2, 3], dtype=torch.int32, device=dev)
        sc_d = torch.full((2, 3), float(PAD), dtype=torch.float32, device=dev)
        sal = torch.full((3, IMG, IMG), float(FENCE), dtype=torch.float32, device=dev)
        assert lib.mpx_softmax_gather_classes(h, _p(logits_d), _p(cls_d), 3, _p(sc_d), 3, 2, None) == MPX_E_STATE
        assert lib.mpx_last_error(h).startswith(b"softmax_gather_classes: ")
        assert lib.mpx_rise_saliency_classes(h, _p(cells_d), _p(shifts_d), _p(sc_d), 3, 2, 3, 7, _p(sal), None) == MPX_E_STATE
        assert lib.mpx_last_error(h).startswith(b"rise_saliency_classes: ")
        assert lib.mpx_softmask_saliency_classes(h, _p(w_d), _p(sc_d), 3, 2, 3, _p(sal), None) == MPX_E_STATE
        assert lib.mpx_last_error(h).startswith(b"softmask_saliency_classes: ")
        torch.cuda.synchronize()
        assert (sal.cpu().numpy() == FENCE).all() and (sc_d.cpu().numpy() == PAD).all()
        with pytest.raises(ValueError):
            e.rise_saliency_classes(np.zeros((IMG, IMG, 3), np.uint8), classes=[1], n_masks=4)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------------------------
N_MASKS, S_E2E, P1, SEED = 40, 7, 0.5, 3


def _three_classes(e, img):
    """The predicted class between two others: unsorted on purpose."""
    label, _ = e.predict(img)
    return [(label + 500) % NCLS, label, (label + 7) % NCLS]


def _whole_path(e, dev, img):
    classes = _three_classes(e, img)
    got_cls, sal = e.rise_saliency_classes(img, classes=classes, n_masks=N_MASKS, s=S_E2E, p1=P1, seed=SEED)
    assert got_cls.dtype == np.int32 and got_cls.tolist() == classes
    assert sal.dtype == np.float32 and sal.shape == (3, IMG, IMG)
    out = torch.full((3, IMG, IMG), 7.0, dtype=torch.float32, device=dev)                   # out= is overwritten, not added to
    got_cls2, sal_d = e.rise_saliency_classes(img, classes=classes, n_masks=N_MASKS, s=S_E2E, p1=P1, seed=SEED, out=out)
    assert sal_d is out and got_cls2.tolist() == classes
    assert (bits(out.cpu().numpy()) == bits(sal)).all()
    cells, shifts = masks.rise_masks(N_MASKS, S_E2E, P1, SEED)
    scores, pred = e.score_rise_classes(img, cells, shifts, S_E2E, classes)
    assert scores.shape == (N_MASKS, 3) and scores.dtype == np.float32 and pred.dtype == np.int32
    for i, c in enumerate(classes):
        one = e.rise_saliency(img, c, n_masks=N_MASKS, s=S_E2E, p1=P1, seed=SEED)
        assert (bits(one) == bits(sal[i])).all(), "map of class %d differs from rise_saliency" % c
        assert np.abs(one).max() > 0
        score1, pred1 = e.score_rise(img, cells, shifts, S_E2E, c)
        assert (bits(score1) == bits(scores[:, i])).all() and (pred1 == pred).all()
    w = masks.rise_weights(cells[:5], shifts[:5], S_E2E)
    soft_scores, soft_pred = e.score_soft_masks_classes(img, w, classes)                    # the explicit twin on the same weights
    assert (bits(soft_scores) == bits(scores[:5])).all() and (soft_pred == pred[:5]).all()
    return classes, scores, pred


def test_whole_path_resnet18(eng, dev, sd18, picture):
    """16 + 16 + 8 masks.  Per class bit-equal to rise_saliency / score_rise, host path and out= path; the scores of five masks within
    SCORE_TOL of the CPU fp32 forward on the same weighted inputs (the reference forward of tests/test_gpu_rise.py)."""
    img, x = picture
    classes, scores, pred = _whole_path(eng, dev, img)
    cells, shifts = masks.rise_masks(N_MASKS, S_E2E, P1, SEED)
    w = masks.rise_weights(cells[:5], shifts[:5], S_E2E)
    for m in range(5):
        for i, c in enumerate(classes):
            ref_score, ref_pred = scorer.score_one(sd18, "resnet18", x.numpy() * w[m][None], c)
            err = abs(float(scores[m, i]) - float(ref_score))
            print("mask %d class %d: |d| against the CPU forward %.3e" % (m, c, err))
            assert err <= SCORE_TOL and pred[m] == ref_pred


def test_whole_path_squeezenet(mpx_lib, dev, picture):
    """Another family behind the same staging and head."""
    e = MaskedForwardEngine("squeezenet1_1", max_batch=16, device=0).load_state_dict(synth.make_state_dict("squeezenet1_1"))
    try:
        _whole_path(e, dev, picture[0])
    finally:
        e.close()


def test_top_classes_of_the_unmasked_forward(eng, picture):
    img = picture[0]
    logits = eng.score_masks(img, np.zeros((IMG, IMG), np.int32), np.ones((1, 1), np.uint8), 0, return_logits=True)[3][0]
    want = np.argsort(-logits, kind="stable")[:3]
    cls, sal = eng.rise_saliency_classes(img, top=3, n_masks=8, s=S_E2E, p1=P1, seed=SEED)
    assert cls.tolist() == want.tolist() and sal.shape == (3, IMG, IMG)
    assert cls[0] == eng.predict(img)[0]
    _c, named = eng.rise_saliency_classes(img, classes=want, n_masks=8, s=S_E2E, p1=P1, seed=SEED)
    assert (bits(named) == bits(sal)).all()


def test_all_classes_sum_to_the_mask_sum(eng, picture):
    """classes=None at n_masks = 8, p1 = 0.5: for every pixel  sum_k sal[k][p] * (n_masks * p1)  against  sum_m w_m(p).

    The bound.  D = n_masks * p1 = 4 is a power of two, so sal[k][p] * D is the fp32 sum S_k(p) the device held before its division, exactly
    (but for results below the normal range: an absolute 2^-149 per map, and 2^-149 per product of the sum).  rise_ref.saliency_bound gives
    |S_k(p) - sum_m s[m][k] w_m(p)| <= (M + 1) u (1 + M u) sum_m |s[m][k]| w_m(p).  Summed over k, with the scores positive and every row
    sum within R = head_row_sum_bound() of 1:
        sum_k sum_m s[m][k] w_m(p) = sum_m w_m(p) (1 + r_m), |r_m| <= R        and        sum_k sum_m |s[m][k]| w_m(p) <= (1 + R) sum_m w_m(p)
    so  |sum_k S_k(p) - sum_m w_m(p)| <= saliency_bound(0, [1 + R] * M, w)(p) + R sum_m w_m(p) + (K M + K) 2^-149, plus the test's own fp64
    sums over k (<= K 2^-52 of the sum)."""
    n, k = 8, NCLS
    cls, sal = eng.rise_saliency_classes(picture[0], n_masks=n, s=S_E2E, p1=P1, seed=SEED)
    assert cls.tolist() == list(range(k)) and sal.shape == (k, IMG, IMG)
    cells, shifts = masks.rise_masks(n, S_E2E, P1, SEED)
    w = masks.rise_weights(cells, shifts, S_E2E)
    w_sum = w.astype(np.float64).sum(0)
    got = sal.astype(np.float64).sum(0) * (n * P1)
    r = head_row_sum_bound()
    bound = (rise_ref.saliency_bound(np.zeros((IMG, IMG)), np.full(n, 1 + r), w) + r * w_sum + (k * n + k) * 2.0 ** -149
             + k * 2.0 ** -52 * (1 + r) * w_sum)
    err = np.abs(got - w_sum)
    print("all classes: max err %.3e, max err / bound %.3f" % (float(err.max()), float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all() and w_sum.max() > 1
