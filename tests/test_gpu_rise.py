"""GPU tests of the real-valued mask convention (csrc/mpx_softmask.h): mpx_rise_apply / mpx_softmask_apply against the numpy fp32 restatement of
the weight formula (masks.rise_weights) BIT FOR BIT on the staged hi / lo planes, binary weights against mpx_mask_apply_normalize bit for bit,
the saliency entries against an fp32 emulation of their written order (bit for bit) and the fp64 sum (derived bound, rise_ref), the whole path
against the CPU forward, and the refusals.  resnet18 with max_batch = 8 unless another engine is named."""

import numpy as np
import pytest
import torch

from gpu_common import PLANE_SENTINEL as SENTINEL, Planes, check_planes, dev, ptr as _p  # noqa: F401  (dev is a fixture)
from network_interpretation_imagenet_amd import _lib, masks, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine, MpxError, rank_segments
from oracle import scorer
import rise_ref

pytestmark = pytest.mark.gpu

IMG, PAD = 224, 230
SCORE_TOL = 1e-4            # the project's tolerance of a score against the CPU forward


@pytest.fixture(scope="module")
def sd18():
    return synth.make_state_dict("resnet18")


@pytest.fixture(scope="module")
def eng(mpx_lib, dev, sd18):
    e = MaskedForwardEngine("resnet18", max_batch=8, device=0).load_state_dict(sd18)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng40(mpx_lib, dev, sd18):
    """Sized for one mask more than the apply kernels' tile (32) behind slot0 = 5."""
    e = MaskedForwardEngine("resnet18", max_batch=40, device=0).load_state_dict(sd18)
    yield e
    e.close()


@pytest.fixture(scope="module")
def picture():
    """(u8 HWC image, its normalised f32 CHW tensor): noise, so that negative normalised pixels are everywhere."""
    img = synth.make_images(2, kind="noise")[1]
    return img, scorer.to_tensor_normalize(img)


def _image(picture, kind, dev):
    img, x = picture
    return (torch.from_numpy(img) if kind == "u8" else x.clone()).contiguous().to(dev)


# ------------------------------------------------------------------------------------------------------------------------------------
# apply
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("s", rise_ref.S_CASES)
def test_rise_apply_bit_exact(eng, dev, picture, s, kind):
    """5 masks (the three corner shifts and two random ones) into slots [2, 7) of 8."""
    cells, shifts = rise_ref.draws(s, 5, seed=10 + s)
    w = masks.rise_weights(cells, shifts, s)
    out = torch.full((5, 3, IMG, IMG), float("nan"), dtype=torch.float32, device=dev)
    with Planes(eng) as planes:
        eng.stage_rise(_image(picture, kind, dev), torch.from_numpy(cells).to(dev), torch.from_numpy(shifts).to(dev), s, 2, out)
        check_planes(planes, picture[1], w, 2, out)


@pytest.mark.parametrize("source", ["rise", "explicit"])
@pytest.mark.parametrize("m,slot0", [(1, 3), (_lib.SOFTMASK_TILE + 1, 5)])
def test_apply_row_counts(eng, eng40, dev, picture, m, slot0, source):
    """One mask, and one mask more than a block's tile (the second tile of the launch holds a single mask), behind slot0 > 0."""
    e = eng if m == 1 else eng40
    cells, shifts = rise_ref.draws(7, m, seed=m)
    w = masks.rise_weights(cells, shifts, 7)
    with Planes(e) as planes:
        if source == "rise":
            e.stage_rise(_image(picture, "u8", dev), torch.from_numpy(cells).to(dev), torch.from_numpy(shifts).to(dev), 7, slot0)
        else:
            e.stage_soft_masks(_image(picture, "u8", dev), torch.from_numpy(w).to(dev), slot0)
        check_planes(planes, picture[1], w, slot0)


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_explicit_apply_bit_exact(eng, dev, picture, kind):
    """Explicit weights: RISE's at s = 13 and a map of arbitrary values in [0, 1] (not representable as any grid)."""
    cells, shifts = rise_ref.draws(13, 4, seed=3)
    w = masks.rise_weights(cells, shifts, 13)
    w[3] = np.random.default_rng(4).random((IMG, IMG), dtype=np.float32)
    out = torch.full((4, 3, IMG, IMG), float("nan"), dtype=torch.float32, device=dev)
    with Planes(eng) as planes:
        eng.stage_soft_masks(_image(picture, kind, dev), torch.from_numpy(w).to(dev), 1, out)
        check_planes(planes, picture[1], w, 1, out)


def _binary_case(picture):
    """A label map, on/off rows and the {0.0, 1.0} weights that say the same; a removed superpixel covers negative normalised pixels."""
    seg = synth.grid_segments()
    onoff = synth.random_onoff(6, 196, seed=21)
    w = np.ascontiguousarray(onoff[:, seg], dtype=np.float32)
    x = picture[1].numpy()
    assert ((x < 0) & (w[0][None] == 0)).any()
    return seg, onoff, w


@pytest.fixture(scope="module")
def binary_staged(eng, dev, picture):
    """The same six rows staged by mpx_mask_apply_normalize and, as {0.0, 1.0} weights, by mpx_softmask_apply, into slots [1, 7):
    (K0 hi, K0 lo, soft hi, soft lo) as int16 bits of all 8 slots and the two f32 outputs."""
    seg, onoff, w = _binary_case(picture)
    image = _image(picture, "u8", dev)
    f_k0 = torch.empty(6, 3, IMG, IMG, dtype=torch.float32, device=dev)
    f_soft = torch.empty_like(f_k0)
    with Planes(eng) as planes:
        eng.stage_masks(image, torch.from_numpy(seg).to(dev), torch.from_numpy(onoff).to(dev), 1, f_k0)
        k0_hi, k0_lo = planes.read()
        planes.hi.fill_(SENTINEL)
        planes.lo.fill_(SENTINEL)
        eng.stage_soft_masks(image, torch.from_numpy(w).to(dev), 1, f_soft)
        hi, lo = planes.read()
    return k0_hi, k0_lo, hi, lo, f_k0.cpu().numpy(), f_soft.cpu().numpy()


def test_binary_weights_give_k0_planes(binary_staged):
    """The planes of {0.0, 1.0} weights equal mpx_mask_apply_normalize's BIT FOR BIT over all 8 slots, the removed negative pixels
    included: there both kernels write the split of a -0.0 product, hi -0.0 and lo +0.0 (both pin the product in an fp32 register before
    the split, csrc/mpx_conv.h fp32_value).  The f32 outputs are bit-identical too and carry the -0.0."""
    k0_hi, k0_lo, hi, lo, f_k0, f_soft = binary_staged
    assert (hi == k0_hi).all() and (lo == k0_lo).all()
    assert (f_k0.view(np.int32) == f_soft.view(np.int32)).all()
    neg_zero = f_soft.view(np.int32) == np.int32(-2 ** 31)                                   # [6,3,224,224]: removed negative pixels
    assert neg_zero.any()
    at = neg_zero.transpose(0, 2, 3, 1)
    inner_hi, inner_lo = hi[1:7, 3:227, 3:227, :3], lo[1:7, 3:227, 3:227, :3]
    assert (inner_hi[at] == np.int16(-2 ** 15)).all() and (inner_lo[at] == 0).all()          # hi -0.0, lo +0.0 in every channel


def _label_map(which):
    """(label map i32[224,224], S): the 14 x 14 grid (S = 196), or five bands (S = 5: a tile of 33 rows is 165 on/off bytes, no multiple of
    4) in which two blocks of pixels carry the labels -1 and 5 -- outside [0, S), where the weight is 0 whatever the rows say."""
    if which == "grid":
        return synth.grid_segments().astype(np.int32), 196
    seg = np.ascontiguousarray(np.broadcast_to((np.arange(IMG, dtype=np.int32) * 5 // IMG)[:, None], (IMG, IMG)))
    seg[10:30, 40:90] = -1
    seg[100:141, 7:19] = 5
    return seg, 5


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("which", ["grid", "five"])
@pytest.mark.parametrize("m,slot0", [(1, 3), (_lib.SOFTMASK_TILE + 1, 5)])
def test_k0_planes_bit_exact(eng, eng40, dev, picture, m, slot0, which, kind):
    """mpx_mask_apply_normalize held to check_planes with w = onoff[:, seg] from numpy: interior bits (hi -0.0 / lo +0.0 where a negative
    pixel is removed), channel 3, the untouched border and other slots, and out_f32 bit for bit -- one row, and one row more than a block's
    tile, behind slot0 > 0."""
    e = eng if m == 1 else eng40
    seg, s = _label_map(which)
    onoff = synth.random_onoff(m, s, seed=50 + m)
    inside = (seg >= 0) & (seg < s)
    w = np.ascontiguousarray(np.where(inside[None], onoff[:, np.where(inside, seg, 0)], 0), dtype=np.float32)
    assert w.shape == (m, IMG, IMG) and ((picture[1].numpy() < 0) & (w[0][None] == 0)).any()
    if which == "five":
        assert (seg == -1).any() and (seg == s).any()           # without the guard label 5 reads the next row's first byte, label -1 the row before
    out = torch.full((m, 3, IMG, IMG), float("nan"), dtype=torch.float32, device=dev)
    with Planes(e) as planes:
        e.stage_masks(_image(picture, kind, dev), torch.from_numpy(seg).to(dev), torch.from_numpy(onoff).to(dev), slot0, out)
        check_planes(planes, picture[1], w, slot0, out)


# ------------------------------------------------------------------------------------------------------------------------------------
# whole path
# ------------------------------------------------------------------------------------------------------------------------------------
def _whole_path(e, picture, m):
    seg = synth.grid_segments()
    onoff = synth.random_onoff(m, 196, seed=33)
    w = np.ascontiguousarray(onoff[:, seg], dtype=np.float32)
    img = picture[0]
    label, _ = e.predict(img)
    _o, score, pred, logits = e.score_masks(img, seg, onoff, label, return_logits=True, stem="conv")
    s_score, s_pred, s_logits = e.score_soft_masks(img, w, label, return_logits=True)
    assert (score.view(np.int32) == s_score.view(np.int32)).all() and (pred == s_pred).all()
    assert (logits.view(np.int32) == s_logits.view(np.int32)).all()
    _o, score2, pred2 = e.score_masks(img, seg, onoff, label, stem="conv")
    s_score2, s_pred2 = e.score_soft_masks(img, w, label)
    assert (score2.view(np.int32) == s_score2.view(np.int32)).all() and (pred2 == s_pred2).all()


def test_score_soft_masks_equals_score_masks_resnet18(eng, picture):
    _whole_path(eng, picture, 11)           # 8 + 3: two forwards


def test_score_soft_masks_equals_score_masks_squeezenet(mpx_lib, dev, picture):
    """Another stem behind the same staging: the soft masks are family-independent."""
    e = MaskedForwardEngine("squeezenet1_1", max_batch=4, device=0).load_state_dict(synth.make_state_dict("squeezenet1_1"))
    try:
        _whole_path(e, picture, 5)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# saliency
# ------------------------------------------------------------------------------------------------------------------------------------
SAL_SCORES = np.array([0.0, -0.37, 3.0e4, 0.91, 1.0e-3], dtype=np.float32)


@pytest.mark.parametrize("s", [7, 13])
def test_saliency_against_emulation(eng, dev, s):
    cells, shifts = rise_ref.draws(s, 5, seed=40 + s)
    w = masks.rise_weights(cells, shifts, s)
    sal0 = np.random.default_rng(5).standard_normal((IMG, IMG)).astype(np.float32)         # accumulation starts from what is there
    cells_d, shifts_d = torch.from_numpy(cells).to(dev), torch.from_numpy(shifts).to(dev)
    score_d = torch.from_numpy(SAL_SCORES).to(dev)
    want = rise_ref.saliency_emulation(sal0, SAL_SCORES, w)

    one = torch.from_numpy(sal0).to(dev)
    eng.rise_saliency_accumulate(cells_d, shifts_d, s, score_d, one)
    got = one.cpu().numpy()
    assert (got.view(np.int32) == want.view(np.int32)).all(), "differs from the fp32 emulation at %d pixels" % int((got != want).sum())

    exact32 = sal0.astype(np.float64) + np.tensordot(SAL_SCORES.astype(np.float64), w.astype(np.float64), 1)
    bound = rise_ref.saliency_bound(sal0, SAL_SCORES, w)
    err = np.abs(got - exact32)
    print("s=%d max err / bound against the fp64 sum of the fp32 weights: %.3f" % (s, float((err / bound).max())))
    assert (err <= bound).all()
    exact64 = sal0.astype(np.float64) + np.tensordot(SAL_SCORES.astype(np.float64), rise_ref.ref_weights64(cells, shifts, s), 1)
    assert (np.abs(got - exact64) <= bound + np.abs(SAL_SCORES).sum() * rise_ref.W_BOUND).all()

    two = torch.from_numpy(sal0).to(dev)                            # the 5 rows as 2 + 3, accumulating in place
    eng.rise_saliency_accumulate(cells_d[:2], shifts_d[:2], s, score_d[:2], two)
    eng.rise_saliency_accumulate(cells_d[2:], shifts_d[2:], s, score_d[2:], two)
    assert (two.cpu().numpy().view(np.int32) == got.view(np.int32)).all()

    w_d = torch.from_numpy(w).to(dev)                               # the explicit entry on the emulation's weights
    ex = torch.from_numpy(sal0).to(dev)
    eng.soft_saliency_accumulate(w_d, score_d, ex)
    assert (ex.cpu().numpy().view(np.int32) == got.view(np.int32)).all()
    ex2 = torch.from_numpy(sal0).to(dev)
    eng.soft_saliency_accumulate(w_d[:2], score_d[:2], ex2)
    eng.soft_saliency_accumulate(w_d[2:], score_d[2:], ex2)
    assert (ex2.cpu().numpy().view(np.int32) == got.view(np.int32)).all()


def test_saliency_over_more_than_one_tile(eng, dev):
    """33 masks: the RISE entry restages its LDS tile once; the bits are still the emulation's."""
    m = _lib.SOFTMASK_TILE + 1
    cells, shifts = rise_ref.draws(32, m, seed=77)
    w = masks.rise_weights(cells, shifts, 32)
    scores = np.random.default_rng(8).standard_normal(m).astype(np.float32)
    sal = torch.zeros(IMG, IMG, dtype=torch.float32, device=dev)
    eng.rise_saliency_accumulate(torch.from_numpy(cells).to(dev), torch.from_numpy(shifts).to(dev), 32, torch.from_numpy(scores).to(dev), sal)
    want = rise_ref.saliency_emulation(np.zeros((IMG, IMG), np.float32), scores, w)
    assert (sal.cpu().numpy().view(np.int32) == want.view(np.int32)).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------------------------
def test_score_rise_against_cpu_forward(eng, sd18, picture):
    img, x = picture
    cells, shifts = rise_ref.draws(7, 5, seed=9)
    w = masks.rise_weights(cells, shifts, 7)
    label, _ = eng.predict(img)
    score, pred = eng.score_rise(img, cells, shifts, 7, label)
    ref = [scorer.score_one(sd18, "resnet18", x.numpy() * w[m][None], label) for m in range(5)]
    ref_score, ref_pred = np.array([r[0] for r in ref]), np.array([r[1] for r in ref])
    err = float(np.abs(score - ref_score).max())
    print("score_rise max |d| against the CPU forward: %.3e" % err)
    assert err <= SCORE_TOL and (pred == ref_pred).all()


def test_rise_saliency_is_the_assembled_sum(eng, dev, picture):
    img = picture[0]
    n, s, p1, seed = 16, 7, 0.5, 3
    label, _ = eng.predict(img)
    cells, shifts = masks.rise_masks(n, s, p1, seed)
    score, _pred = eng.score_rise(img, cells, shifts, s, label)
    w = masks.rise_weights(cells, shifts, s)
    sal = eng.rise_saliency(img, label, n_masks=n, s=s, p1=p1, seed=seed)
    assert sal.dtype == np.float32 and sal.shape == (IMG, IMG)
    want = np.tensordot(score.astype(np.float64), w.astype(np.float64), 1) / (n * p1)
    # the fp32 sum's bound, carried through the division, plus the division's own rounding
    bound = rise_ref.saliency_bound(np.zeros((IMG, IMG)), score, w) / (n * p1) + rise_ref.U32 * np.abs(want) * 1.001
    assert (np.abs(sal - want) <= bound).all()
    assert np.abs(want).max() > 0
    out = torch.full((IMG, IMG), 7.0, dtype=torch.float32, device=dev)             # out= is overwritten, not added to
    assert eng.rise_saliency(img, label, n_masks=n, s=s, p1=p1, seed=seed, out=out) is out
    assert (out.cpu().numpy().view(np.int32) == sal.view(np.int32)).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------------
MPX_E_ARG, MPX_E_STATE = -1, -2


def test_refusals_write_nothing(eng, dev, picture):
    lib, h = eng._lib, eng._h
    u8 = _image(picture, "u8", dev)
    f32 = _image(picture, "f32", dev)
    cells, shifts = rise_ref.draws(7, 2)
    cells_d, shifts_d = torch.from_numpy(cells).to(dev), torch.from_numpy(shifts).to(dev)
    w_d = torch.from_numpy(masks.rise_weights(cells, shifts, 7)).to(dev)
    mean, std = eng._mean, eng._std
    sal = torch.full((IMG, IMG), 3.0, dtype=torch.float32, device=dev)
    score_d = torch.ones(2, dtype=torch.float32, device=dev)
    with Planes(eng) as planes:
        rise = lambda img8, img32, c, sh, m, s, slot0: lib.mpx_rise_apply(h, _p(img8), _p(img32), _p(c), _p(sh), m, s, mean, std, slot0, None, None)
        soft = lambda img8, img32, w, m, slot0: lib.mpx_softmask_apply(h, _p(img8), _p(img32), _p(w), m, mean, std, slot0, None, None)

        def refused(rc, entry, why):
            """MPX_E_ARG, and mpx_last_error is THIS call's message: it names the entry and the reason."""
            msg = lib.mpx_last_error(h)
            assert rc == MPX_E_ARG and msg.startswith(entry + b": ") and why in msg, (rc, msg)

        sal_rise = lambda c, sh, m, s: lib.mpx_rise_saliency(h, _p(c), _p(sh), _p(score_d), m, s, _p(sal), None)
        sal_soft = lambda w, m: lib.mpx_softmask_saliency(h, _p(w), _p(score_d), m, _p(sal), None)
        for s in (1, 33, 0, -3):                                                   # s outside [2, 32]
            refused(rise(u8, None, cells_d, shifts_d, 2, s, 0), b"rise_apply", b"s=%d outside" % s)
            refused(sal_rise(cells_d, shifts_d, 2, s), b"rise_saliency", b"s=%d outside" % s)
        refused(rise(u8, None, cells_d, shifts_d, 2, 7, 7), b"rise_apply", b"slots [7,9)")             # slot0 + M > max_batch
        refused(soft(u8, None, w_d, 2, 7), b"softmask_apply", b"slots [7,9)")
        refused(rise(u8, None, cells_d, shifts_d, -1, 7, 0), b"rise_apply", b"slots [0,-1)")           # M < 0
        refused(soft(u8, None, w_d, -1, 0), b"softmask_apply", b"slots [0,-1)")
        refused(rise(u8, f32, cells_d, shifts_d, 2, 7, 0), b"rise_apply", b"exactly one of")           # both image pointers
        refused(soft(u8, f32, w_d, 2, 0), b"softmask_apply", b"exactly one of")
        refused(rise(None, None, cells_d, shifts_d, 2, 7, 0), b"rise_apply", b"exactly one of")        # neither
        refused(soft(None, None, w_d, 2, 0), b"softmask_apply", b"exactly one of")
        refused(rise(u8, None, None, shifts_d, 2, 7, 0), b"rise_apply", b"null mask pointer")          # a NULL mask pointer
        refused(rise(u8, None, cells_d, None, 2, 7, 0), b"rise_apply", b"null mask pointer")
        refused(soft(u8, None, None, 2, 0), b"softmask_apply", b"null mask pointer")
        refused(sal_soft(None, 2), b"softmask_saliency", b"null pointer")
        refused(sal_rise(None, shifts_d, 2, 7), b"rise_saliency", b"null pointer")
        refused(sal_soft(w_d, -1), b"softmask_saliency", b"M=-1")
        assert rise(u8, None, cells_d, shifts_d, 0, 7, 0) == 0                     # M == 0: success, nothing written
        assert soft(u8, None, w_d, 0, 8) == 0
        assert sal_rise(cells_d, shifts_d, 0, 7) == 0
        assert planes.intact()
    assert (sal.cpu().numpy() == 3.0).all()
    # the Python layer refuses before anything is uploaded
    bad = shifts.copy()
    bad[1, 0] = 32
    with pytest.raises(ValueError):
        eng.score_rise(picture[0], cells, bad, 7, 0)
    with pytest.raises(ValueError):
        eng.score_rise(picture[0], cells, shifts, 33, 0)
    with pytest.raises(ValueError):
        eng.score_soft_masks(picture[0], np.zeros((2, 224, 223), np.float32), 0)
    with pytest.raises(MpxError):
        eng.stage_rise(u8, cells_d, shifts_d, 7, 7)


def test_small_network_is_refused(mpx_lib, dev, picture):
    e = MaskedForwardEngine("mnist_net", max_batch=4, device=0)
    try:
        lib, h = e._lib, e._h
        u8 = _image(picture, "u8", dev)
        cells, shifts = rise_ref.draws(7, 2)
        cells_d, shifts_d = torch.from_numpy(cells).to(dev), torch.from_numpy(shifts).to(dev)
        w_d = torch.ones(2, IMG, IMG, dtype=torch.float32, device=dev)
        sal = torch.zeros(IMG, IMG, dtype=torch.float32, device=dev)
        score_d = torch.ones(2, dtype=torch.float32, device=dev)
        hi, lo = (t.view(torch.int16) for t in e.input_planes())
        before = hi.clone(), lo.clone()
        assert lib.mpx_rise_apply(h, _p(u8), None, _p(cells_d), _p(shifts_d), 2, 7, e._mean, e._std, 0, None, None) == MPX_E_STATE
        assert lib.mpx_softmask_apply(h, _p(u8), None, _p(w_d), 2, e._mean, e._std, 0, None, None) == MPX_E_STATE
        assert lib.mpx_rise_saliency(h, _p(cells_d), _p(shifts_d), _p(score_d), 2, 7, _p(sal), None) == MPX_E_STATE
        assert lib.mpx_softmask_saliency(h, _p(w_d), _p(score_d), 2, _p(sal), None) == MPX_E_STATE
        torch.cuda.synchronize()
        assert torch.equal(hi, before[0]) and torch.equal(lo, before[1]) and not sal.any()
        with pytest.raises(ValueError):
            e.score_rise(picture[0], cells, shifts, 7, 0)
    finally:
        e.close()
