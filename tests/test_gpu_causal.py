"""GPU tests of the second pixel source (csrc/mpx_rankmask.h): mpx_rank_apply against masks.rank_masks_apply BIT FOR BIT on the staged hi / lo
planes and the f32 output, against mpx_mask_apply_normalize over pseudo-segments bit for bit, mpx_blur_fill against masks.blur_fill bit for
bit, the device ranking against masks.saliency_rank, deletion_insertion against the CPU forward and against itself packed, and the refusals.
resnet18 with max_batch = 8 unless another engine is named."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_common import dev, ptr as _p  # noqa: F401  (dev is a fixture)
from network_interpretation_imagenet_amd import _lib, api, masks, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine, MpxError
from oracle import scorer
import causal_ref
import squeezenet_ref

pytestmark = pytest.mark.gpu

IMG, PAD, HW = 224, 230, 224 * 224
SENTINEL = 0x5A3C           # fp16 bits of 199.5: neither 0 nor what a normalised pixel or a unit-variance fill splits into at every element
SCORE_TOL = 1e-4            # the project's tolerance of a score against the CPU forward
MPX_E_ARG, MPX_E_STATE = -1, -2


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


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
    """Sized for one row more than rank_apply_kernel's tile (32) behind slot0 = 5, and for a 29-row curve."""
    e = MaskedForwardEngine("resnet18", max_batch=40, device=0).load_state_dict(sd18)
    yield e
    e.close()


@pytest.fixture(scope="module")
def picture():
    """(u8 HWC image, its normalised f32 CHW array): noise, so that negative normalised pixels are everywhere."""
    img = synth.make_images(2, kind="noise")[1]
    return img, scorer.to_tensor_normalize(img).numpy()


@pytest.fixture(scope="module")
def tied_rank():
    """The rank of a superpixel-constant map (every pixel tied with at least 255 others, signed zeros among them), through saliency_rank."""
    return masks.saliency_rank(causal_ref.superpixel_saliency())


@pytest.fixture(scope="module")
def noise_fill():
    return causal_ref.noise_chw(11)


class Planes:
    """The engine's input staging filled with a sentinel for the length of a `with` block, and put back afterwards (the 3-pixel border is
    zero for the life of an engine and the stem conv reads it)."""

    def __init__(self, e):
        self.e = e
        self.hi, self.lo = (t.view(torch.int16) for t in e.input_planes())

    def __enter__(self):
        self.saved = self.hi.clone(), self.lo.clone()
        self.fill()
        return self

    def fill(self):
        self.hi.fill_(SENTINEL)
        self.lo.fill_(SENTINEL)

    def __exit__(self, *exc):
        self.hi.copy_(self.saved[0])
        self.lo.copy_(self.saved[1])
        torch.cuda.synchronize()

    def read(self):
        torch.cuda.synchronize()
        return self.hi.cpu().numpy(), self.lo.cpu().numpy()

    def intact(self):
        hi, lo = self.read()
        return bool((hi == SENTINEL).all() and (lo == SENTINEL).all())


def check_planes(planes, want, slot0, out=None):
    """Slots [slot0, slot0 + M) hold split(want[m]) bit for bit in channels 0..2 and +0.0 in channel 3; their 3-pixel border and every other
    slot still hold the sentinel; out (f32[M,3,224,224]) holds want bit for bit."""
    hi, lo = planes.read()
    m = len(want)
    assert want.dtype == np.float32 and want.shape == (m, 3, IMG, IMG)
    whi, wlo = causal_ref.split16(want.transpose(0, 2, 3, 1))       # NHWC
    for name, got, exp in (("hi", hi, whi), ("lo", lo, wlo)):
        inner = got[slot0:slot0 + m, 3:3 + IMG, 3:3 + IMG]
        assert (inner[..., :3] == exp).all(), "%s plane differs from the split of the selected pixel at %d elements" % (name, int((inner[..., :3] != exp).sum()))
        assert (inner[..., 3] == 0).all(), "%s: channel 3 is not +0.0" % name
        border = got[slot0:slot0 + m].copy()
        border[:, 3:3 + IMG, 3:3 + IMG] = SENTINEL
        assert (border == SENTINEL).all(), "%s: the 3-pixel border was written" % name
        assert (got[:slot0] == SENTINEL).all() and (got[slot0 + m:] == SENTINEL).all(), "%s: a slot outside [slot0, slot0 + M) was written" % name
    if out is not None:
        assert (_bits(out.cpu().numpy()) == _bits(want)).all(), "out_f32_nchw differs from the selected pixel"


def _image(picture, kind, dev):
    img, x = picture
    return torch.from_numpy(img if kind == "u8" else x.copy()).contiguous().to(dev)


def _up(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------------------------------------------
# apply against numpy
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep_top", [False, True])
@pytest.mark.parametrize("with_fill", [False, True])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_rank_apply_bit_exact(eng, dev, picture, tied_rank, noise_fill, kind, with_fill, keep_top):
    """Thresholds 0 (nothing below), 1, one in the middle, 50175 (all but the last pixel) and 50176 (everything), into slots [2, 7) of 8."""
    thresh = np.array([0, 1, 20011, HW - 1, HW], dtype=np.int32)
    fill = noise_fill if with_fill else None
    want = masks.rank_masks_apply(picture[1], tied_rank, thresh, fill, keep_top)
    if not with_fill:
        assert (_bits(want) == np.int32(-2 ** 31)).any()            # the -0.0 of a replaced negative pixel is in the expectation
    out = torch.full((5, 3, IMG, IMG), float("nan"), dtype=torch.float32, device=dev)
    with Planes(eng) as planes:
        eng.stage_rank_masks(_image(picture, kind, dev), _up(tied_rank, dev), _up(thresh, dev), _up(fill, dev), keep_top, 2, out)
        check_planes(planes, want, 2, out)


@pytest.mark.parametrize("m,slot0", [(1, 3), (_lib.RANKMASK_TILE + 1, 5)])
def test_rank_apply_row_counts(eng, eng40, dev, picture, tied_rank, noise_fill, m, slot0):
    """One row, and one row more than a block's tile (the second tile of the launch holds a single row), behind slot0 > 0."""
    e = eng if m == 1 else eng40
    thresh = np.random.default_rng(m).integers(-5, HW + 5, size=m).astype(np.int32)      # any i32 is a threshold, below 0 and above hw too
    want = masks.rank_masks_apply(picture[1], tied_rank, thresh, noise_fill, True)
    with Planes(e) as planes:
        e.stage_rank_masks(_image(picture, "u8", dev), _up(tied_rank, dev), _up(thresh, dev), _up(noise_fill, dev), True, slot0)
        check_planes(planes, want, slot0)


# ------------------------------------------------------------------------------------------------------------------------------------
# apply against K0
# ------------------------------------------------------------------------------------------------------------------------------------
STEP = 224 * 8


def _pseudo_segments(rank):
    """Zero-fill deletion as K0 sees it: pseudo-segments rank // step, S = 28, row m keeps the segments s >= m."""
    seg = (rank // STEP).astype(np.int32)
    onoff = (np.arange(28)[None, :] >= np.arange(29)[:, None]).astype(np.uint8)
    return seg, onoff


def test_zero_fill_deletion_gives_k0_planes(eng40, dev, picture):
    rank = masks.saliency_rank(np.random.default_rng(6).standard_normal((IMG, IMG)).astype(np.float32))
    seg, onoff = _pseudo_segments(rank)
    thresh = masks.curve_thresholds(STEP)
    assert thresh.shape == (29,)
    image = _image(picture, "u8", dev)
    f_k0 = torch.empty(29, 3, IMG, IMG, dtype=torch.float32, device=dev)
    f_rank = torch.empty_like(f_k0)
    with Planes(eng40) as planes:
        eng40.stage_masks(image, _up(seg, dev), _up(onoff, dev), 4, f_k0)
        k0_hi, k0_lo = planes.read()
        planes.fill()
        eng40.stage_rank_masks(image, _up(rank, dev), _up(thresh, dev), None, False, 4, f_rank)
        hi, lo = planes.read()
    assert (hi == k0_hi).all() and (lo == k0_lo).all()              # all 40 slots, sentinels included
    assert (_bits(f_k0.cpu().numpy()) == _bits(f_rank.cpu().numpy())).all()
    assert (hi[4:33, 3:227, 3:227, :3] == np.int16(-2 ** 15)).any()  # hi -0.0: removed negative pixels are among them


def test_score_rank_masks_equals_score_masks(eng, picture):
    """29 rows on the 8-slot engine: four forwards."""
    img = picture[0]
    rank = masks.saliency_rank(np.random.default_rng(6).standard_normal((IMG, IMG)).astype(np.float32))
    seg, onoff = _pseudo_segments(rank)
    thresh = masks.curve_thresholds(STEP)
    label, _ = eng.predict(img)
    _o, score, pred, logits = eng.score_masks(img, seg, onoff, label, return_logits=True, stem="conv")
    r_score, r_pred, r_logits = eng.score_rank_masks(img, rank, thresh, label, return_logits=True)
    assert (_bits(score) == _bits(r_score)).all() and (pred == r_pred).all() and (_bits(logits) == _bits(r_logits)).all()
    _o, score2, pred2 = eng.score_masks(img, seg, onoff, label, stem="conv")
    r_score2, r_pred2 = eng.score_rank_masks(img, rank, thresh, label)
    assert (_bits(score2) == _bits(r_score2)).all() and (pred2 == r_pred2).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# blur and ranking
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("klen", causal_ref.KLEN_CASES)
def test_blur_fill_bit_exact(eng, dev, picture, klen, kind):
    taps = causal_ref.taps_for(klen)
    want = masks.blur_fill(picture[1], taps)
    n = 3 * HW
    buf = torch.full((n + 2 * 512,), float("nan"), dtype=torch.float32, device=dev)     # the output between two NaN guards
    out = buf[512:512 + n].view(3, IMG, IMG)
    assert eng.blur_fill(_image(picture, kind, dev), taps, out=out) is out
    got = buf.cpu().numpy()
    assert np.isnan(got[:512]).all() and np.isnan(got[512 + n:]).all(), "a guard element was written"
    diff = _bits(got[512:512 + n]) != _bits(want).ravel()
    assert not diff.any(), "klen=%d: differs from masks.blur_fill at %d of %d elements" % (klen, int(diff.sum()), n)
    if klen == 1:
        assert (_bits(want) == _bits(picture[1])).all()             # one tap of 1.0 returns the normalised image


def test_blur_fill_defaults_to_rises_gaussian(eng, picture):
    got = eng.blur_fill(picture[0])
    assert (_bits(got.cpu().numpy()) == _bits(masks.blur_fill(picture[1], masks.gaussian_taps(11, 5.0)))).all()


def test_device_saliency_rank(eng, dev):
    """Ties (a superpixel-constant map with +0.0 and -0.0 superpixels) and a map of distinct values."""
    for sal in (causal_ref.superpixel_saliency(), np.random.default_rng(2).standard_normal((IMG, IMG)).astype(np.float32)):
        got = eng.saliency_rank(torch.from_numpy(sal).to(dev))
        assert got.dtype == torch.int32 and tuple(got.shape) == (IMG, IMG) and got.is_contiguous()
        assert (got.cpu().numpy() == masks.saliency_rank(sal)).all()
    zeros = np.zeros((IMG, IMG), dtype=np.float32)
    zeros.ravel()[::3] = -0.0
    assert (eng.saliency_rank(torch.from_numpy(zeros).to(dev)).cpu().numpy().ravel() == np.arange(HW)).all()
    bad = torch.zeros(IMG, IMG, dtype=torch.float32, device=dev)
    bad[7, 7] = float("nan")
    with pytest.raises(ValueError):
        eng.saliency_rank(bad)


# ------------------------------------------------------------------------------------------------------------------------------------
# deletion_insertion
# ------------------------------------------------------------------------------------------------------------------------------------
def test_deletion_insertion_ends_and_aucs(eng40, dev, picture):
    """Deletion row 0 and insertion's last row are the whole image: they carry the score bits of score_masks' all-on row (conv staging)."""
    img = picture[0]
    sal = np.random.default_rng(9).standard_normal((IMG, IMG)).astype(np.float32)
    label, _ = eng40.predict(img)
    res = eng40.deletion_insertion(img, sal, label)
    assert (res["thresholds"] == masks.curve_thresholds(STEP)).all()
    for key, dt in (("del_scores", np.float32), ("ins_scores", np.float32), ("del_pred", np.int32), ("ins_pred", np.int32)):
        assert res[key].dtype == dt and res[key].shape == (29,)
    _o, whole, whole_pred = eng40.score_masks(img, np.zeros((IMG, IMG), np.int32), np.ones((1, 1), np.uint8), label, stem="conv")
    assert _bits(res["del_scores"])[0] == _bits(res["ins_scores"])[-1] == _bits(whole)[0]
    assert res["del_pred"][0] == res["ins_pred"][-1] == whole_pred[0]
    assert res["del_auc"] == masks.curve_auc(res["del_scores"]) and res["ins_auc"] == masks.curve_auc(res["ins_scores"])
    # a device map (what rise_saliency(out=...) returns) gives the same curves, and so does the api
    res_d = api.deletion_insertion(eng40, img, torch.from_numpy(sal).to(dev), label)
    for key in ("del_scores", "ins_scores", "del_pred", "ins_pred"):
        assert (_bits(res_d[key]) == _bits(res[key])).all()


def _cpu_curves(score_one, x, sal, label, step, taps):
    rank, thresh = masks.saliency_rank(sal), masks.curve_thresholds(step)
    dele = masks.rank_masks_apply(x, rank, thresh, None, False)
    ins = masks.rank_masks_apply(x, rank, thresh, masks.blur_fill(x, taps), True)
    return [np.array([score_one(row, label) for row in rows]) for rows in (dele, ins)]


def _check_e2e(e, score_one, picture):
    img, x = picture
    sal = np.random.default_rng(12).standard_normal((IMG, IMG)).astype(np.float32)
    label, _ = e.predict(img)
    res = e.deletion_insertion(img, sal, label, step=224 * 56)      # 5 + 5 rows
    want_del, want_ins = _cpu_curves(score_one, x, sal, label, 224 * 56, masks.gaussian_taps())
    for name, got, want in (("deletion", res["del_scores"], want_del), ("insertion", res["ins_scores"], want_ins)):
        assert got.shape == (5,)
        err = float(np.abs(got - want[:, 0]).max())
        print("%s %s max |d| against the CPU forward: %.3e" % (e.arch, name, err))
        assert err <= SCORE_TOL
    assert (res["del_pred"] == want_del[:, 1]).all() and (res["ins_pred"] == want_ins[:, 1]).all()


def test_deletion_insertion_against_cpu_forward_resnet18(eng, sd18, picture):
    _check_e2e(eng, lambda row, label: scorer.score_one(sd18, "resnet18", row, label), picture)


def test_deletion_insertion_against_cpu_forward_squeezenet(mpx_lib, dev, picture):
    sd = synth.make_state_dict("squeezenet1_1")
    sd32 = squeezenet_ref.cast(sd, torch.float32)

    def score_one(row, label):
        with torch.no_grad():
            logits = squeezenet_ref.forward(sd32, torch.from_numpy(row[None]))
        return F.softmax(logits, 1).numpy()[0][label], int(logits.argmax(1)[0])

    e = MaskedForwardEngine("squeezenet1_1", max_batch=4, device=0).load_state_dict(sd)
    try:
        _check_e2e(e, score_one, picture)
    finally:
        e.close()


@pytest.mark.parametrize("step,rows", [(224 * 32, 16), (224 * 15, 32)])
def test_packed_curves_equal_each_image_alone(eng40, dev, step, rows):
    """3 images in forwards of 40 slots.  step 224 * 32: 16 rows an image (8 + 8), 48 rows, the third image straddles the batch boundary
    (its deletion rows end one forward, its insertion rows are the next).  step 224 * 15: 32 rows an image (16 + 16, the last step short),
    96 rows, the boundary at row 40 cuts the second image's deletion curve in two: one mpx_rank_apply per row range.  A device map, a fill
    image for deletion and a label that is not the prediction are in the mix."""
    imgs = list(synth.make_images(3, kind="noise"))
    rng = np.random.default_rng(13)
    sals = [rng.standard_normal((IMG, IMG)).astype(np.float32) for _ in range(3)]
    sals[1] = torch.from_numpy(sals[1]).to(dev)
    labels = [int(eng40.predict(im)[0]) for im in imgs]
    labels[2] = (labels[2] + 1) % 1000
    assert 2 * masks.curve_thresholds(step).size == rows and 3 * rows > eng40.max_batch
    del_fill = causal_ref.noise_chw(14)
    packed = api.deletion_insertion_many(eng40, imgs, sals, labels, step=step, del_fill=del_fill)
    assert len(packed) == 3
    for i in range(3):
        alone = eng40.deletion_insertion(imgs[i], sals[i], labels[i], step=step, del_fill=del_fill)
        for key in ("thresholds", "del_scores", "ins_scores", "del_pred", "ins_pred"):
            assert (_bits(packed[i][key]) == _bits(alone[key])).all(), (i, key)
        assert packed[i]["del_auc"] == alone["del_auc"] and packed[i]["ins_auc"] == alone["ins_auc"]
    assert eng40.deletion_insertion_many([], [], []) == []


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(eng, dev, picture, tied_rank):
    lib, h = eng._lib, eng._h
    u8, f32 = _image(picture, "u8", dev), _image(picture, "f32", dev)
    rank_d = _up(tied_rank, dev)
    thresh_d = _up(np.array([5, 500], dtype=np.int32), dev)
    mean, std = eng._mean, eng._std
    taps = causal_ref.taps_for(3)
    taps_p = taps.ctypes.data_as(C.POINTER(C.c_float))
    out = torch.full((3, IMG, IMG), 3.0, dtype=torch.float32, device=dev)

    def refused(rc, entry, why):
        """MPX_E_ARG, and mpx_last_error is THIS call's message: it names the entry and the reason."""
        msg = lib.mpx_last_error(h)
        assert rc == MPX_E_ARG and msg.startswith(entry + b": ") and why in msg, (rc, msg)

    with Planes(eng) as planes:
        rank = lambda img8, img32, r, t, m, keep_top, slot0: lib.mpx_rank_apply(h, _p(img8), _p(img32), _p(r), _p(t), m, None, keep_top, mean, std,
                                                                              slot0, None, None)
        blur = lambda img8, img32, t, klen, o: lib.mpx_blur_fill(h, _p(img8), _p(img32), t, klen, mean, std, _p(o), None)
        refused(rank(u8, f32, rank_d, thresh_d, 2, 0, 0), b"rank_apply", b"exactly one of")            # both image pointers
        refused(rank(None, None, rank_d, thresh_d, 2, 0, 0), b"rank_apply", b"exactly one of")         # neither
        refused(rank(u8, None, None, thresh_d, 2, 0, 0), b"rank_apply", b"null rank or thresh")        # a NULL rank / thresh
        refused(rank(u8, None, rank_d, None, 2, 0, 0), b"rank_apply", b"null rank or thresh")
        refused(rank(u8, None, rank_d, thresh_d, -1, 0, 0), b"rank_apply", b"slots [0,-1)")            # M < 0
        refused(rank(u8, None, rank_d, thresh_d, 2, 0, 7), b"rank_apply", b"slots [7,9)")              # slot0 + M > max_batch
        for keep_top in (2, -1):
            refused(rank(u8, None, rank_d, thresh_d, 2, keep_top, 0), b"rank_apply", b"keep_top=%d" % keep_top)
        assert rank(u8, None, rank_d, thresh_d, 0, 0, 0) == 0                      # M == 0: success, nothing written
        assert rank(u8, None, rank_d, thresh_d, 0, 1, 8) == 0
        refused(blur(u8, f32, taps_p, 3, out), b"blur_fill", b"exactly one of")
        refused(blur(None, None, taps_p, 3, out), b"blur_fill", b"exactly one of")
        refused(blur(u8, None, None, 3, out), b"blur_fill", b"null taps or out")
        refused(blur(u8, None, taps_p, 3, None), b"blur_fill", b"null taps or out")
        for klen in (0, 2, 30, 33, -3):
            refused(blur(u8, None, taps_p, klen, out), b"blur_fill", b"klen=%d" % klen)
        before = f32.clone()
        refused(blur(None, f32, taps_p, 3, f32), b"blur_fill", b"must not be the image")
        assert planes.intact()
        assert torch.equal(f32, before)
    assert (out.cpu().numpy() == 3.0).all()
    # the Python layer: dtype, shape, device, step
    img, x = picture
    thresh = np.array([5, 500], dtype=np.int32)
    with pytest.raises(ValueError):
        eng.score_rank_masks(img, tied_rank.astype(np.int64), thresh, 0)
    with pytest.raises(ValueError):
        eng.score_rank_masks(img, tied_rank[:, :223], thresh, 0)
    with pytest.raises(ValueError):
        eng.score_rank_masks(img, tied_rank, thresh.astype(np.int64), 0)
    with pytest.raises(ValueError):
        eng.score_rank_masks(img, tied_rank, thresh, 0, fill=x[:2])
    with pytest.raises(ValueError):
        eng.score_rank_masks(img, tied_rank, thresh, 1000)
    with pytest.raises(ValueError):
        eng.stage_rank_masks(u8, torch.from_numpy(tied_rank), thresh_d)            # a host tensor where a device one is asked
    with pytest.raises(ValueError):
        eng.stage_rank_masks(u8, rank_d, thresh_d, fill=out.double())
    with pytest.raises(ValueError):
        eng.blur_fill(img, np.ones(4, np.float32))
    with pytest.raises(ValueError):
        eng.blur_fill(img, taps, out=torch.empty(3, IMG, IMG))
    sal = np.zeros((IMG, IMG), dtype=np.float32)
    for step in (0, -7):
        with pytest.raises(ValueError):
            eng.deletion_insertion(img, sal, 0, step=step)
    with pytest.raises(ValueError):
        eng.deletion_insertion(img, sal.astype(np.int32), 0)
    with pytest.raises(ValueError):
        eng.deletion_insertion(img, sal, 0, ins_fill="mean")
    with pytest.raises(ValueError):
        eng.deletion_insertion_many([img], [sal, sal], [0])
    with pytest.raises(MpxError):
        eng.stage_rank_masks(u8, rank_d, thresh_d, slot0=7)


def test_small_network_is_refused(mpx_lib, dev, picture, tied_rank):
    e = MaskedForwardEngine("mnist_net", max_batch=4, device=0)
    try:
        lib, h = e._lib, e._h
        u8 = _image(picture, "u8", dev)
        rank_d, thresh_d = _up(tied_rank, dev), _up(np.array([5, 500], dtype=np.int32), dev)
        taps = causal_ref.taps_for(3)
        out = torch.zeros(3, IMG, IMG, dtype=torch.float32, device=dev)
        hi, lo = (t.view(torch.int16) for t in e.input_planes())
        before = hi.clone(), lo.clone()
        assert lib.mpx_rank_apply(h, _p(u8), None, _p(rank_d), _p(thresh_d), 2, None, 0, e._mean, e._std, 0, None, None) == MPX_E_STATE
        assert lib.mpx_blur_fill(h, _p(u8), None, taps.ctypes.data_as(C.POINTER(C.c_float)), 3, e._mean, e._std, _p(out), None) == MPX_E_STATE
        torch.cuda.synchronize()
        assert torch.equal(hi, before[0]) and torch.equal(lo, before[1]) and not out.any()
        sal = np.zeros((IMG, IMG), dtype=np.float32)
        with pytest.raises(ValueError):
            e.deletion_insertion(picture[0], sal, 0)
        with pytest.raises(ValueError):
            e.score_rank_masks(picture[0], tied_rank, np.array([5], dtype=np.int32), 0)
        with pytest.raises(ValueError):
            e.blur_fill(picture[0])
    finally:
        e.close()
