"""GPU tests of the Score-CAM path (csrc/mpx_softmask.h MapWeights -> mpx_cam_apply; csrc/mpx_cam.h -> mpx_planes_to_chw, mpx_cam_cells,
mpx_cam_combine; mpx_pool_input): the staged planes against x * masks.cam_weights BIT FOR BIT, the normalised cells and the combined maps
against masks.cam_cells / cam_combine bit for bit, the tap on hand-written planes exactly and after a forward against the CPU trunks
(reference against reference, factor 4), the scores against the explicit-weights path bit for bit and against the CPU forward, score_cam()
against its parts, and the refusals.  resnet18 and squeezenet1_1 at max_batch = 40 (one row more than the apply kernel's tile behind
slot0 = 5), mobilenet_v2 for the pool that clamps on load; the noise picture, so that negative normalised pixels are everywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_common import SCORE_TOL, Planes, check_planes, dev, ptr as _p  # noqa: F401  (dev is a fixture)
from network_interpretation_imagenet_amd import _lib, api, masks, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine, MpxError
from oracle import resnet_ref, scorer
import mobilenet_ref
import scorecam_ref as ref
import squeezenet_ref

pytestmark = pytest.mark.gpu

IMG = 224
MPX_E_ARG, MPX_E_STATE = -1, -2
FACTOR = 4.0        # logits_lens.FACTOR: |engine - fp64| <= 4 x |fp32 CPU - fp64|


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.shape == want.shape and bool((_bits(got) == _bits(want)).all())


@pytest.fixture(scope="module")
def sd18():
    return synth.make_state_dict("resnet18")


@pytest.fixture(scope="module")
def eng(mpx_lib, dev, sd18):
    e = MaskedForwardEngine("resnet18", max_batch=40, device=0).load_state_dict(sd18)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sd_sq():
    return synth.make_state_dict("squeezenet1_1")


@pytest.fixture(scope="module")
def eng_sq(mpx_lib, dev, sd_sq):
    e = MaskedForwardEngine("squeezenet1_1", max_batch=40, device=0).load_state_dict(sd_sq)
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


def _nan_out(m, dev):
    return torch.full((m, 3, IMG, IMG), float("nan"), dtype=torch.float32, device=dev)


# ------------------------------------------------------------------------------------------------------------------------------------
# apply
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("g", ref.GRIDS)
def test_apply_one_row_bit_exact(eng, dev, picture, g, kind):
    """M = 1 behind slot 3: the row with an exact 0.0, an exact 1.0, a cell below 0 and one above 1."""
    cells = ref.cells(2, g)[:1]
    w = masks.cam_weights(cells)
    assert w.min() == 0.0 and w.max() == 1.0 and cells.min() < 0 and cells.max() > 1
    out = _nan_out(1, dev)
    with Planes(eng) as planes:
        eng.stage_cam(_image(picture, kind, dev), torch.from_numpy(cells).to(dev), 3, out)
        check_planes(planes, picture[1], w, 3, out)


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("g", ref.GRIDS)
def test_apply_one_row_past_the_tile_bit_exact(eng, dev, picture, g, kind):
    """M = 33 at slot0 = 5: a second tile of one row (the all-ones row); slots 0 .. 4 and 38, 39 stay as they were."""
    cells = ref.cells(33, g)
    assert len(cells) == _lib.SOFTMASK_TILE + 1 and eng.max_batch == 40
    w = masks.cam_weights(cells)
    out = _nan_out(33, dev) if kind == "u8" else None
    with Planes(eng) as planes:
        eng.stage_cam(_image(picture, kind, dev), torch.from_numpy(cells).to(dev), 5, out)
        check_planes(planes, picture[1], w, 5, out)


def test_apply_all_ones_is_the_unmasked_staging(eng, dev, picture):
    u8 = _image(picture, "u8", dev)
    ones = torch.ones(1, 7, 7, dtype=torch.float32, device=dev)
    with Planes(eng) as planes:
        eng.stage_cam(u8, ones, 0)
        got = tuple(a[:1].copy() for a in planes.read())
    with Planes(eng) as planes:
        eng.stage_boxes(u8, torch.zeros(1, 4, dtype=torch.int32, device=dev), 0)       # the empty box: nothing covered
        want = tuple(a[:1].copy() for a in planes.read())
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# cells
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", ref.GRIDS)
@pytest.mark.parametrize("c", [1, 5, 257])
def test_cells_bit_exact(eng, dev, c, g):
    """The interior peak (channel 0: the upsampled maximum lies below the cell), then constant, all-zero, negative and mixed channels."""
    act = ref.activations(c, g)
    want = masks.cam_cells(act)
    cells, lo, hi, valid = eng.cam_cells(torch.from_numpy(act).to(dev))
    assert valid.dtype == torch.uint8 and (valid.cpu().numpy() == want[3]).all()
    assert _same(lo, want[1]) and _same(hi, want[2])
    assert _same(cells, want[0]), int((_bits(cells.cpu().numpy()) != _bits(want[0])).sum())
    if g > 2:
        assert float(hi[0]) < float(act[0].max())
    if c > 3:
        assert valid.cpu().numpy()[:4].tolist() == [1, 0, 0, 1]


# ------------------------------------------------------------------------------------------------------------------------------------
# the tap
# ------------------------------------------------------------------------------------------------------------------------------------
def _hand_planes(side, channels, pitch, seed):
    """(hi, lo) fp16 [3][side * side][pitch]: values on both sides of 0 and of 6; the pad channels hold a sentinel."""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal((3, side * side, pitch)) * 4.0).astype(np.float32)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    hi[:, :, channels:], lo[:, :, channels:] = 777.0, 0.5
    return hi, lo


@pytest.mark.parametrize("load", [0, 1, 2])
@pytest.mark.parametrize("slot", [0, 2])
@pytest.mark.parametrize("side, channels, pitch", [(7, 5, 32), (13, 40, 64)])
def test_planes_to_chw_on_hand_written_planes(eng, dev, side, channels, pitch, slot, load):
    hi, lo = _hand_planes(side, channels, pitch, 10 * side + load)
    x = hi[slot, :, :channels].astype(np.float32) + lo[slot, :, :channels].astype(np.float32)      # fp32: one rounded sum
    out = torch.full((channels + 1, side, side), -5.0, dtype=torch.float32, device=dev)
    hi_d, lo_d = torch.from_numpy(hi).to(dev), torch.from_numpy(lo).to(dev)
    rc = eng._lib.mpx_planes_to_chw(eng._h, _p(hi_d), _p(lo_d), slot, side, channels, pitch, load, _p(out), None)
    assert rc == 0, eng._lib.mpx_last_error(eng._h)
    got = out.cpu().numpy()
    assert (got[channels] == -5.0).all()                            # nothing behind the C logical channels
    got = got[:channels].reshape(channels, side * side).T
    assert np.abs(got).max() < 100                                  # no pad channel (777.5) came through
    if load == 0:
        assert (_bits(got) == _bits(x)).all()
    elif load == 1:
        assert (x > 6).any() and (_bits(got) == _bits(np.minimum(x, np.float32(6.0)))).all()
    else:
        x64 = x.astype(np.float64)
        want = x64 / (1.0 + np.exp(-x64))
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - want) <= 4 * ulp).all()


def _three_rows(e, dev, picture, g):
    """Stage three masked rows, run them -> (inputs f32[3,3,224,224] as the engine staged them, logits f32[3,1000])."""
    cells = ref.cells(3, g, seed=5)
    out = _nan_out(3, dev)
    e.stage_cam(_image(picture, "u8", dev), torch.from_numpy(cells).to(dev), 0, out)
    logits = e.forward(3, torch.zeros(3, dtype=torch.int32, device=dev), want_logits=True)[2]
    return out.cpu(), logits.cpu().numpy()


def _tap_rule(name, taps, want32, want64):
    d_cpu = float(np.abs(want32.astype(np.float64) - want64).max())
    d_eng = float(np.abs(taps.astype(np.float64) - want64).max())
    print("%s tap: |map| up to %.2f, fp32 CPU vs fp64 %.3e, engine vs fp64 %.3e" % (name, np.abs(want64).max(), d_cpu, d_eng))
    assert d_cpu > 0 and d_eng <= FACTOR * d_cpu


def test_pool_input_resnet18_against_layer4(eng, dev, sd18, picture):
    x, _logits = _three_rows(eng, dev, picture, 7)
    taps = np.stack([eng.pool_input(s).cpu().numpy() for s in range(3)])
    assert taps.shape == (3, 512, 7, 7) and taps.dtype == np.float32
    t32, t64 = {}, {}
    with torch.no_grad():
        resnet_ref.forward(sd18, x, "resnet18", taps=t32)
        resnet_ref.forward(resnet_ref.cast_state_dict(sd18, torch.float64), x.double(), "resnet18", taps=t64)
    _tap_rule("resnet18", taps, t32["layer4.1"].numpy(), t64["layer4.1"].numpy())
    with pytest.raises(ValueError):
        eng.pool_input(3)                                           # the last forward ran slots 0 .. 2
    with pytest.raises(ValueError):
        eng.pool_input(-1)


def test_pool_input_mobilenet_v2_applies_the_clamp(mpx_lib, dev, picture):
    sd = synth.make_state_dict("mobilenet_v2")
    e = MaskedForwardEngine("mobilenet_v2", max_batch=4, device=0).load_state_dict(sd)
    try:
        x, _logits = _three_rows(e, dev, picture, 7)
        taps = np.stack([e.pool_input(s).cpu().numpy() for s in range(3)])
        assert taps.shape == (3, 1280, 7, 7) and taps.max() <= 6.0 and taps.min() >= 0.0
        with torch.no_grad():
            w32 = mobilenet_ref.features(sd, x).numpy()
            w64 = mobilenet_ref.features(mobilenet_ref.netref.cast(sd, torch.float64), x.double()).numpy()
        _tap_rule("mobilenet_v2", taps, w32, w64)
    finally:
        e.close()


def test_pool_input_squeezenet_means_are_the_logits(eng_sq, dev, sd_sq, picture):
    x, logits = _three_rows(eng_sq, dev, picture, 13)
    taps = np.stack([eng_sq.pool_input(s).cpu().numpy() for s in range(3)])
    assert taps.shape == (3, 1000, 13, 13) and (taps >= 0).all()
    with torch.no_grad():
        l32 = squeezenet_ref.forward(sd_sq, x).numpy()
        l64 = squeezenet_ref.forward(squeezenet_ref.cast(sd_sq, torch.float64), x.double()).numpy()
    _tap_rule("squeezenet1_1 (spatial mean)", taps.astype(np.float64).mean(axis=(2, 3)), l32, l64)
    assert np.abs(taps.astype(np.float64).mean(axis=(2, 3)) - logits).max() <= 1e-5 * max(1.0, np.abs(logits).max())     # the pool's own sum: 169 fp32 additions of non-negative values, 169 * 2^-24 = 1.0e-5 relative


@pytest.mark.parametrize("arch", ["vgg11", "alexnet"])
def test_pool_input_refuses_a_network_without_a_pool(mpx_lib, dev, arch):
    e = MaskedForwardEngine(arch, max_batch=1, device=0)
    try:
        with pytest.raises(MpxError) as err:
            e.pool_input(0)
        assert "no global average pool" in str(err.value)
        out = [C.c_void_p(), C.c_void_p()] + [C.c_int() for _ in range(4)]
        assert e._lib.mpx_pool_input(e._h, *[C.byref(v) for v in out]) == MPX_E_STATE
        assert ("VGG" if arch == "vgg11" else "AlexNet").encode() in e._lib.mpx_last_error(e._h)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# combine
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 5, 33])
@pytest.mark.parametrize("r, g", [(1, 2), (33, 7), (257, 13), (33, 16)])
def test_combine_bit_exact(eng, dev, r, g, k):
    """score_pitch = K + 3; scores of both signs, so that sums are negative and the ReLU writes +0.0."""
    rng = np.random.default_rng(100 * r + k)
    act = ref.activations(r, g, seed=1)
    wide = rng.standard_normal((r, k + 3)).astype(np.float32)
    want_low, want_sal = masks.cam_combine(act, wide[:, :k])
    wide_d = torch.from_numpy(wide).to(dev)
    scores_d = wide_d[:, :k]
    assert r == 1 or scores_d.stride(0) == k + 3
    low_d = torch.full((k, g, g), 9.0, dtype=torch.float32, device=dev)            # overwritten, not accumulated into
    out_d = torch.full((k, IMG, IMG), 9.0, dtype=torch.float32, device=dev)
    low, sal = eng.cam_combine(torch.from_numpy(act).to(dev), scores_d, low=low_d, out=out_d)
    assert low is low_d and sal is out_d
    assert _same(low, want_low) and _same(sal, want_sal)
    got = sal.cpu().numpy()
    assert (got >= 0).all() and not np.signbit(got).any()
    if r > 1:
        assert (got == 0).any() and (got > 0).any() and (want_low < 0).any()
    assert _same(wide_d, wide)


def test_combine_without_rows_writes_zero_maps(eng, dev):
    low, sal = eng.cam_combine(torch.empty(0, 7, 7, dtype=torch.float32, device=dev), torch.empty(0, 3, dtype=torch.float32, device=dev),
                               out=torch.full((3, IMG, IMG), 9.0, dtype=torch.float32, device=dev))
    want = masks.cam_combine(np.empty((0, 7, 7), np.float32), np.empty((0, 3), np.float32))
    assert _same(low, want[0]) and _same(sal, want[1]) and (sal == 0).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# scores: the map source against the explicit weights, and against the CPU forward
# ------------------------------------------------------------------------------------------------------------------------------------
def _scores_equal_explicit(e, picture, g):
    """44 rows: two chunks at max_batch = 40."""
    img = picture[0]
    cells = ref.cells(44, g, seed=2)
    assert e.max_batch == 40
    w = masks.cam_weights(cells)
    classes = [int(e.predict(img)[0]), 3, 999]
    scores, pred = e.score_cam_rows_classes(img, cells, classes)
    w_scores, w_pred = e.score_soft_masks_classes(img, w, classes)
    assert scores.shape == (44, 3) and (_bits(scores) == _bits(w_scores)).all() and (pred == w_pred).all()
    one, one_pred, logits = e.score_cam_rows(img, cells, classes[0], return_logits=True)
    w_one, w_one_pred, w_logits = e.score_soft_masks(img, w, classes[0], return_logits=True)
    assert (_bits(one) == _bits(w_one)).all() and (one_pred == w_one_pred).all() and (_bits(logits) == _bits(w_logits)).all()
    assert (_bits(one) == _bits(scores[:, 0])).all()
    assert len(set(one.tolist())) > 3                               # the maps move the score


def test_scores_equal_the_explicit_path_resnet18(eng, picture):
    _scores_equal_explicit(eng, picture, 7)


def test_scores_equal_the_explicit_path_squeezenet(eng_sq, picture):
    _scores_equal_explicit(eng_sq, picture, 13)


def test_scores_against_cpu_forward(eng, sd18, picture):
    img, x = picture
    cells = ref.cells(6, 7, seed=3)
    label, _ = eng.predict(img)
    score, pred = eng.score_cam_rows(img, cells, label)
    w = masks.cam_weights(cells)
    cpu = [scorer.score_one(sd18, "resnet18", x.numpy() * w[m][None], label) for m in range(6)]
    err = float(np.abs(score - np.array([r[0] for r in cpu])).max())
    print("score_cam_rows max |d| against the CPU forward: %.3e" % err)
    assert err <= SCORE_TOL and (pred == np.array([r[1] for r in cpu])).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# the driver
# ------------------------------------------------------------------------------------------------------------------------------------
def _tap_of_the_unmasked_image(e, dev, picture):
    e.stage_boxes(_image(picture, "u8", dev), torch.zeros(1, 4, dtype=torch.int32, device=dev), 0)
    logits = e.forward(1, torch.zeros(1, dtype=torch.int32, device=dev), want_logits=True)[2]
    return e.pool_input(0).cpu().numpy(), logits.cpu().numpy()[0]


def _driver_is_its_parts(e, dev, picture, c, g):
    img = picture[0]
    act, logits = _tap_of_the_unmasked_image(e, dev, picture)
    assert act.shape == (c, g, g)
    cells, _lo, _hi, valid = masks.cam_cells(act)
    keep = np.flatnonzero(valid)
    classes = [7, int(np.argmax(logits))]
    cls, channels, scores, low, sal = e.score_cam(img, classes=classes)
    assert cls.dtype == np.int32 and cls.tolist() == classes and channels.dtype == np.int32 and channels.tolist() == keep.tolist()
    assert 0 < len(keep) <= c and scores.shape == (len(keep), 2) and low.shape == (2, g, g) and sal.shape == (2, IMG, IMG)
    row_scores, _pred = e.score_cam_rows_classes(img, cells[keep], classes)
    assert (_bits(scores) == _bits(row_scores)).all()
    want_low, want_sal = masks.cam_combine(act[keep], scores)
    assert _same(low, want_low) and _same(sal, want_sal) and sal.max() > 0
    return act, classes, (cls, channels, scores, low, sal)


def test_score_cam_is_its_parts_resnet18(eng, dev, picture):
    act, classes, res = _driver_is_its_parts(eng, dev, picture, 512, 7)
    img = picture[0]
    out = torch.full((2, IMG, IMG), 7.0, dtype=torch.float32, device=dev)           # out= is overwritten and returned
    _cls, channels2, scores2, low2, sal2 = eng.score_cam(img, classes=classes, out=out)
    assert sal2 is out and _same(out, res[4]) and scores2.is_cuda and low2.is_cuda     # nothing further was downloaded
    assert _same(scores2, res[2]) and _same(low2, res[3]) and (channels2 == res[1]).all()
    given = eng.score_cam(img, classes=classes, activations=act)                        # the tap handed back in: the same job
    assert all(_same(a, b) for a, b in zip(given[2:], res[2:])) and (given[1] == res[1]).all()


def test_score_cam_is_its_parts_squeezenet(eng_sq, dev, picture):
    _driver_is_its_parts(eng_sq, dev, picture, 1000, 13)


def test_score_cam_top_classes_api_and_flat_maps(eng, dev, picture):
    img = picture[0]
    act, logits = _tap_of_the_unmasked_image(eng, dev, picture)
    some = np.ascontiguousarray(act[:24])                           # a short job: 24 channels of the tap ...
    some[5] = 1.5                                                   # ... one of them flat: skipped
    cls, channels, scores, low, sal = eng.score_cam(img, top=2, activations=some)
    assert cls.tolist() == masks.top_classes(logits, 2).tolist()
    assert 5 not in channels.tolist() and channels.tolist() == np.flatnonzero(masks.cam_cells(some)[3]).tolist()
    a = api.score_cam_saliency(eng, img, label=int(cls[0]), activations=some)
    assert a[0].tolist() == [int(cls[0])] and (a[1] == channels).all() and (_bits(a[2][:, 0]) == _bits(scores[:, 0])).all()
    assert _same(a[3][0], low[0]) and _same(a[4][0], sal[0])
    flat = np.ones((3, 7, 7), dtype=np.float32)                     # R = 0: zero maps
    cls0, channels0, scores0, low0, sal0 = eng.score_cam(img, classes=[1, 2], activations=flat)
    assert channels0.shape == (0,) and scores0.shape == (0, 2) and (low0 == 0).all() and (sal0 == 0).all() and sal0.shape == (2, IMG, IMG)
    with pytest.raises(ValueError):
        api.score_cam_saliency(eng, img, label=1, top=2)


def test_driver_refusals_leave_the_planes_intact(eng, dev, picture):
    img = picture[0]
    with Planes(eng) as planes:
        for kw in (dict(classes=[1], top=2), dict(classes=[1000]), dict(top=0), dict(classes=[1], activations=np.zeros((4, 17, 17), np.float32)),
                   dict(classes=[1], activations=np.zeros((4, 7, 7), np.float64)), dict(classes=[1], activations=np.full((4, 7, 7), np.nan, np.float32)),
                   dict(classes=[1], activations=np.zeros((0, 7, 7), np.float32))):
            with pytest.raises(ValueError):
                eng.score_cam(img, **kw)
        with pytest.raises(ValueError):
            eng.score_cam(img[:100], classes=[1], activations=np.ones((2, 7, 7), np.float32))
        with pytest.raises(ValueError):
            eng.score_cam_rows(img, np.zeros((2, 17, 17), np.float32), 0)
        with pytest.raises(ValueError):
            eng.score_cam_rows(img, np.zeros((2, 7, 7), np.float32), 1000)
        with pytest.raises(ValueError):
            eng.score_cam_rows_classes(img, np.zeros((2, 7, 7), np.float64), [0])
        assert planes.intact()


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals of the C entries
# ------------------------------------------------------------------------------------------------------------------------------------
def test_apply_refusals_write_nothing(eng, dev, picture):
    lib, h = eng._lib, eng._h
    u8, f32 = _image(picture, "u8", dev), _image(picture, "f32", dev)
    cells_d = torch.from_numpy(ref.cells(4, 7)).to(dev)
    mean, std = eng._mean, eng._std

    def call(img8=u8, img32=None, c=cells_d, m=2, g=7, slot0=0):
        return lib.mpx_cam_apply(h, _p(img8), _p(img32), _p(c), m, g, mean, std, slot0, None, None)

    with Planes(eng) as planes:
        def refused(rc, why):
            msg = lib.mpx_last_error(h)
            assert rc == MPX_E_ARG and msg.startswith(b"cam_apply: ") and why in msg, (rc, msg)

        refused(call(m=-1), b"slots [0,-1)")
        refused(call(slot0=39, m=2), b"slots [39,41)")
        refused(call(slot0=-1), b"slots [-1,1)")
        refused(call(slot0=2 ** 31 - 1, m=2), b"slots [2147483647,2147483649)")           # slot0 + M in 64 bits
        refused(call(c=None), b"null cells pointer")
        refused(call(g=1), b"g=1 outside [2, 16]")
        refused(call(g=17), b"g=17 outside [2, 16]")
        refused(call(img8=u8, img32=f32), b"exactly one of")
        refused(call(img8=None, img32=None), b"exactly one of")
        assert call(m=0) == 0 and call(m=0, slot0=40) == 0                              # M == 0: success, nothing written
        assert planes.intact()
        with pytest.raises(MpxError):
            eng.stage_cam(u8, cells_d, 37)                                              # 4 rows from slot 37 of 40
        with pytest.raises(ValueError):
            eng.stage_cam(u8, cells_d.double())
        with pytest.raises(ValueError):
            eng.stage_cam(u8, cells_d[:, :, :6])
        with pytest.raises(ValueError):
            eng.stage_cam(u8, torch.zeros(2, 17, 17, device=dev))
        assert planes.intact()


def test_cells_combine_and_tap_refusals_write_nothing(eng, dev):
    lib, h = eng._lib, eng._h
    act = torch.from_numpy(ref.activations(6, 7)).to(dev)
    cells = torch.full((6, 7, 7), 3.0, dtype=torch.float32, device=dev)
    lo, hi = torch.full((6,), 3.0, device=dev), torch.full((6,), 3.0, device=dev)
    valid = torch.full((6,), 3, dtype=torch.uint8, device=dev)
    scores = torch.ones(6, 4, dtype=torch.float32, device=dev)
    low = torch.full((4, 7, 7), 3.0, dtype=torch.float32, device=dev)
    sal = torch.full((4, IMG, IMG), 3.0, dtype=torch.float32, device=dev)
    planes = torch.zeros(2, 49, 32, dtype=torch.float16, device=dev)
    chw = torch.full((5, 7, 7), 3.0, dtype=torch.float32, device=dev)

    def do_cells(a=act, c=6, g=7, ce=cells, l=lo, hh=hi, v=valid):
        return lib.mpx_cam_cells(h, _p(a), c, g, _p(ce), _p(l), _p(hh), _p(v), None)

    def do_combine(a=act, s=scores, pitch=4, r=6, g=7, k=4, lw=low, sl=sal):
        return lib.mpx_cam_combine(h, _p(a), _p(s), pitch, r, g, k, _p(lw), _p(sl), None)

    def do_tap(a=planes, b=planes, slot=0, side=7, ch=5, pitch=32, load=0, out=chw):
        return lib.mpx_planes_to_chw(h, _p(a), _p(b), slot, side, ch, pitch, load, _p(out), None)

    def refused(rc, prefix):
        msg = lib.mpx_last_error(h)
        assert rc == MPX_E_ARG and msg.startswith(prefix), (rc, msg)

    for kw in (dict(a=None), dict(ce=None), dict(l=None), dict(hh=None), dict(v=None), dict(c=-1), dict(g=1), dict(g=17)):
        refused(do_cells(**kw), b"cam_cells: ")
    for kw in (dict(a=None), dict(s=None), dict(lw=None), dict(sl=None), dict(r=-1), dict(k=0), dict(k=-2), dict(pitch=3), dict(g=1), dict(g=17)):
        refused(do_combine(**kw), b"cam_combine: ")
    for kw in (dict(a=None), dict(b=None), dict(out=None), dict(slot=-1), dict(slot=40), dict(side=0), dict(side=225), dict(ch=-1), dict(ch=33),
               dict(pitch=0), dict(load=-1), dict(load=3)):
        refused(do_tap(**kw), b"planes_to_chw: ")
    assert do_cells(c=0) == 0 and do_tap(ch=0) == 0                 # a count of zero: success, nothing written
    torch.cuda.synchronize()
    for t in (cells, lo, hi, low, sal, chw):
        assert (t == 3.0).all()
    assert (valid == 3).all()
    with pytest.raises(ValueError):
        eng.cam_cells(act.double())
    with pytest.raises(ValueError):
        eng.cam_cells(torch.zeros(3, 17, 17, device=dev))
    with pytest.raises(ValueError):
        eng.cam_combine(act, scores[:5])
    with pytest.raises(ValueError):
        eng.cam_combine(act, scores, low=low[:3])
    with pytest.raises(ValueError):
        eng.cam_combine(act, scores, out=sal[:3])


def test_small_network_is_refused(mpx_lib, dev, picture):
    e = MaskedForwardEngine("mnist_net", max_batch=4, device=0)
    try:
        u8 = _image(picture, "u8", dev)
        cells_d = torch.from_numpy(ref.cells(2, 7)).to(dev)
        hi, lo = (t.view(torch.int16) for t in e.input_planes())
        before = hi.clone(), lo.clone()
        assert e._lib.mpx_cam_apply(e._h, _p(u8), None, _p(cells_d), 2, 7, e._mean, e._std, 0, None, None) == MPX_E_STATE
        out = torch.zeros(2, 7, 7, dtype=torch.float32, device=dev)
        v = torch.zeros(2, dtype=torch.float32, device=dev)
        v8 = torch.zeros(2, dtype=torch.uint8, device=dev)
        sal = torch.zeros(1, IMG, IMG, dtype=torch.float32, device=dev)
        assert e._lib.mpx_cam_cells(e._h, _p(cells_d), 2, 7, _p(out), _p(v), _p(v), _p(v8), None) == MPX_E_STATE
        assert e._lib.mpx_cam_combine(e._h, _p(cells_d), _p(v), 1, 2, 7, 1, _p(out), _p(sal), None) == MPX_E_STATE
        torch.cuda.synchronize()
        assert torch.equal(hi, before[0]) and torch.equal(lo, before[1]) and (out == 0).all() and (sal == 0).all()
        with pytest.raises(MpxError):
            e.pool_input(0)
        with pytest.raises(ValueError):
            e.score_cam(picture[0], classes=[0], activations=np.ones((2, 7, 7), np.float32))
        with pytest.raises(ValueError):
            e.score_cam_rows(picture[0], ref.cells(2, 7), 0)
    finally:
        e.close()
