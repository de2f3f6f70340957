"""The fused launches of the benchmarked ResNet path at their edges (run on the MI355X box: pytest -m gpu): layer1's block tails
(mpx_bottleneck_tail: BtHeadC64, BtDualC64, BtResC64, BtResC128), layer2's pointwise tails (mpx_pointwise_tail: BtPw128) and the ImageNet stem,
as mpx_conv_bn_act on layer 0 from the staged input and as mpx_stem_conv_maxpool.

Every OUTPUT plane is [front fence | payload | back fence] prefilled with the sentinel 0x7e00 (test_gpu_conv_edges.Fenced): after a launch
both fences are intact bit for bit and no sentinel is left in the payload.  Every INPUT plane (t1, x, t2) sits between NaN fences of the same
size: a halo row, a dead lane or a ragged tile that reads outside its image or its M and uses the value puts a NaN into the payload, and every
comparison here fails on a NaN.  Batches come from fused_edge_draws (workgroups without a tile, with a second and a third tile; the smallest and
the largest ragged pointwise tile, a launch that ends on a tile boundary, second tiles).  Bounds (fused_edge_draws): every output
one layer away from planes the test can see takes conv_edge_draws' tol = C_TOL 2^-22 B + 2^-24 -- the next conv1 of either tail against the fp64
conv1' of the launch's OWN stored block output --, the block tail's block output C_CHAIN against the fp64 chain, the pooled stem the largest tol
of its window; the older max norm stays as a second assertion, and clearly negative pre-activations must be +0 in both planes.  References are
built on the device in fp64, once per (form, batch).  On an MI355X the file's 46 tests take 10 s; the slowest is the first block-tail launch (0.8 s)
behind 2.6 s of set-up for the trained-like engine."""

import pytest
import torch

import conv_edge_draws as ced
import fused_edge_draws as fed
from gpu_common import dev, Fenced, ptr as _p  # noqa: F401  (dev is a fixture)
from network_interpretation_imagenet_amd import _lib, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine

pytestmark = pytest.mark.gpu

WORST = {}                              # form -> (worst err / tol, where)
CONFIGS = {(0, True): "BtHeadC64", (0, False): "BtDualC64", (1, False): "BtResC64", (2, False): "BtResC128"}
WHICH = ("one image", "second tiles", "third tiles")
PT_WHICH = ("ragged 16", "ragged 112", "whole tiles", "second tiles")


def _engine(arch, sd):
    return MaskedForwardEngine(arch, max_batch=8, device=0).load_state_dict(sd)


@pytest.fixture(scope="module")
def eng50(dev):
    sd = synth.make_state_dict("resnet50")
    e = _engine("resnet50", sd)
    yield e, sd
    e.close()


@pytest.fixture(scope="module")
def eng101(dev):
    sd = synth.make_state_dict("resnet101")
    e = _engine("resnet101", sd)
    yield e, sd
    e.close()


@pytest.fixture(scope="module")
def trained(dev):
    from oracle import trained_like
    sd = trained_like.make_trained_like_state_dict("resnet101")
    e = _engine("resnet101", sd)
    yield e, sd
    e.close()


class NanFenced:
    """An input plane between two fences of FENCE_ROWS pixel rows of NaNs."""

    def __init__(self, t):
        c, n = t.shape[-1], t.numel()
        fence = ced.FENCE_ROWS * c
        self.buf = torch.full((2 * fence + n,), float("nan"), dtype=torch.float16, device=t.device)
        self.payload = self.buf[fence:fence + n]
        self.payload.copy_(t.reshape(-1))
        assert self.payload.data_ptr() % 16 == 0


def _check(what, form, hi, lo, pre, want, tol, c_name):
    """The checks of one output (hi / lo: Fenced planes) against its fp64 reference [rows][cout] and per-element tol."""
    for plane, which in ((hi, "hi"), (lo, "lo")):
        assert plane.problems() == [], "%s, %s plane: %s" % (what, which, "; ".join(plane.problems()))
    got = hi.payload.double() + lo.payload.double()
    assert not torch.isnan(got).any(), "%s: NaN in the payload (a read outside an input plane was used)" % what
    err = (got - want).abs()
    ratio = (err / tol).max().item()
    worst = torch.argmax(err / tol).item()
    print("%s: worst err / tol %.3f (%s; pixel row %d, channel %d); max norm %.2e" % (what, ratio, c_name, worst // want.shape[1], worst % want.shape[1],
                                                                                    err.max().item() / max(want.abs().max().item(), 1.0)))
    if not ratio <= WORST.get(form, (0.0, ""))[0]:
        WORST[form] = (ratio, what)
    over = int((~(err <= tol)).sum())                               # (plain numbers in the asserts: a failure must not print tensors of this size)
    assert over == 0, "%s: %d elements over their bound, worst err / tol %.3f at pixel row %d, channel %d" % (
        what, over, ratio, worst // want.shape[1], worst % want.shape[1])
    assert ced.max_norm_ok(got, want), what                         # the suite's older check, kept
    if pre is not None:
        _check_zeros(what, hi, lo, pre < -tol)


def _check_zeros(what, hi, lo, surely_zero):
    """Exact +0 in both planes wherever the fp64 pre-activation is clearly negative."""
    n = int(surely_zero.sum())
    assert n > 0, what
    bad_hi, bad_lo = int((hi.payload_bits[surely_zero] != 0).sum()), int((lo.payload_bits[surely_zero] != 0).sum())
    assert bad_hi == 0 and bad_lo == 0, "%s: of %d clearly negative pre-activations %d are not +0 in hi (bits %#06x, ...), %d not in lo" % (
        what, n, bad_hi, int(hi.payload_bits[surely_zero][hi.payload_bits[surely_zero] != 0][0]) & 0xffff if bad_hi else 0, bad_lo)


def _check_next(what, form, sd, dn, oh, ol, zh, zl, batch):
    """The next block's conv1 against the fp64 conv1' of the block output the launch stored: a single layer, C_TOL."""
    out = ced.merge(oh.payload, ol.payload).view(batch, dn.hin, dn.hin, dn.cin)
    pre, want, b = (q.view(-1, dn.cout) for q in fed.next_reference(sd, dn, out))
    _check(what + ", next conv1", form + " next conv1", zh, zl, pre, want, ced.tol(b), "C_TOL")


# ------------------------------------------------------------------------------------------------
# block tails
# ------------------------------------------------------------------------------------------------
def _tail_layers(eng, k):
    t = fed.block_tail(k)
    c2, c3, ds, n1 = eng.bottleneck_tails()[k]
    as_d = lambda i: ced.as_desc(eng.layers[i])
    assert (as_d(c2 - 1), as_d(c2), as_d(c3), as_d(n1)) == (t.d1, t.d2, t.d3, t.dn) and (ds >= 0) == (t.dd is not None)
    assert t.dd is None or as_d(ds) == t.dd
    return t, c2


def _launch_tail(eng, c2, t, t1, x, batch, whole):
    """One mpx_bottleneck_tail over `batch` images -> fenced (out_hi, out_lo, next_hi, next_lo); t1 / x: fp16 (hi, lo) planes."""
    rows = batch * fed.BT_MAP * fed.BT_MAP
    planes = [Fenced(rows, c, eng.device) for c in (t.d3.cout, t.d3.cout, t.dn.cout, t.dn.cout)]
    tf = [None, None] if whole else [NanFenced(q) for q in t1]
    xf = [NanFenced(q) for q in x]
    rc = eng._lib.mpx_bottleneck_tail(eng._h, c2, *[_p(q.payload) if q else None for q in tf], *[_p(q.payload) for q in xf],
                                      *[_p(q.payload) for q in planes], batch, eng._stream())
    _lib.check(eng._h, rc, "mpx_bottleneck_tail")
    torch.cuda.synchronize()
    return planes


def _run_tail(eng, sd, k, whole, batch, mixed, kind):
    t, c2 = _tail_layers(eng, k)
    form = CONFIGS[k, whole]
    t1, x = fed.tail_draws(t, batch, mixed, device=eng.device)
    pre, want, b = (q.view(-1, t.d3.cout) for q in fed.tail_reference(sd, t, t1[2], x[2], whole))
    ced.preconditions(want)
    oh, ol, zh, zl = _launch_tail(eng, c2, t, t1[:2], x[:2], batch, whole)
    what = "%s layer1.%d %s%s batch %d (%d tiles on %d workgroups)" % (form, k, kind, " mixed" if mixed else "", batch, fed.tail_tiles(batch),
                                                                       fed.tail_grid(batch, eng.num_cus))
    _check(what + ", block output", form + " block output", oh, ol, pre, want, fed.tol_chain(b), "C_CHAIN")
    del pre, want, b
    _check_next(what, form, sd, t.dn, oh, ol, zh, zl, batch)


@pytest.mark.parametrize("which", range(3), ids=[w.replace(" ", "_") for w in WHICH])
@pytest.mark.parametrize("k,whole", list(CONFIGS), ids=list(CONFIGS.values()))
def test_block_tails_at_their_tile_edges(eng101, k, whole, which):
    """All three blocks of layer1, and layer1.0 whole (t1 = NULL): one image (28 tiles on 32 workgroups), the first batch with second tiles
    (the weight ring and the next-patch request cross a tile boundary), the first with third tiles."""
    eng, sd = eng101
    _run_tail(eng, sd, k, whole, fed.tail_batches(eng.num_cus)[which], False, "synthetic")


@pytest.mark.parametrize("k,whole", list(CONFIGS), ids=list(CONFIGS.values()))
def test_block_tails_on_trained_like_weights_and_mixed_draws(trained, k, whole):
    """Each config once on the trained-like ResNet-101 (layer1.0.downsample has channels whose B is a thousandth of the tensor's largest: the
    folded planes of build_fused feeding upload_tail_planes) with a quarter of the input channels x 1e-3, a quarter x 8, at the second-tile batch."""
    eng, sd = trained
    _run_tail(eng, sd, k, whole, fed.tail_batches(eng.num_cus)[1], True, "trained-like")


@pytest.mark.parametrize("k,whole", list(CONFIGS), ids=list(CONFIGS.values()))
def test_block_tail_bits_do_not_depend_on_the_tile_slot(eng101, k, whole):
    """The second-tile batch as copies of image 0: every output image has the bits of the one-image launch, whichever workgroup computed its
    tiles and whether as a first or a second tile."""
    eng, _sd = eng101
    t, c2 = _tail_layers(eng, k)
    batch = fed.tail_batches(eng.num_cus)[1]
    t1, x = fed.tail_draws(t, 1, False, device=eng.device)
    alone = _launch_tail(eng, c2, t, t1[:2], x[:2], 1, whole)
    rep = lambda q: q.expand(batch, -1, -1, -1).contiguous()
    many = _launch_tail(eng, c2, t, [rep(q) for q in t1[:2]], [rep(q) for q in x[:2]], batch, whole)
    for a, m, name in zip(alone, many, ("out_hi", "out_lo", "next_hi", "next_lo")):
        assert a.problems() == [] and m.problems() == [], name
        same = (m.payload_bits.view(batch, -1) == a.payload_bits.view(1, -1)).all(1)
        assert bool(same.all()), "%s %s: images %s differ from the one-image launch" % (CONFIGS[k, whole], name, (~same).nonzero().flatten().tolist()[:8])


# ------------------------------------------------------------------------------------------------
# pointwise tails
# ------------------------------------------------------------------------------------------------
def _ptail_layers(eng, arch, k):
    t = fed.pointwise_tail(k, arch)
    c3, n1 = eng.pointwise_tails()[k - 1]
    assert (ced.as_desc(eng.layers[c3]), ced.as_desc(eng.layers[n1])) == (t.d3, t.dn)
    return t, c3


def _launch_ptail(eng, c3, t, t2, x, batch):
    rows = batch * fed.PT_PIXELS
    planes = [Fenced(rows, c, eng.device) for c in (t.d3.cout, t.d3.cout, t.dn.cout, t.dn.cout)]
    ins = [NanFenced(q) for q in tuple(t2) + tuple(x)]
    rc = eng._lib.mpx_pointwise_tail(eng._h, c3, *[_p(q.payload) for q in ins], *[_p(q.payload) for q in planes], batch, eng._stream())
    _lib.check(eng._h, rc, "mpx_pointwise_tail")
    torch.cuda.synchronize()
    return planes


def _run_ptail(eng, sd, arch, k, batch, mixed, kind):
    t, c3 = _ptail_layers(eng, arch, k)
    t2, x = fed.ptail_draws(t, batch, mixed, device=eng.device, arch=arch)
    pre, want, b = (q.view(-1, t.d3.cout) for q in ced.reference(sd, t.d3, t2[2], x[2]))
    ced.preconditions(want)
    oh, ol, zh, zl = _launch_ptail(eng, c3, t, t2[:2], x[:2], batch)
    what = "BtPw128 %s layer2.%d %s%s batch %d (%d tiles on %d workgroups, the last of %d pixels)" % (
        arch, k, kind, " mixed" if mixed else "", batch, fed.ptail_tiles(batch), fed.ptail_grid(batch, eng.num_cus), fed.ptail_ragged(batch) or fed.PT_TP)
    _check(what + ", block output", "BtPw128 block output", oh, ol, pre, want, ced.tol(b), "C_TOL")
    del pre, want, b
    _check_next(what, "BtPw128", sd, t.dn, oh, ol, zh, zl, batch)


@pytest.mark.parametrize("which", range(4), ids=[w.replace(" ", "_") for w in PT_WHICH])
@pytest.mark.parametrize("k", [1, 2])
def test_pointwise_tails_at_their_tile_edges(eng50, k, which):
    """Both of ResNet-50's pairs: the smallest ragged last tile (16 pixels), the largest (112), a launch that ends on a tile boundary, and
    more tiles than workgroups."""
    eng, sd = eng50
    _run_ptail(eng, sd, "resnet50", k, fed.ptail_batches(eng.num_cus)[which], False, "synthetic")


def test_pointwise_tail_on_trained_like_weights_and_mixed_draws(trained):
    eng, sd = trained
    _run_ptail(eng, sd, "resnet101", 1, fed.ptail_batches(eng.num_cus)[3], True, "trained-like")


def test_pointwise_tail_bits_do_not_depend_on_the_tile_slot(eng50):
    """The second-tile batch as copies of image 0 (784 n mod 128 runs through every multiple of 16: every offset of an image within a tile,
    every tile slot of every workgroup): each output image has the bits of the one-image launch."""
    eng, _sd = eng50
    t, c3 = _ptail_layers(eng, "resnet50", 1)
    batch = fed.ptail_batches(eng.num_cus)[3]
    assert {fed.PT_PIXELS * n % fed.PT_TP for n in range(batch)} == set(range(0, fed.PT_TP, 16))
    t2, x = fed.ptail_draws(t, 1, False, device=eng.device)
    alone = _launch_ptail(eng, c3, t, t2[:2], x[:2], 1)
    rep = lambda q: q.expand(batch, -1, -1, -1).contiguous()
    many = _launch_ptail(eng, c3, t, [rep(q) for q in t2[:2]], [rep(q) for q in x[:2]], batch)
    for a, m, name in zip(alone, many, ("out_hi", "out_lo", "next_hi", "next_lo")):
        assert a.problems() == [] and m.problems() == [], name
        same = (m.payload_bits.view(batch, -1) == a.payload_bits.view(1, -1)).all(1)
        assert bool(same.all()), "BtPw128 %s: images %s differ from the one-image launch" % (name, (~same).nonzero().flatten().tolist()[:8])


# ------------------------------------------------------------------------------------------------
# the ImageNet stem
# ------------------------------------------------------------------------------------------------
_STEM = {}                              # (kind, mixed) -> the draw of three images and its fp64 references, built once


def _stem_case(eng, sd, kind, mixed):
    if (kind, mixed) not in _STEM:
        hi, lo, x = fed.stem_draws(3, mixed, device=eng.device)
        pre, want, b = ced.reference(sd, fed.STEM, x, None)
        ced.preconditions(want)
        pooled = fed.pool_reference(pre, want, b)
        ced.preconditions(pooled[0])
        _STEM[kind, mixed] = (hi, lo, pre, want, b) + pooled
    return _STEM[kind, mixed]


def _stage_by_hand(eng, hi, lo, batch):
    """The interior of the input planes written by hand; the 3-pixel border and the 4th channel stay as the engine made them (zero)."""
    assert ced.as_desc(eng.layers[0]) == fed.STEM
    for plane, src in zip(eng.input_planes(batch), (hi, lo)):
        assert tuple(plane.shape) == (batch, fed.IMG_PAD, fed.IMG_PAD, 4)
        plane[:, 3:227, 3:227, :3] = src[:batch]
        assert (plane[..., 3] == 0).all() and (plane[:, :3] == 0).all() and (plane[:, 227:] == 0).all() and (plane[:, :, :3] == 0).all() \
            and (plane[:, :, 227:] == 0).all()
    eng.mark_input_staged(0, batch)
    torch.cuda.synchronize()


def _check_removed_image(what, sd, hi, lo, per_image):
    """Image 1 (every segment removed) is relu(shift) to within C_TOL 2^-22 |shift| + 2^-24 everywhere, borders included."""
    _s, shift = (q.to(hi.payload.device) for q in ced.bn_affine(sd, fed.STEM))
    got = (hi.payload.double() + lo.payload.double())[per_image:2 * per_image]
    over = int((~((got - torch.relu(shift)).abs() <= ced.C_TOL * 2.0 ** -22 * shift.abs() + 2.0 ** -24)).sum())
    assert over == 0, "%s: %d elements of the all-removed image are not relu(shift)" % (what, over)
    off = (shift < -2.0 ** -20).expand_as(got)
    nonzero = int((hi.payload_bits[per_image:2 * per_image][off] != 0).sum()) + int((lo.payload_bits[per_image:2 * per_image][off] != 0).sum())
    assert nonzero == 0, "%s: %d planes' elements of the all-removed image are not +0 under a negative shift" % (what, nonzero)


def _run_stem_conv(eng, sd, kind, mixed, tile, batch):
    hi, lo, pre, want, b = _stem_case(eng, sd, kind, mixed)[:5]
    _stage_by_hand(eng, hi, lo, batch)
    rows = batch * 112 * 112
    oh, ol = Fenced(rows, 64, eng.device), Fenced(rows, 64, eng.device)
    eng.set_conv_tile(0, tile)
    try:
        rc = eng._lib.mpx_conv_bn_act(eng._h, 0, None, None, None, None, _p(oh.payload), _p(ol.payload), None, batch, eng._stream())
        _lib.check(eng._h, rc, "mpx_conv_bn_act(stem)")
        ran = eng._lib.mpx_last_conv_kernels(eng._h)
        torch.cuda.synchronize()
    finally:
        eng.set_conv_tile(0, -1)
    what = "stem conv %s%s tile %d batch %d (M mod %d = %d)" % (kind, " mixed" if mixed else "", tile, batch, ced.TILE_PIXELS[tile][0], rows % ced.TILE_PIXELS[tile][0])
    assert ran == 1 << tile, "%s ran kernels %#x" % (what, ran)
    v = lambda q: q[:batch].reshape(rows, 64)
    _check(what, "stem conv", oh, ol, v(pre), v(want), ced.tol(v(b)), "C_TOL")
    if batch >= 2:
        _check_removed_image(what, sd, oh, ol, 112 * 112)


def _run_stem_pool(eng, sd, kind, mixed, batch):
    hi, lo, _pre, _want, _b, pw, ptol, zero = _stem_case(eng, sd, kind, mixed)
    _stage_by_hand(eng, hi, lo, batch)
    rows = batch * 56 * 56
    oh, ol = Fenced(rows, 64, eng.device), Fenced(rows, 64, eng.device)
    _lib.check(eng._h, eng._lib.mpx_stem_conv_maxpool(eng._h, _p(oh.payload), _p(ol.payload), batch, eng._stream()), "mpx_stem_conv_maxpool")
    torch.cuda.synchronize()
    what = "stem + pool %s%s batch %d (%d workgroups)" % (kind, " mixed" if mixed else "", batch, fed.POOL_BLOCKS_PER_IMAGE * batch)
    v = lambda q: q[:batch].reshape(rows, 64)
    _check(what, "stem + pool", oh, ol, None, v(pw), v(ptol), "largest C_TOL tol of the window")
    _check_zeros(what, oh, ol, v(zero))
    if batch >= 2:
        _check_removed_image(what, sd, oh, ol, 56 * 56)


@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mixed"])
@pytest.mark.parametrize("tile", fed.STEM_TILES)
def test_stem_conv_on_every_tile_it_accepts(eng101, tile, mixed):
    """mpx_conv_bn_act on layer 0 from input planes written by hand: one image, where one image is no whole number of tiles (P = 192) the
    smallest batch that is, and on every tile the three images that differ: image 0 keeps every segment, image 1 none, image 2 about half."""
    eng, sd = eng101
    accepted = [t for t in ced.ALL_TILES if eng._lib.mpx_set_conv_tile(eng._h, 0, t) == 0]
    eng.set_conv_tile(0, -1)
    assert accepted == list(fed.STEM_TILES)
    for batch in sorted(set(fed.stem_batches(tile)) | {3}):
        _run_stem_conv(eng, sd, "synthetic", mixed, tile, batch)


@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mixed"])
@pytest.mark.parametrize("batch", [1, 3])
def test_stem_with_its_max_pool(eng101, batch, mixed):
    eng, sd = eng101
    _run_stem_pool(eng, sd, "synthetic", mixed, batch)


def test_stem_on_trained_like_weights_and_mixed_draws(trained):
    """Three images (kept, removed, half) through the default tile's conv and through the conv + pool launch."""
    eng, sd = trained
    _run_stem_conv(eng, sd, "trained-like", True, eng.conv_tile(0), 3)
    _run_stem_pool(eng, sd, "trained-like", True, 3)


def test_print_the_worst_ratios():
    """Last in the file: the worst err / tol per form of this session's cases (DESIGN.md 20 records a run)."""
    print()
    for form in sorted(WORST):
        print("fusededges worst err / tol  %-28s %.3f  (%s)" % (form, WORST[form][0], WORST[form][1]))
    assert WORST and all(r <= 1.0 for r, _w in WORST.values())
