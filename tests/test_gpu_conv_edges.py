"""The ResNet conv kernels at their tile edges (run on the MI355X box: pytest -m gpu): the generic tiles 0 / 1 / 2 / 4 / 7, the patch kernels
6 / 12, the 256x256 kernels 9 / 13, the expanding 1x1 kernels 10 / 14, the three dual forms and fc, through mpx_conv_bn_act and
mpx_conv_dual_bn_act.

Every output plane is [front fence | payload | back fence], each fence conv_edge_draws.FENCE_ROWS pixel rows of cout elements, all of it
prefilled with the sentinel 0x7e00 (fc: an fp32 NaN pattern): after a launch both fences are intact bit for bit and no sentinel is left
in the payload.  Batches come from conv_edge_draws.edge_batches: the smallest that put M = B hout^2 one past a tile boundary, one short of
it and on it, at which the kernel under test itself runs the whole launch (asserted through mpx_last_conv_kernels).  Every element is held
to tol = C_TOL 2^-22 B + 2^-24 against the fp64 conv + BN (+ residual) (+ ReLU) of the merged input planes (conv_edge_draws; the CPU
emulation in tests/test_conv_bounds_cpu.py is where C_TOL comes from), the suite's older max norm of 4e-6 stays as a second assertion,
pre-activations clearly below zero must be +0 in both planes, and on the pointwise forms image 0 has the same bits alone and as the first
image of the batch.  Inputs and references are built once per (layer, batch) on the device and shared by the tiles."""

import pytest
import torch

import conv_edge_draws as ced
from gpu_common import dev, Fenced, layer_index as _index, ptr as _p  # noqa: F401  (dev is a fixture)
from network_interpretation_imagenet_amd import _lib, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine

pytestmark = pytest.mark.gpu

WORST = {}                              # kernel form -> (worst err / tol, where)
COVERED = {}                            # kernel form -> {(layer, residue class)}


def _engine(arch, sd):
    return MaskedForwardEngine(arch, max_batch=8, device=0).load_state_dict(sd)


@pytest.fixture(scope="module")
def eng18(dev):
    e = _engine("resnet18", synth.make_state_dict("resnet18"))
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng50(dev):
    e = _engine("resnet50", synth.make_state_dict("resnet50"))
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng101(dev):
    e = _engine("resnet101", synth.make_state_dict("resnet101"))
    yield e
    e.close()


@pytest.fixture(scope="module")
def trained(dev):
    from oracle import trained_like
    sd = trained_like.make_trained_like_state_dict("resnet101")
    e = _engine("resnet101", sd)
    yield e, sd
    e.close()


def test_the_fence_check_turns_red(dev):
    """The detector itself, from the host side: one poked element on either side, one unwritten payload element."""
    for f32 in (False, True):
        plane = Fenced(5, 16, dev, f32)
        assert plane.payload.data_ptr() % 16 == 0
        assert len(plane.problems()) == 1 and "never written" in plane.problems()[0]
        plane.payload.zero_()
        assert plane.problems() == []
        plane.values[plane.fence - 1] = 1.0
        assert len(plane.problems()) == 1 and "front fence: 1 elements overwritten, the last at 1 before" in plane.problems()[0]
        plane.bits[plane.fence - 1] = plane.sentinel
        plane.values[plane.fence + 5 * 16] = 0.0            # what a store of one row too many would do
        assert len(plane.problems()) == 1 and "back fence: 1 elements overwritten, the first at 0 behind" in plane.problems()[0]
        plane.bits[plane.fence + 5 * 16] = plane.sentinel
        plane.payload_bits[3, 7] = plane.sentinel
        assert plane.problems() == ["payload: 1 elements never written, the first in pixel row 3"]


# ------------------------------------------------------------------------------------------------
# one case = one (layer, batch) draw with its fp64 reference on the device, shared by the tiles
# ------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, eng, sd, arch, name, batch, mixed, with_res=None):
        self.eng, self.name, self.batch = eng, name, batch
        self.i = _index(eng, name)
        self.d = ced.as_desc(eng.layers[self.i])
        assert self.d == ced.layer_desc(arch, name), (self.d, ced.layer_desc(arch, name))
        self.with_res = bool(self.d.residual) if with_res is None else with_res
        self.x, self.res = ced.draws(self.d, batch, ced.draw_seed(arch, name), mixed, device=eng.device, with_res=self.with_res)
        pre, want, b = ced.reference(sd, self.d, self.x[2], self.res[2] if self.res else None)
        self.rows = batch * self.d.hout * self.d.hout
        self.pre, self.want, self.b = (t.view(self.rows, self.d.cout) for t in (pre, want, b))
        self.top, self.small = ced.preconditions(self.want)         # on the reference alone, on the very draw that runs


def _launch(case, tile, batch=None):
    """mpx_conv_bn_act on `tile` over the first `batch` images of the case -> (hi, lo fenced planes, kernels that ran)."""
    eng, d = case.eng, case.d
    batch = case.batch if batch is None else batch
    rows = batch * d.hout * d.hout
    hi, lo = Fenced(rows, d.cout, eng.device), Fenced(rows, d.cout, eng.device)
    r = case.res or (None, None)
    eng.set_conv_tile(case.i, tile)
    try:
        rc = eng._lib.mpx_conv_bn_act(eng._h, case.i, _p(case.x[0]), _p(case.x[1]), _p(r[0]), _p(r[1]), _p(hi.payload), _p(lo.payload), None,
                                      batch, eng._stream())
        _lib.check(eng._h, rc, "mpx_conv_bn_act(%s, tile %d, batch %d)" % (case.name, tile, batch))
        mask = eng._lib.mpx_last_conv_kernels(eng._h)
        torch.cuda.synchronize()
    finally:
        eng.set_conv_tile(case.i, -1)
    return hi, lo, mask


def _check_planes(what, form, hi, lo, pre, want, b, relu, resplit=True):
    """The checks of one launch; hi / lo: Fenced planes (fc: the fp32 plane twice)."""
    for plane, which in ((hi, "hi"), (lo, "lo")):
        assert plane.problems() == [], "%s, %s plane: %s" % (what, which, "; ".join(plane.problems()))
    got = (hi.payload.double() + lo.payload.double()) if resplit else hi.payload.double()
    assert not torch.isnan(got).any(), what
    err, tol = (got - want).abs(), ced.tol(b, resplit)
    ratio = (err / tol).max().item()
    worst = torch.argmax(err / tol).item()
    print("%s: worst err / tol %.3f (pixel row %d, channel %d); max norm %.2e" % (what, ratio, worst // want.shape[1], worst % want.shape[1],
                                                                                 err.max().item() / max(want.abs().max().item(), 1.0)))
    if ratio > WORST.get(form, (0.0, ""))[0]:
        WORST[form] = (ratio, what)
    assert ratio <= 1.0, "%s: %d elements over their bound, worst err / tol %.3f at pixel row %d, channel %d" % (
        what, int((err > tol).sum()), ratio, worst // want.shape[1], worst % want.shape[1])
    assert ced.max_norm_ok(got, want), what                         # the suite's older check, kept
    if relu:
        neg = pre < -tol
        assert neg.any(), what
        assert (hi.payload_bits[neg] == 0).all() and (lo.payload_bits[neg] == 0).all(), "%s: a clearly negative pre-activation is not +0 in both planes" % what


def _run(case, tile, cls, want_mask=None):
    """One launch of the case on `tile` with every check; the kernel of `tile` itself must have run the whole launch."""
    d = case.d
    what = "%s tile %d batch %d (M mod %d = %s)" % (case.name, tile, case.batch, ced.tile_pixels(d, tile), cls)
    hi, lo, mask = _launch(case, tile)
    want_mask = 1 << tile if want_mask is None else want_mask
    assert mask == want_mask, "%s ran kernels %#x, not %#x" % (what, mask, want_mask)
    form = "tile %d" % tile if want_mask == 1 << tile else "tile %d -> %d" % (tile, want_mask.bit_length() - 1)
    _check_planes(what, form, hi, lo, case.pre, case.want, case.b, d.relu)
    COVERED.setdefault(form, set()).add((case.name, cls))
    if tile in ced.POINTWISE_TILES and d.ksize == 1 and d.stride == 1 and case.batch > 1:
        # image 0 alone (under a round of tiles: the fallback kernel, documented as bit-identical) against image 0 of the batch
        ahi, alo, _mask = _launch(case, tile, batch=1)
        n = d.hout * d.hout
        assert ahi.problems() == [] and alo.problems() == [], what
        assert torch.equal(ahi.payload_bits, hi.payload_bits[:n]) and torch.equal(alo.payload_bits, lo.payload_bits[:n]), \
            "%s: image 0 has other bits alone than as the first image of the batch" % what


def _accepted(eng, i, d):
    """The tile ids mpx_set_conv_tile accepts for the layer; conv_edge_draws.accepts must say the same."""
    out = []
    for tile in ced.ALL_TILES:
        ok = eng._lib.mpx_set_conv_tile(eng._h, i, tile) == 0
        assert ok == ced.accepts(d, tile), "%s tile %d: the engine says %s" % (d.name, tile, ok)
        if ok:
            out.append(tile)
    eng.set_conv_tile(i, -1)
    return out


def _cases_by_batch(eng, sd, arch, name, mixed, jobs, with_res=None):
    """jobs: [(tile, class, batch)] -> runs them grouped by batch, one Case per batch."""
    for batch in sorted({j[2] for j in jobs}):
        case = Case(eng, sd, arch, name, batch, mixed, with_res)
        for tile, cls, b in jobs:
            if b == batch:
                _run(case, tile, cls)
        del case


# ------------------------------------------------------------------------------------------------
# mpx_conv_bn_act
# ------------------------------------------------------------------------------------------------
def test_descriptors_are_the_topology_the_draws_assume(eng18, eng50, eng101):
    for eng, arch in ((eng18, "resnet18"), (eng50, "resnet50"), (eng101, "resnet101")):
        assert [ced.as_desc(d) for d in eng.layers[1:]] == ced.resnet_layers(arch)


@pytest.mark.parametrize("name", [d.name for d in ced.distinct_shapes("resnet101")])
def test_every_shape_on_every_tile_it_accepts(eng101, name):
    """The 23 distinct conv shapes of ResNet-50 / 101 x every tile id the layer accepts, at the first residue class that exists."""
    sd = synth.make_state_dict("resnet101")
    i = _index(eng101, name)
    d = ced.as_desc(eng101.layers[i])
    jobs = []
    for tile in _accepted(eng101, i, d):
        if tile == 14 and not (d.residual and d.relu):
            continue                                    # (hands over to tile 10 without a residual: test_gpu_parity.py; no such ResNet layer)
        cls, batch = next((c, b) for c, b in ced.edge_batches(d, tile, eng101.num_cus).items() if b is not None)
        jobs.append((tile, cls, batch))
    assert jobs
    _cases_by_batch(eng101, sd, "resnet101", name, False, jobs)


@pytest.mark.parametrize("tile", ced.ALL_TILES)
def test_every_residue_class_per_kernel_form(eng101, tile):
    """Per kernel form: every residue class that exists, on the smallest layers that serve (conv_edge_draws.FORM_LAYERS)."""
    sd = synth.make_state_dict("resnet101")
    seen = set()
    for name in ced.FORM_LAYERS[tile]:
        d = ced.layer_desc("resnet101", name)
        classes = ced.edge_batches(d, tile, eng101.num_cus)
        jobs = [(tile, c, b) for c, b in classes.items() if b is not None]
        _cases_by_batch(eng101, sd, "resnet101", name, False, jobs)
        seen |= {c for _t, c, _b in jobs}
        assert {c for n, c in COVERED["tile %d" % tile] if n == name} >= {c for c, b in classes.items() if b is not None}
    assert seen == set(ced.RESIDUES) - ({"1", "P-1"} if tile == 14 else set())     # (K = 256 expanding layers live on 14 x 14 maps: 0 only)


@pytest.mark.parametrize("tile", ced.ALL_TILES)
def test_trained_like_statistics_on_mixed_draws(trained, tile):
    """Trained-like BatchNorm (gammas -0.2 .. 1.6, variances 4e-6 .. 100) on the mixed draws (a quarter of the input channels x 1e-3, a
    quarter x 8): per kernel form, its first layer of FORM_LAYERS at the first residue class that exists."""
    eng, sd = trained
    name = ced.FORM_LAYERS[tile][0]
    d = ced.layer_desc("resnet101", name)
    cls, batch = next((c, b) for c, b in ced.edge_batches(d, tile, eng.num_cus).items() if b is not None)
    _cases_by_batch(eng, sd, "resnet101", name, True, [(tile, cls, batch)])


@pytest.mark.parametrize("name", ced.QUIET_CHANNEL_LAYERS)
def test_trained_like_layers_with_quiet_channels(trained, name):
    """The layers of the trained-like ResNet-101 that have output channels whose B is under 1 % of the tensor's largest (a scale a
    thousandth of the neighbours'): what the max norm is blind to (tests/test_conv_bounds_cpu.py shows it on the first of them), on every
    tile the layer accepts."""
    eng, sd = trained
    i = _index(eng, name)
    d = ced.as_desc(eng.layers[i])
    jobs = []
    for tile in _accepted(eng, i, d):
        cls, batch = next((c, b) for c, b in ced.edge_batches(d, tile, eng.num_cus).items() if b is not None)
        jobs.append((tile, cls, batch))
    for batch in sorted({j[2] for j in jobs}):
        case = Case(eng, sd, "resnet101", name, batch, False)
        assert (case.b.max(0).values < 0.01 * case.b.max()).any(), "%s has no quiet channel" % name
        for tile, cls, b in jobs:
            if b == batch:
                _run(case, tile, cls)


@pytest.mark.parametrize("name", ced.R18_RESIDUAL_LAYERS)
def test_resnet18_blocks_with_a_residual(eng18, name):
    """The 3x3 layers that DO take a residual (BasicBlock conv2) on tiles 0, 1, 2 and 6; the persistent patch kernel refuses them."""
    sd = synth.make_state_dict("resnet18")
    i = _index(eng18, name)
    d = ced.as_desc(eng18.layers[i])
    assert d.residual and d.ksize == 3
    assert _accepted(eng18, i, d) == [0, 1, 2, 4, 6, 7]
    jobs = [(tile, c, b) for tile in (0, 1, 2, 6) for c, b in ced.edge_batches(d, tile, eng18.num_cus).items() if b is not None]
    _cases_by_batch(eng18, sd, "resnet18", name, False, jobs)


def test_tile12_with_a_residual_operand_hands_over_to_tile6(eng18):
    """A layer the persistent patch kernel accepts, called WITH residual planes at a batch that fills its round of tiles: the launch must
    run the patch kernel of tile 6 (bit 6), and everything else holds as for any case."""
    sd = synth.make_state_dict("resnet18")
    name = ced.R18_HANDOVER_LAYER
    d = ced.layer_desc("resnet18", name)
    batch = ced.edge_batches(d, 12, eng18.num_cus, with_res=False)["0"]
    assert ced.expected_kernels(d, 12, batch, False, eng18.num_cus) == 1 << 12 and ced.expected_kernels(d, 12, batch, True, eng18.num_cus) == 1 << 6
    case = Case(eng18, sd, "resnet18", name, batch, False, with_res=True)
    _run(case, 12, "0", want_mask=1 << 6)
    plain = Case(eng18, sd, "resnet18", name, batch, False, with_res=False)
    _run(plain, 12, "0")                                # without the operand the same launch is the persistent kernel's


# ------------------------------------------------------------------------------------------------
# mpx_conv_dual_bn_act
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", ced.DUAL_TILES)
@pytest.mark.parametrize("stage", ced.DUAL_STAGES)
def test_dual_launch(eng50, stage, tile):
    """layerN.0.conv3 + layerN.0.downsample.0 K-concatenated in one launch, on the dual kernels of tiles 2 and 7 and the dual form of the
    persistent 256x256 kernel (tile 13), both operands drawn as the single launches' are; B sums both branches."""
    eng, arch = eng50, "resnet50"
    sd = synth.make_state_dict(arch)
    i, j = _index(eng, "layer%d.0.conv3" % stage), _index(eng, "layer%d.0.downsample.0" % stage)
    d3, dd = ced.as_desc(eng.layers[i]), ced.as_desc(eng.layers[j])
    classes = ced.edge_batches(d3, tile, eng.num_cus, dual=True)
    assert any(b is not None for b in classes.values())
    for cls, batch in classes.items():
        if batch is None:
            continue
        assert ced.expected_dual_kernels(d3, tile, batch, eng.num_cus) == 1 << tile
        t2, _ = ced.draws(d3, batch, ced.draw_seed(arch, d3.name), False, device=eng.device, with_res=False)
        x, _ = ced.draws(dd, batch, ced.draw_seed(arch, dd.name), False, device=eng.device)
        pre, want, b = (t.view(-1, d3.cout) for t in ced.dual_reference(sd, d3, dd, t2[2], x[2]))
        ced.preconditions(want)
        rows = batch * d3.hout * d3.hout
        hi, lo = Fenced(rows, d3.cout, eng.device), Fenced(rows, d3.cout, eng.device)
        # (conv3 takes a residual, so mpx_set_conv_tile refuses it tile 13: its dual form is what the layer's DEFAULT, a 256-row id, runs)
        assert tile != 13 or eng.conv_tile(i) in (9, 10, 14)
        eng.set_conv_tile(i, -1 if tile == 13 else tile)
        try:
            rc = eng._lib.mpx_conv_dual_bn_act(eng._h, i, _p(t2[0]), _p(t2[1]), _p(x[0]), _p(x[1]), _p(hi.payload), _p(lo.payload), batch, eng._stream())
            _lib.check(eng._h, rc, "mpx_conv_dual_bn_act")
            mask = eng._lib.mpx_last_conv_kernels(eng._h)
            torch.cuda.synchronize()
        finally:
            eng.set_conv_tile(i, -1)
        what = "layer%d.0 dual tile %d batch %d (M mod %d = %s)" % (stage, tile, batch, ced.tile_pixels(d3, tile), cls)
        assert mask == 1 << tile, "%s ran kernels %#x" % (what, mask)
        _check_planes(what, "dual %d" % tile, hi, lo, pre, want, b, True)
        COVERED.setdefault("dual %d" % tile, set()).add((d3.name, cls))
    if stage == 4:
        assert {c for _n, c in COVERED["dual %d" % tile]} == set(ced.RESIDUES)


# ------------------------------------------------------------------------------------------------
# fc
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", ced.GENERIC_TILES)
def test_fc_around_a_pixel_tile(eng50, tile):
    """fc = the generic kernel with M = batch and an fp32 [B][1000] output (1000 columns: no multiple of any tile width), at batches 1,
    P - 1, P and P + 1 of the tile; fp32-NaN fences; the per-element bound without the re-split's floor.  The preconditions are checked on
    the draw (P + 1 rows), of which the smaller batches are the first rows."""
    eng, arch = eng50, "resnet50"
    sd = synth.make_state_dict(arch)
    i = _index(eng, "fc")
    d = ced.as_desc(eng.layers[i])
    assert d == ced.layer_desc(arch, "fc") and _accepted(eng, i, d) == list(ced.GENERIC_TILES)
    p = ced.TILE_PIXELS[tile][0]
    x, _ = ced.draws(d, p + 1, ced.draw_seed(arch, "fc"), False, device=eng.device)
    pre, want, b = (t.view(p + 1, d.cout) for t in ced.reference(sd, d, x[2], None))
    ced.preconditions(want)
    for batch in (1, p - 1, p, p + 1):
        out = Fenced(batch, d.cout, eng.device, f32=True)
        eng.set_conv_tile(i, tile)
        try:
            rc = eng._lib.mpx_conv_bn_act(eng._h, i, _p(x[0]), _p(x[1]), None, None, None, None, _p(out.payload), batch, eng._stream())
            _lib.check(eng._h, rc, "mpx_conv_bn_act(fc)")
            mask = eng._lib.mpx_last_conv_kernels(eng._h)
            torch.cuda.synchronize()
        finally:
            eng.set_conv_tile(i, -1)
        what = "fc tile %d batch %d (P = %d)" % (tile, batch, p)
        assert mask == 1 << tile, "%s ran kernels %#x" % (what, mask)
        _check_planes(what, "fc on tile %d" % tile, out, out, pre[:batch], want[:batch], b[:batch], False, resplit=False)


def test_print_the_worst_ratios():
    """Last in the file: the worst err / tol per kernel form of this session's cases (DESIGN.md 19 records a run)."""
    print()
    for form in sorted(WORST, key=lambda f: (f.split()[0], int(f.split()[-1]))):
        classes = sorted({c for _n, c in COVERED.get(form, ())})
        print("convedges worst err / tol  %-14s %.3f  (%s)%s" % (form, WORST[form][0], WORST[form][1], "  classes " + ",".join(classes) if classes else ""))
    assert all(r <= 1.0 for r, _w in WORST.values())
