"""The generic conv kernel beyond the ResNet shapes, at its edges (run on the MI355X box: pytest -m gpu): the rows of
generic_edge_draws.FORMS -- K loops of 1, 2, 3, 5 and an odd number of steps, stored widths of 32 / 64 / 80 / 1000 under tiles 64 or 128
channels wide, the SLICE epilogue, input slices and two-half maps, bias-only 5x5 and 3x3 layers, three stems on the NHWC4 staging and
DenseNet's 32-channel conv2 on the patch kernel -- through mpx_conv_bn_act on every tile mpx_set_conv_tile accepts for the row's layer
(AlexNet's 13x13 layers: the patch kernels, tiles 6 and 12, too), held to what tests/test_gpu_conv_edges.py holds the ResNet layers to.

Every launch.  Output planes are rows x y_pitch between two sentinel fences of 256 x y_pitch (test_gpu_conv_edges.Fenced, unchanged):
both fences intact bit for bit, every channel outside [y_offset, y_offset + stored) still the sentinel, none left inside, the stored pad
channels [cout, stored) exactly +0 in both planes.  Input planes lie between NaN fences of 256 pixel rows, the last pixel directly in
front of one, and the half an input-slice layer must not read is NaN: a value read from there and used puts a NaN into the payload.  Every
element is within tol = C_TOL 2^-22 B + 2^-24 of the fp64 conv + epilogue of the merged planes (the fp32 classifier: without the floor), the
older max norm holds too, a ReLU layer is exactly +0 in both planes wherever the fp64 pre-activation is below -tol, and on a 1x1 stride-1
layer image 0 has the same bits alone as in front of the batch.  The kernel of the tile under test ran the whole launch
(mpx_last_conv_kernels).  Batches: generic_edge_draws.row_batches.  Per row, the synthetic weights with the plain draw run every batch; the
mixed draw and the quiet-channel weights (both draws) the smallest batch of every tile (the classifier: all four).  A stem's planes are written by hand into the
staging: image 1 keeps no segment and must be relu(shift) everywhere, the last output row and column included."""
import ctypes as C

import pytest
import torch

import conv_edge_draws as ced
import generic_edge_draws as ged
from gpu_common import Fenced, layer_index as _index, ptr as _p
from network_interpretation_imagenet_amd import _lib
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine

pytestmark = pytest.mark.gpu

WORST = {}                              # form -> (worst err / tol, where)
COVERED = {}                            # form -> {(layer, residue class)}
ON_TILE = {}                            # (form, tile) -> {residue class}
ROW_IDS = ["%s-%s" % (r.arch, r.name) for r in ged.FORMS]


@pytest.fixture(scope="module")
def engines(mpx_lib):
    """arch -> an engine at max_batch 8 with the synthetic weights, made on first use."""
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    made = {}

    def get(arch):
        if arch not in made:
            made[arch] = MaskedForwardEngine(arch, max_batch=8, device=0).load_state_dict(ged.synthetic_state_dict(arch))
        return made[arch]

    yield get
    for e in made.values():
        e.close()


def _ints(fn, eng, i, n):
    v = [C.c_int(-1) for _ in range(n)]
    assert fn(eng._h, i, *[C.byref(q) for q in v]) == 0
    return tuple(q.value for q in v)


def _accepted(eng, i):
    acc = [t for t in ced.ALL_TILES if eng._lib.mpx_set_conv_tile(eng._h, i, t) == 0]
    eng.set_conv_tile(i, -1)
    return acc


class FencedInput:
    """Physical input planes [batch][hin][hin][x_pitch] between two NaN fences of FENCE_ROWS pixels, the last pixel directly in front of one."""

    def __init__(self, s, plane):
        phys = ged.physical(s, plane, fill=float("nan"))
        fence = ced.FENCE_ROWS * s.x_pitch
        self.buf = torch.full((2 * fence + phys.numel(),), float("nan"), dtype=torch.float16, device=plane.device)
        self.payload = self.buf[fence:fence + phys.numel()]
        self.payload.copy_(phys.reshape(-1))
        assert self.payload.data_ptr() % 16 == 0


class Case:
    """One (row, weights, draw form): the draw at the row's largest batch and its fp64 reference, on the device; a smaller batch is a prefix."""

    def __init__(self, eng, row, kind, mixed, batch):
        self.eng, self.row, self.s, self.batch = eng, row, ged.spec(row), batch
        s, sd = self.s, ged.state_dict(kind, row.arch)
        self.i = _index(eng, row.name)
        self.kind, self.mixed, self.sd = kind, mixed, sd
        self.x = ged.draws(row, batch, mixed, device=eng.device)
        pre, want, b = ged.reference(sd, s, self.x[2])
        self.pre, self.want, self.b = (t.view(-1, s.d.cout) for t in (pre, want, b))
        ced.preconditions(self.want)                                    # on the reference alone, on the very draw that runs
        self.per_image = s.d.hout * s.d.hout
        self.inputs = {}

    def planes(self, batch):
        """Input pointers of the first `batch` images: fenced planes, or None for a stem (whose staging is written here)."""
        s, eng = self.s, self.eng
        if s.stem_run:
            for plane, src in zip(eng.input_planes(batch), self.x[:2]):
                assert tuple(plane.shape) == (batch, 230, 230, 4)
                plane[:, 3:227, 3:227, :3] = src[:batch]
                assert not plane[..., 3].any() and not plane[:, :3].any() and not plane[:, 227:].any() and not plane[:, :, :3].any() \
                    and not plane[:, :, 227:].any()
            eng.mark_input_staged(0, batch)
            torch.cuda.synchronize()
            return None, None
        if batch not in self.inputs:
            self.inputs = {batch: (FencedInput(s, self.x[0][:batch]), FencedInput(s, self.x[1][:batch]))}
        return tuple(f.payload for f in self.inputs[batch])


def _launch(case, tile, batch):
    eng, s, i = case.eng, case.s, case.i
    rows = batch * case.per_image
    in_hi, in_lo = case.planes(batch)
    if s.f32:
        hi = lo = Fenced(rows, s.y_pitch, eng.device, f32=True)
        outs = (None, None, _p(hi.payload))
    else:
        hi, lo = Fenced(rows, s.y_pitch, eng.device), Fenced(rows, s.y_pitch, eng.device)
        outs = (_p(hi.payload), _p(lo.payload), None)
    eng.set_conv_tile(i, tile)
    try:
        rc = eng._lib.mpx_conv_bn_act(eng._h, i, _p(in_hi), _p(in_lo), None, None, *outs, batch, eng._stream())
        _lib.check(eng._h, rc, "mpx_conv_bn_act(%s, tile %d, batch %d)" % (s.d.name, tile, batch))
        mask = eng._lib.mpx_last_conv_kernels(eng._h)
        torch.cuda.synchronize()
    finally:
        eng.set_conv_tile(i, -1)
    return hi, lo, mask


def _check(what, form, s, hi, lo, pre, want, b):
    """The checks of one launch; pre / want / b: [rows][cout]."""
    off, st, cout = s.y_offset, s.stored, s.d.cout
    for plane, which in ((hi, "hi"),) + (() if s.f32 else ((lo, "lo"),)):
        fences = [p for p in plane.problems() if not p.startswith("payload")]
        assert fences == [], "%s, %s plane: %s" % (what, which, "; ".join(fences))
        bits = plane.payload_bits
        outside = torch.ones(s.y_pitch, dtype=torch.bool, device=bits.device)
        outside[off:off + st] = False
        touched = int((bits[:, outside] != plane.sentinel).sum())
        assert touched == 0, "%s, %s plane: %d elements outside channels [%d, %d) overwritten" % (what, which, touched, off, off + st)
        left = int((bits[:, off:off + st] == plane.sentinel).sum())
        assert left == 0, "%s, %s plane: %d elements of the stored channels never written" % (what, which, left)
        pads = int((bits[:, off + cout:off + st] != 0).sum())
        assert pads == 0, "%s, %s plane: %d elements of the pad channels [%d, %d) are not +0" % (what, which, pads, off + cout, off + st)
    got = hi.payload[:, off:off + cout].double()
    if not s.f32:
        got = got + lo.payload[:, off:off + cout].double()
    assert not torch.isnan(got).any(), "%s: NaN in the payload (a fence or the other half was read and used)" % what
    err, tol = (got - want).abs(), ged.tol(b, s)
    ratio = (err / tol).max().item()
    worst = torch.argmax(err / tol).item()
    print("%s: worst err / tol %.3f (pixel row %d, channel %d); max norm %.2e" % (what, ratio, worst // cout, worst % cout,
                                                                                 err.max().item() / max(want.abs().max().item(), 1.0)))
    if ratio > WORST.get(form, (0.0, ""))[0]:
        WORST[form] = (ratio, what)
    assert ratio <= 1.0, "%s: %d elements over their bound, worst err / tol %.3f at pixel row %d, channel %d" % (
        what, int((err > tol).sum()), ratio, worst // cout, worst % cout)
    assert ced.max_norm_ok(got, want), what                             # the suite's older check, kept
    if s.d.relu:
        neg = pre < -tol
        assert neg.any(), what
        hb, lb = hi.payload_bits[:, off:off + cout], lo.payload_bits[:, off:off + cout]
        assert (hb[neg] == 0).all() and (lb[neg] == 0).all(), "%s: a clearly negative pre-activation is not +0 in both planes" % what


def _check_removed_image(what, case, hi, lo):
    """A stem's image 1 (every segment removed) is relu(shift) within C_TOL 2^-22 |shift| + 2^-24 everywhere, the last row and column included."""
    s, n = case.s, case.per_image
    _sc, shift = (q.to(case.eng.device) for q in ged.affine(case.sd, s))
    got = (hi.payload.double() + lo.payload.double())[n:2 * n, :s.d.cout]
    over = int((~((got - torch.relu(shift)).abs() <= ged.C_TOL * 2.0 ** -22 * shift.abs() + 2.0 ** -24)).sum())
    assert over == 0, "%s: %d elements of the all-removed image are not relu(shift)" % (what, over)
    off = (shift < -2.0 ** -20).expand_as(got)
    nonzero = int((hi.payload_bits[n:2 * n, :s.d.cout][off] != 0).sum()) + int((lo.payload_bits[n:2 * n, :s.d.cout][off] != 0).sum())
    assert nonzero == 0, "%s: %d plane elements of the all-removed image are not +0 under a negative shift" % (what, nonzero)


def _run(case, tile, cls, batch):
    s, row = case.s, case.row
    p = ced.tile_pixels(s.d, tile)
    rows = batch * case.per_image
    what = "%s %s %s%s tile %d batch %d (M mod %d = %s)" % (row.arch, row.name, case.kind, " mixed" if case.mixed else "", tile, batch, p, cls)
    hi, lo, mask = _launch(case, tile, batch)
    assert mask == 1 << tile, "%s ran kernels %#x, not %#x" % (what, mask, 1 << tile)
    _check(what, row.form, s, hi, lo, case.pre[:rows], case.want[:rows], case.b[:rows])
    COVERED.setdefault(row.form, set()).add((row.name, cls))
    ON_TILE.setdefault((row.form, tile), set()).add(cls)
    if s.stem_run and batch >= 2:
        _check_removed_image(what, case, hi, lo)
    if s.d.ksize == 1 and s.d.stride == 1 and not s.stem_run and batch > 1:
        ahi, alo, _mask = _launch(case, tile, 1)
        n = case.per_image
        assert torch.equal(ahi.bits[:ahi.fence + n * s.y_pitch], hi.bits[:hi.fence + n * s.y_pitch]) \
            and torch.equal(alo.bits[:alo.fence + n * s.y_pitch], lo.bits[:lo.fence + n * s.y_pitch]), \
            "%s: image 0 has other bits alone than as the first image of the batch" % what


def _check_descriptors(eng, row):
    """The Spec against the engine: mpx_conv_info, mpx_conv_out_slice, mpx_conv_in_slice, and the tiles mpx_set_conv_tile accepts."""
    s, i = ged.spec(row), _index(eng, row.name)
    d = eng.layers[i]
    assert ced.as_desc(d) == s.d, (ced.as_desc(d), s.d)
    assert d.k_packed == ged.k_packed(s) and d.cout_pad == -(-s.d.cout // 128) * 128, (row.name, d.k_packed, d.cout_pad)
    assert _ints(eng._lib.mpx_conv_out_slice, eng, i, 2) == (s.y_pitch, s.y_offset), (row.name, _ints(eng._lib.mpx_conv_out_slice, eng, i, 2))
    assert _ints(eng._lib.mpx_conv_in_slice, eng, i, 4) == (s.x_pitch, s.x_offset, s.bf, s.hp), (row.name, _ints(eng._lib.mpx_conv_in_slice, eng, i, 4))
    accepted = _accepted(eng, i)
    if ged.only_generic(s):
        assert accepted == list(ced.GENERIC_TILES), "%s accepts %s" % (row.name, accepted)
    assert accepted == list(row.tiles) == list(ged.accepted_tiles(s)), "%s accepts %s, the row runs %s" % (row.name, accepted, row.tiles)
    assert (i == len(eng.layers) - 1) == s.f32


@pytest.mark.parametrize("row", ged.FORMS, ids=ROW_IDS)
@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mixed"])
@pytest.mark.parametrize("kind", ["synthetic", "quiet"])
def test_row_on_every_tile(engines, row, kind, mixed):
    eng = engines(row.arch)
    _check_descriptors(eng, row)
    every = (kind == "synthetic" and not mixed) or ged.spec(row).f32      # (the classifier's four batches are rows of one small draw)
    jobs = []
    for tile in row.tiles:
        batches = ged.row_batches(row, tile, eng.num_cus)
        assert batches, (row, tile)
        jobs += [(tile, c, b) for c, b in (batches if every else [min(batches, key=lambda cb: cb[1])])]
    if kind == "quiet":
        eng.load_state_dict(ged.quiet_state_dict(row.arch), only=[row.name])
    try:
        case = Case(eng, row, kind, mixed, max(j[2] for j in jobs))
        if kind == "quiet":
            ch = ged.quiet_channels(case.s.d.cout)
            assert case.b[:, ch].max() < 2.0 ** -5 * case.b.max(), "%s has no quiet channels" % row.name
        for batch in sorted({j[2] for j in jobs}):
            for tile, cls, b in jobs:
                if b == batch:
                    _run(case, tile, cls, batch)
    finally:
        if kind == "quiet":
            eng.load_state_dict(ged.synthetic_state_dict(row.arch), only=[row.name])


def test_print_the_worst_ratios_and_the_classes_covered(engines):
    """Last in the file: the worst err / tol per form and the (layer, residue class) pairs of this session's launches (DESIGN.md 26 records a
    run); every form met, on every tile its rows run, every residue class generic_edge_draws.row_batches yields there.  That is every class
    that exists EXCEPT generic_edge_draws.KNOWN_HOLES, printed here: classes whose smallest batch is over the cap on the planes of a case."""
    print()
    for form, name, tiles, classes in ged.KNOWN_HOLES:
        print("genericedges NOT run          %-28s %s on tile%s %s: class%s %s (over %d MB of planes)" % (
            form, name, "s" * (len(tiles) > 1), ",".join(map(str, tiles)), "es" * (len(classes) > 1), ",".join(classes), ged.PLANE_BYTES_CAP >> 20))
    for form in ged.FORM_NAMES:
        ratio, what = WORST.get(form, (float("nan"), "not run"))
        pairs = sorted(COVERED.get(form, ()))
        print("genericedges worst err / tol  %-28s %.3f  (%s)" % (form, ratio, what))
        print("genericedges covered          %-28s %s" % (form, "; ".join("%s: %s" % (n, ",".join(c for m, c in pairs if m == n)) for n in dict.fromkeys(m for m, _c in pairs))))
    num_cus = engines(ged.ARCHS[0]).num_cus
    for form in ged.FORM_NAMES:
        need = ged.classes_of_form(form, num_cus)
        met = {c for _n, c in COVERED.get(form, ())}
        assert need <= met, "%s: residue classes %s never ran" % (form, sorted(need - met))
        assert WORST[form][0] <= 1.0
        for tile in sorted({t for row in ged.FORMS if row.form == form for t in row.tiles}):
            need = ged.classes_of_form(form, num_cus, tile)
            assert need <= ON_TILE.get((form, tile), set()), "%s, tile %d: residue classes %s never ran" % (
                form, tile, sorted(need - ON_TILE.get((form, tile), set())))
        for row in ged.FORMS:
            if row.form == form and row.all_classes:
                assert {c for n, c in COVERED[form] if n == row.name} >= set(ced.RESIDUES), row.name
