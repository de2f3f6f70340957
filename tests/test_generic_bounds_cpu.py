"""The per-element bound of tests/test_gpu_generic_edges.py on the CPU, as tests/test_conv_bounds_cpu.py is for the ResNet layers: that file's
numpy emulation of the kernels' arithmetic (emulate, unchanged) with the library's own packer on every row of generic_edge_draws.FORMS --
plain and mixed draws, synthetic and quiet-channel weights -- against fp64.  It measures r_ref = max err / (2^-22 B + 2^-24), asserts that
the constant of the draws module is 4 x the worst r_ref rounded up to a power of two, checks on the reference alone the preconditions of
every draw the GPU test makes, the batches every (row, tile) runs, and that the Specs are the families' own topologies.  No GPU.

What the emulation restates per kind of row.  The packer is called with the row's own descriptor: k_packed = k^2 cin_pad (pad channels get
zero weights), the conv bias, the family's BatchNorm eps.  A layer that reads a slice or a two-half map is emulated on the DENSE layout of
its cin_pad channels, as mpx_pack_conv_weights packs it (the engine places the columns itself; which 32 channels share a K step differs,
the arithmetic does not).  A stem is emulated in the K order of the staging the packer documents (include/mpx.h: k = (ky run + px) 4 + c,
run = 8 pixels, 16 for AlexNet's 11-wide row): the input is gathered into those runs and the layer emulated as a 1x1 conv over them, so a
packer whose K order were another would miss the fp64 conv of the image."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import conv_edge_draws as ced
import generic_edge_draws as ged
import test_conv_bounds_cpu as tcb
from network_interpretation_imagenet_amd import _lib

F32 = np.float32
KINDS = ("synthetic", "quiet")
_cases, _measured = {}, {}


def images(s):
    """Images of a CPU case: one, or as many as give a few thousand output elements; the classifier: the P + 1 = 257 rows of the largest tile."""
    return 257 if s.f32 else 3 if s.stem_run else 4 if s.d.hout == 7 else 1


def emulated_desc(s):
    """The layer as emulate sees it.  A stem: a 1x1 conv over its gathered runs.  Every other layer: its own conv on cin_pad dense channels.
    The classifier carries the name by which emulate knows an fp32 output."""
    d = s.d
    if s.stem_run:
        return d._replace(cin=ged.k_packed(s), ksize=1, stride=1, pad=0, hin=d.hout)
    return d._replace(cin=ged.pitch_of(d.cin), name="fc" if s.f32 else d.name)


def pack(mpx_lib, sd, s):
    """The library's packer on the row's layer: tcb.pack with the descriptor's k_packed, a conv bias and the family's eps ->
    (w_hi, w_lo [cout][k_packed] fp32 values of the fp16 planes, scale, shift)."""
    d = s.d
    cd = _lib.ConvDesc()
    cd.cin, cd.cout, cd.ksize = d.cin, d.cout, d.ksize
    cd.k_packed = ged.k_packed(s) if s.stem_run else d.ksize ** 2 * ged.pitch_of(d.cin)
    cd.cout_pad = (d.cout + 127) // 128 * 128
    hi = np.zeros((cd.cout_pad, cd.k_packed), dtype=np.uint16)
    lo = np.zeros_like(hi)
    sc, sh = np.zeros(cd.cout_pad, dtype=F32), np.zeros(cd.cout_pad, dtype=F32)
    arr = lambda key: np.ascontiguousarray(sd[key].float().numpy()) if key in sd else None
    w = arr(d.name + ".weight").reshape(d.cout, d.cin, d.ksize, d.ksize)
    if s.affine == "bn":
        args = [arr(d.name + ".bias")] + [arr(d.bn_name + k) for k in (".weight", ".bias", ".running_mean", ".running_var")]
    else:       # engine.load_state_dict: a bias-only layer's bias goes in as beta, DenseNet's conv2 gets nothing at all
        args = [None, None, arr(d.name + ".bias") if s.affine == "bias" else None, None, None]
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    rc = mpx_lib.mpx_pack_conv_weights(C.byref(cd), p(w), *[p(a) for a in args], s.eps, p(hi), p(lo), p(sc), p(sh))
    assert rc == 0
    rows = lambda pl: tcb._row_major(pl, cd.cout_pad, cd.k_packed)
    unpack = lambda pl: rows(pl).view(np.float16)[:d.cout].astype(F32)
    w_hi, w_lo = unpack(hi), unpack(lo)
    top = np.abs(w_hi + w_lo).max(1)
    assert ((top >= 512) & (top < 1024)).all()
    assert not rows(hi)[d.cout:].any() and not rows(lo)[d.cout:].any()             # rows behind the last real channel: zero weights
    return w_hi, w_lo, sc[:d.cout], sh[:d.cout]


def case(row, kind, mixed):
    """The draw of one (row, weights, draw form) and its fp64 reference, computed once: (spec, sd, x, pre, want, B), the last three [M][cout]."""
    key = (row, kind, mixed)
    if key not in _cases:
        s = ged.spec(row)
        sd = ged.state_dict(kind, row.arch)
        x = ged.draws(row, images(s), mixed)
        pre, want, b = (t.reshape(-1, s.d.cout) for t in ged.reference(sd, s, x[2]))
        _cases[key] = (s, sd, x, pre, want, b)
    return _cases[key]


def measure(mpx_lib, row, kind, mixed):
    key = (row, kind, mixed)
    if key not in _measured:
        s, sd, x, pre, want, b = case(row, kind, mixed)
        if s.stem_run:
            xh, xl = ged.staging_patches(s, x[0]), ged.staging_patches(s, x[1])
        else:
            dense = s._replace(x_pitch=ged.pitch_of(s.d.cin), x_offset=0, bf=0, hp=0)
            xh, xl = ged.physical(dense, x[0]), ged.physical(dense, x[1])
        hi, lo = tcb.emulate(emulated_desc(s), pack(mpx_lib, sd, s), xh, xl, None)
        got = torch.from_numpy(hi.astype(np.float64) + (0.0 if s.f32 else lo.astype(np.float64)))
        r_ref = ((got - want).abs() / (2.0 ** -22 * b + (0.0 if s.f32 else 2.0 ** -24))).max().item()
        _measured[key] = (hi, lo, got, r_ref)
    return _measured[key]


ROW_IDS = ["%s-%s" % (r.arch, r.name) for r in ged.FORMS]


@pytest.mark.parametrize("row", ged.FORMS, ids=ROW_IDS)
@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mixed"])
@pytest.mark.parametrize("kind", KINDS)
def test_emulated_arithmetic_stays_inside_the_bound(mpx_lib, row, kind, mixed):
    s, sd, x, pre, want, b = case(row, kind, mixed)
    hi, lo, got, r_ref = measure(mpx_lib, row, kind, mixed)
    print("r_ref %-9s %-16s %-40s nk = %3d %s: %.3f (max norm: %.2e)" % (kind, row.arch, row.name, ged.nk(s), "mixed" if mixed else "plain", r_ref,
                                                                       (got - want).abs().max().item() / max(want.abs().max().item(), 1.0)))
    assert ((got - want).abs() <= ged.tol(b, s)).all()
    assert ced.max_norm_ok(got, want)
    if s.d.relu:
        neg = (pre < -ged.tol(b, s)).numpy()
        assert neg.any() and (hi.view(np.uint16)[neg] == 0).all() and (lo.view(np.uint16)[neg] == 0).all()


def test_c_tol_is_four_times_the_worst_r_ref(mpx_lib):
    worst, where = max((measure(mpx_lib, row, kind, mixed)[3], (row.name, kind, mixed)) for row in ged.FORMS for kind in KINDS for mixed in (False, True))
    print("worst r_ref %.3f at %s over %d cases; recorded %.3f; C_TOL %g" % (worst, where, len(_measured), ged.R_REF_MAX, ged.C_TOL))
    # the recorded figure is the measured one to its three decimals (the emulation sums every K chunk exactly: no order of summation in it)
    assert abs(worst - ged.R_REF_MAX) <= 5e-4, "generic_edge_draws.R_REF_MAX is not what this file measures: %.4f" % worst
    assert ged.C_TOL == 2.0 ** math.ceil(math.log2(4 * worst))
    assert ged.C_TOL is ced.C_TOL


@pytest.mark.parametrize("row", ged.FORMS, ids=ROW_IDS)
@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mixed"])
@pytest.mark.parametrize("kind", KINDS)
def test_preconditions_hold_on_the_reference(row, kind, mixed):
    """Every draw the GPU test makes is (row, synthetic | quiet, plain | mixed): on its first images, the reference alone."""
    s, sd, x, pre, want, b = case(row, kind, mixed)
    assert all(torch.isfinite(t).all() for t in x[:2]) and torch.equal(ced.merge(*ced.split(x[2])), x[2])
    top, small = ced.preconditions(want)
    print("%s %s %s %s: max |want| %.3g, %.1f %% of the elements under 1 %% of it" % (row.arch, kind, row.name, "mixed" if mixed else "plain", top, 100 * small))
    if kind == "quiet":
        ch = ged.quiet_channels(s.d.cout)
        loud = np.setdiff1d(np.arange(s.d.cout), ch)
        bc = b.max(0).values
        assert bc[ch].max() < 2.0 ** -5 * bc[loud].median(), "%s: the quiet channels are not quiet" % row.name
    if mixed and s.stem_run:
        assert x[2][..., 0].abs().max() < 1e-2 and x[2][..., 1].abs().max() > 20
    elif mixed:
        c = s.d.cin
        lin = 1.0 if s.d.relu or s.f32 else 4.0                         # (a linear map layer's draw is times 4)
        assert x[2][..., : c // 4].abs().max() < 1e-2 * lin and x[2][..., c // 4: c // 2].abs().max() > 20 * lin
    if s.stem_run:
        assert not x[2][1].any() and x[2][0].ne(0).double().mean() > x[2][2].ne(0).double().mean() + 0.3      # image 1 keeps nothing, image 2 half


def test_quiet_state_dict_differs_in_the_rows_layers_only():
    for arch in ged.ARCHS:
        a, q = ged.synthetic_state_dict(arch), ged.quiet_state_dict(arch)
        changed = {k for k in a if not torch.equal(a[k], q[k])}
        want = set()
        for s in ged.SPECS.values():
            if s.arch == arch:
                d = s.d
                want |= {d.bn_name + ".weight", d.bn_name + ".bias"} if s.affine == "bn" else {k for k in (d.name + ".weight", d.name + ".bias") if k in a}
        assert changed == want, (arch, changed ^ want)


# ------------------------------------------------------------------------------------------------
# the Specs are the families' topologies
# ------------------------------------------------------------------------------------------------
def _topology(arch):
    import densenet_ref, efficientnet_ref, googlenet_ref, mobilenet_ref, shufflenet_ref, squeezenet_ref
    t = {"mobilenet_v2": lambda: mobilenet_ref.topology()[0], "squeezenet1_1": squeezenet_ref.topology,
         "shufflenet_v2_x1_0": lambda: shufflenet_ref.topology(arch)[0], "densenet121": lambda: densenet_ref.topology(arch)[0],
         "efficientnet_b0": lambda: efficientnet_ref.topology()[0], "googlenet": googlenet_ref.topology}.get(arch)
    return None if t is None else {r[0]: tuple(r) for r in t()}


def test_specs_are_the_families_topologies():
    import googlenet_ref, shufflenet_ref, squeezenet_ref
    for (arch, name), s in ged.SPECS.items():
        d, topo = s.d, _topology(arch)
        if arch == "alexnet":                                           # (tests/alexnet_ref.py has no topology(): torchvision's alexnet.py)
            assert (name, d.cin, d.cout, d.ksize, d.stride, d.pad, d.hin) in {
                ("features.0", 3, 64, 11, 4, 2, 224), ("features.3", 64, 192, 5, 1, 2, 27), ("features.6", 192, 384, 3, 1, 1, 13),
                ("features.8", 384, 256, 3, 1, 1, 13), ("features.10", 256, 256, 3, 1, 1, 13)}
        elif arch == "densenet121":                                     # (name, cin, cout, k, stride, pad, hin, hout, relu)
            assert topo[name] == (name, d.cin, d.cout, d.ksize, d.stride, d.pad, d.hin, d.hout, d.relu)
        else:
            assert topo[name][:11] == tuple(d), (topo[name], d)
        w = ged.synthetic_state_dict(arch)[name + ".weight"]
        assert w.numel() == d.cout * d.cin * d.ksize ** 2
    sq = dict(zip([r[0] for r in squeezenet_ref.topology()], squeezenet_ref.out_slices()))
    gn = dict(zip([r[0] for r in googlenet_ref.topology()], googlenet_ref.out_slices()))
    for (arch, name), s in ged.SPECS.items():
        if arch == "squeezenet1_1":
            assert sq[name] == (s.y_pitch, s.y_offset)
        if arch == "googlenet":
            assert gn[name] == (s.y_pitch, s.y_offset, s.stored)
    assert shufflenet_ref.halves("shufflenet_v2_x1_0") == ((58, 64), (116, 128), (232, 256))
    s = ged.SPECS["shufflenet_v2_x1_0", "conv5.0"]
    assert np.array_equal(ged.in_columns(s), shufflenet_ref.two_half_index(s.bf, s.hp))


def test_every_row_has_the_property_it_is_there_for():
    spec = lambda arch, name: ged.SPECS[arch, name]
    nks = {(r.arch, r.name): ged.nk(ged.spec(r)) for r in ged.FORMS}
    assert [nks[r.arch, r.name] for r in ged.FORMS if r.form == "nk = 1"] == [1, 1, 1]
    assert [nks[r.arch, r.name] for r in ged.FORMS if r.form == "nk = 2 / 3 / 5"] == [2, 3, 5]
    # odd K loops on 7 x 7: MobileNetV2's 160 and DenseNet's 544 channels; conv5 reads 464 channels as a two-half map of 2 x 256: nk = 16,
    # even -- it stays as the whole-two-half-map reader on a 7 x 7 map
    assert [nks[r.arch, r.name] for r in ged.FORMS if r.form == "odd nk on 7x7"] == [5, 17, 16]
    assert nks["alexnet", "features.0"] == 22 and nks["squeezenet1_1", "features.0"] == 3 == nks["mobilenet_v2", "features.0.0"]
    for r in ged.FORMS:
        s = ged.spec(r)
        assert r.tiles == ged.accepted_tiles(s), r                              # every tile mpx_set_conv_tile accepts (the GPU test asks the engine)
        if not r.form.startswith(("odd nk", "bias-only", "patch kernel")):      # sliced, padded and stem layers: the generic tiles and no other
            assert ged.only_generic(s) and r.tiles == ced.GENERIC_TILES, r
        if r.all_classes:
            assert s.d.hout in (7, 13)
    assert [ged.spec(r).stored for r in ged.FORMS if r.form == "narrow / padded store"] == [64, 32, 1000]
    assert ced.patch_tile(spec("densenet121", "features.denseblock4.denselayer1.conv2").d, 6) == "PatchTile1"
    for name in ("features.6", "features.8", "features.10"):            # AlexNet's 13 x 13 layers: both patch kernels, on the 256-pixel tile
        assert [ced.patch_tile(spec("alexnet", name).d, t) for t in (6, 12)] == ["PatchTile0", "PatchTile0"]
        assert ged.accepted_tiles(spec("alexnet", name)) == (0, 1, 2, 4, 6, 7, 12)
    assert ged.classes_of_form("bias-only 5x5 / 3x3", tile=12) == set(ced.RESIDUES)


# ------------------------------------------------------------------------------------------------
# batches
# ------------------------------------------------------------------------------------------------
BATCHES_13 = {128: {"1": 25, "P-1": 103, "0": 128}, 192: {"1": 25, "P-1": 167, "0": 192}, 256: {"1": 153, "P-1": 103, "0": 256}}
BATCHES_7 = {128: {"1": 81, "P-1": 47, "0": 128}, 192: {"1": 145, "P-1": 47, "0": 192}, 256: {"1": 209, "P-1": 47, "0": 256}}
# tile 12 (PatchTile0: 256 pixels x 128 channels) runs a 13 x 13 layer itself from one round of 256 tiles on: 2 cout tiles need 128 pixel
# tiles (193 images and more), 3 cout tiles 86 (129 images); under that launch_patchp hands the launch to tile 6's kernel
BATCHES_13_TILE_12 = {"features.8": {"1": 409, "P-1": 359, "0": 256}, "features.6": {"1": 153, "P-1": 359, "0": 256},
                      "features.10": {"1": 409, "P-1": 359, "0": 256}}


def test_batches_of_every_row_and_tile():
    for row in ged.FORMS:
        s = ged.spec(row)
        for tile in row.tiles:
            p = ced.tile_pixels(s.d, tile)
            got = ged.row_batches(row, tile)
            assert got, (row, tile)
            for cls, batch in got:
                assert ged.plane_bytes(s, batch) <= ged.PLANE_BYTES_CAP, (row, tile, batch)
                assert ged.residue_class(batch * s.d.hout ** 2, p) == cls
                if not s.f32:
                    assert ced.expected_kernels(s.d, tile, batch, False) == 1 << tile
            if s.f32:
                assert [b for _c, b in got] == [1, p - 1, p, p + 1]
            elif s.stem_run:
                assert [b for _c, b in got] == [1, 3]
            elif s.d.hout in (7, 13):
                want = BATCHES_13_TILE_12[row.name] if tile == 12 else (BATCHES_13 if s.d.hout == 13 else BATCHES_7)[p]
                assert ced.edge_batches(s.d, tile) == want
                assert dict(got) == {c: b for c, b in want.items() if ged.plane_bytes(s, b) <= ged.PLANE_BYTES_CAP}, (row, tile, got)
                assert dict(got) == want or tile == 12, (row, tile, got)
            elif s.d.hout % 2 == 0:
                assert got[0][0] == "0" and got[-1][1] == 3 and len(got) == (1 if got[0][1] == 3 else 2), (row, tile, got)
    # what the cap leaves out is generic_edge_draws.KNOWN_HOLES and nothing else
    known = {(form, name, t): set(classes) for form, name, tiles, classes in ged.KNOWN_HOLES for t in tiles}
    assert ged.holes() == known, (ged.holes(), known)
    # a row the issue lists with all three classes meets them on every tile but a known hole, and its form meets them on that tile through
    # another row; every form meets what exists for it under the cap
    for row in ged.FORMS:
        if row.all_classes:
            for tile in row.tiles:
                assert {c for c, _b in ged.row_batches(row, tile)} | known.get((row.form, row.name, tile), set()) == set(ced.RESIDUES), (row, tile)
                assert ged.classes_of_form(row.form, tile=tile) == set(ced.RESIDUES), (row.form, tile)
    want = {f: set(ced.RESIDUES) for f in ged.FORM_NAMES}
    want["nk = 1"] = {"0", "1"}         # a hole: P - 1 exists on the 55 x 55 map alone, at 79 images and more: 153 MB of planes, over the cap
    want["stem on the staging"] = {"0"}                 # 1 and 3 images: 112 x 112 and 55 x 55 x 3 land on P = 128 / 256 or ragged, 111 x 111 ragged
    got = {f: ged.classes_of_form(f) for f in ged.FORM_NAMES}
    print({f: sorted(c) for f, c in got.items()})
    assert got == want
