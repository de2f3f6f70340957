"""The generic conv kernel (csrc/mpx_conv.h on tiles 0 / 1 / 2 / 4 / 7) beyond the ResNet shapes: the layers, draws, references and batches of
tests/test_gpu_generic_edges.py (the kernels) and tests/test_generic_bounds_cpu.py (a numpy emulation of their arithmetic), in one place, as
tests/conv_edge_draws.py is for the ResNet layers.  Everything of that module is used unchanged -- Desc, draws, conv64, tol, preconditions,
max_norm_ok, edge_batches, TILE_PIXELS --; what the later families add is here:

  * a layer is a Spec: its Desc plus how its planes are laid out (the channels per input pixel cin_pad, an input slice or a two-half input
    map, the stored output width, an output slice) and what its epilogue folds (BatchNorm with the family's eps and a conv bias, a bias
    alone, or nothing).  The GPU test asserts every field against mpx_conv_info / mpx_conv_out_slice / mpx_conv_in_slice; the CPU test
    against the family's *_ref.topology();
  * FORMS: which layers stand for which code path of the kernel, on every tile mpx_set_conv_tile accepts for them (accepted_tiles: the
    generic ones, and for AlexNet's 13 x 13 layers and DenseNet's conv2 the patch kernels too); KNOWN_HOLES: the residue classes left out;
  * the fp64 reference and the bound B = |s| (|W| * |x|) + |shift| of conv_edge_draws with that epilogue;
  * quiet_state_dict: synthetic weights on which every seventh output channel of a layer, and its last real one, is 2^-8 of its neighbours
    (trained-like statistics exist for the ResNets only: oracle/trained_like.py);
  * the stems' draws (tests/fused_edge_draws.py's recipe on the family's own stem) and their K order in the NHWC4 staging.

C_TOL is conv_edge_draws.C_TOL itself: tests/test_generic_bounds_cpu.py measures r_ref on every row below and asserts that 4 x the worst,
rounded up to a power of two, is that constant."""
import functools
from collections import namedtuple

import numpy as np
import torch

import conv_edge_draws as ced
import fused_edge_draws as fed
from gpu_common import pitch_of

PLANE_BYTES_CAP = 128 << 20                 # hi + lo input and output planes of one case, fences not counted
R_REF_MAX = 1.499                           # tests/test_generic_bounds_cpu.py: the worst of its 104 cases to three decimals, a stem on the mixed draw
C_TOL = ced.C_TOL

Spec = namedtuple("Spec", "arch d cin_pad x_pitch x_offset bf hp stored y_pitch y_offset eps affine f32 stem_run")
Row = namedtuple("Row", "form arch name tiles all_classes")


def _spec(arch, name, bn, cin, cout, k, stride, pad, hin, relu, affine="bn", eps=1e-5, cin_pad=None, x_pitch=None, x_offset=0, bf=0, hp=0,
          stored=None, y_pitch=None, y_offset=0, f32=False, stem_run=0):
    hout = (hin + 2 * pad - k) // stride + 1
    d = ced.Desc(name, bn, cin, cout, k, stride, pad, hin, hout, relu, 0)
    cin_pad = (4 if stem_run else pitch_of(cin)) if cin_pad is None else cin_pad
    stored = (cout if f32 else pitch_of(cout)) if stored is None else stored
    return Spec(arch, d, cin_pad, cin_pad if x_pitch is None else x_pitch, x_offset, bf, hp, stored, stored if y_pitch is None else y_pitch,
                y_offset, eps, affine, f32, stem_run)


_MB, _SQ, _SH, _DN, _EF, _GN, _AX = "mobilenet_v2", "squeezenet1_1", "shufflenet_v2_x1_0", "densenet121", "efficientnet_b0", "googlenet", "alexnet"
_D4 = "features.denseblock4."
SPECS = {(s.arch, s.d.name): s for s in (
    # MobileNetV2: the linear projections store 16 / 24 channels at pitch 32; features.4 reads 144 channels at pitch 160; ReLU6's clamp is the consumer's
    _spec(_MB, "features.0.0", "features.0.1", 3, 32, 3, 2, 1, 224, 1, stem_run=8),
    _spec(_MB, "features.1.conv.1", "features.1.conv.2", 32, 16, 1, 1, 0, 112, 0),
    _spec(_MB, "features.2.conv.2", "features.2.conv.3", 96, 24, 1, 1, 0, 56, 0),
    _spec(_MB, "features.4.conv.2", "features.4.conv.3", 144, 32, 1, 1, 0, 28, 0),
    _spec(_MB, "features.15.conv.0.0", "features.15.conv.0.1", 160, 960, 1, 1, 0, 7, 1),
    _spec(_MB, "classifier.1", "", 1280, 1000, 1, 1, 0, 1, 0, affine="bias", f32=True),
    # SqueezeNet 1.1: bias + ReLU everywhere; the expand convs write halves of a pitch-2e buffer
    _spec(_SQ, "features.0", "", 3, 64, 3, 2, 0, 224, 1, affine="bias", stem_run=8),
    _spec(_SQ, "features.3.squeeze", "", 64, 16, 1, 1, 0, 55, 1, affine="bias"),
    _spec(_SQ, "features.3.expand1x1", "", 16, 64, 1, 1, 0, 55, 1, affine="bias", stored=64, y_pitch=128),
    _spec(_SQ, "features.12.expand1x1", "", 64, 256, 1, 1, 0, 13, 1, affine="bias", y_pitch=512),
    _spec(_SQ, "features.12.expand3x3", "", 64, 256, 3, 1, 1, 13, 1, affine="bias", y_pitch=512, y_offset=256),
    # ShuffleNetV2 x1.0: (bf, hp) = (58, 64) (116, 128) (232, 256); a stride-2 block's branch1.2 writes the first half of the next stage map
    _spec(_SH, "stage2.0.branch1.2", "stage2.0.branch1.3", 24, 58, 1, 1, 0, 28, 1, y_pitch=128),
    _spec(_SH, "stage4.1.branch2.0", "stage4.1.branch2.1", 232, 232, 1, 1, 0, 7, 1, x_pitch=512, x_offset=256),
    _spec(_SH, "stage4.0.branch2.0", "stage4.0.branch2.1", 232, 232, 1, 1, 0, 14, 1, bf=116, hp=128),
    _spec(_SH, "conv5.0", "conv5.1", 464, 1024, 1, 1, 0, 7, 1, cin_pad=512, bf=232, hp=256),
    # DenseNet-121: norm2 + ReLU are conv1's epilogue; conv2 has no epilogue at all
    _spec(_DN, _D4 + "denselayer2.conv1", _D4 + "denselayer2.norm2", 544, 128, 1, 1, 0, 7, 1),
    _spec(_DN, _D4 + "denselayer1.conv2", "", 128, 32, 3, 1, 1, 7, 0, affine="none"),
    # EfficientNet-B0: the projection of features.3.0 stores 40 channels at pitch 64 and reads 144 at pitch 160
    _spec(_EF, "features.3.0.block.3.0", "features.3.0.block.3.1", 144, 40, 1, 1, 0, 28, 0),
    # GoogLeNet: eps 1e-3; a branch's last conv writes its range of the concatenation (inception4d.branch4.1 the 16 pad channels too)
    _spec(_GN, "inception4a.branch3.0.conv", "inception4a.branch3.0.bn", 480, 16, 1, 1, 0, 14, 1, eps=1e-3),
    _spec(_GN, "inception5b.branch2.1.conv", "inception5b.branch2.1.bn", 192, 384, 3, 1, 1, 7, 1, eps=1e-3, y_pitch=1024, y_offset=384),
    _spec(_GN, "inception4d.branch4.1.conv", "inception4d.branch4.1.bn", 512, 64, 1, 1, 0, 14, 1, eps=1e-3, stored=80, y_pitch=544, y_offset=464),
    # AlexNet: bias + ReLU; the 11-wide stem row is a run of 16 pixels, two K steps
    _spec(_AX, "features.0", "", 3, 64, 11, 4, 2, 224, 1, affine="bias", stem_run=16),
    _spec(_AX, "features.3", "", 64, 192, 5, 1, 2, 27, 1, affine="bias"),
    _spec(_AX, "features.6", "", 192, 384, 3, 1, 1, 13, 1, affine="bias"),
    _spec(_AX, "features.8", "", 384, 256, 3, 1, 1, 13, 1, affine="bias"),
    _spec(_AX, "features.10", "", 256, 256, 3, 1, 1, 13, 1, affine="bias"),
)}

G = ced.GENERIC_TILES
G_PATCH = (0, 1, 2, 4, 6, 7, 12)
FORMS = (
    # form, engine architecture, layer, tiles to run (accepted_tiles: every tile mpx_set_conv_tile accepts), whether all three residue classes
    # are asked for on this very layer
    Row("nk = 1", _MB, "features.1.conv.1", G, False),
    Row("nk = 1", _SQ, "features.3.expand1x1", G, False),
    Row("nk = 1", _SH, "stage2.0.branch1.2", G, False),
    Row("nk = 2 / 3 / 5", _SQ, "features.3.squeeze", G, False),
    Row("nk = 2 / 3 / 5", _MB, "features.2.conv.2", G, False),
    Row("nk = 2 / 3 / 5", _MB, "features.4.conv.2", G, False),
    Row("odd nk on 7x7", _MB, "features.15.conv.0.0", G, True),
    Row("odd nk on 7x7", _DN, _D4 + "denselayer2.conv1", G, True),
    Row("odd nk on 7x7", _SH, "conv5.0", G, True),
    Row("narrow / padded store", _EF, "features.3.0.block.3.0", G, False),
    Row("narrow / padded store", _GN, "inception4a.branch3.0.conv", G, False),
    Row("narrow / padded store", _MB, "classifier.1", G, False),
    Row("output slice", _SQ, "features.12.expand1x1", G, True),
    Row("output slice", _SQ, "features.12.expand3x3", G, True),
    Row("output slice", _GN, "inception5b.branch2.1.conv", G, True),
    Row("output slice", _GN, "inception4d.branch4.1.conv", G, False),
    Row("input slice / two-half map", _SH, "stage4.1.branch2.0", G, True),
    Row("input slice / two-half map", _SH, "stage4.0.branch2.0", G, False),
    Row("bias-only 5x5 / 3x3", _AX, "features.3", G, False),
    # the 13 x 13 layers also run the patch kernels (PatchTile0, P = 256), tile 12 as itself from a round of tiles on: 256 images and more on
    # 256 output channels, 153 on 384.  features.8 meets class 0 there under the cap; features.6 adds class 1, features.10 class P - 1
    # (the two stand at the end of the table: a row's place is the seed of its draw)
    Row("bias-only 5x5 / 3x3", _AX, "features.8", G_PATCH, True),
    Row("stem on the staging", _AX, "features.0", G, False),
    Row("stem on the staging", _SQ, "features.0", G, False),
    Row("stem on the staging", _MB, "features.0.0", G, False),
    Row("patch kernel, cout 32", _DN, _D4 + "denselayer1.conv2", (0, 1, 2, 4, 6, 7), True),
    Row("bias-only 5x5 / 3x3", _AX, "features.6", G_PATCH, True),
    Row("bias-only 5x5 / 3x3", _AX, "features.10", G_PATCH, True),
)
FORM_NAMES = tuple(dict.fromkeys(r.form for r in FORMS))
ARCHS = tuple(dict.fromkeys(r.arch for r in FORMS))
STEM_BATCHES = (1, 3)


def spec(row):
    return SPECS[row.arch, row.name]


def only_generic(s):
    """Sliced, padded and stem layers accept the generic tiles and nothing else."""
    return bool(s.stem_run or s.x_offset or s.bf or s.y_pitch != s.stored or s.d.cin % 32 or s.d.cout % 32 or s.stored != s.d.cout)


def accepted_tiles(s):
    """The tiles mpx_set_conv_tile accepts for the layer: eligible() of csrc/mpx_api.hip refuses every kernel with a predicate to an fc, a stem,
    a padded and a sliced layer; every other layer is judged by its descriptor, as conv_edge_draws.accepts judges a ResNet layer."""
    return G if only_generic(s) else tuple(t for t in ced.ALL_TILES if ced.accepts(s.d, t))


# What the batches below leave out, and why (tests/test_generic_bounds_cpu.py pins each; tests/test_gpu_generic_edges.py prints them):
# (form, layer, tiles, classes never run there) -- every one because the smallest batch of the class holds more planes than PLANE_BYTES_CAP.
KNOWN_HOLES = (
    ("nk = 1", "features.3.expand1x1", G, ("P-1", "0")),        # the only nk = 1 layer on an odd map: the FORM never meets P - 1
    ("nk = 2 / 3 / 5", "features.3.squeeze", (0, 1, 4), ("P-1", "0")),   # the 55 x 55 map again: P - 1 met at P = 128 alone (79 images) ...
    ("nk = 2 / 3 / 5", "features.3.squeeze", (2, 7), ("0",)),            # ... and class 0 by the form's other two layers
    ("bias-only 5x5 / 3x3", "features.3", (0, 1), ("0",)),      # met on tiles 2 and 7
    ("bias-only 5x5 / 3x3", "features.8", (12,), ("1", "P-1")),   # tile 12 as itself: met by features.6 (1) and features.10 (P - 1)
    ("bias-only 5x5 / 3x3", "features.6", (12,), ("P-1",)),
    ("bias-only 5x5 / 3x3", "features.10", (12,), ("1",)),
)


def nk(s):
    """K steps of 32 of the layer in the engine."""
    return k_packed(s) // 32


def k_packed(s):
    return s.d.ksize * s.stem_run * 4 if s.stem_run else s.d.ksize ** 2 * s.cin_pad


def draw_seed(row):
    return 100 + FORMS.index(row)


# ------------------------------------------------------------------------------------------------
# batches
# ------------------------------------------------------------------------------------------------
def plane_bytes(s, batch):
    d = s.d
    x = 230 * 230 * 4 if s.stem_run else d.hin * d.hin * s.x_pitch
    return batch * (x + d.hout * d.hout * s.y_pitch) * 4            # (hi + lo fp16, or one fp32 plane: 4 bytes per element)


def row_batches(row, tile, num_cus=ced.NUM_CUS):
    """[(class, batch)] of one (row, tile).  The classifier: 1, P - 1, P and P + 1 rows (conv_edge_draws' fc).  A stem: 1 and 3 images.  Every
    other layer: conv_edge_draws.edge_batches' batch of every residue class that exists and whose planes stay under PLANE_BYTES_CAP, and on a
    map where class 0 alone exists also batch 3 (a ragged last tile of whatever size)."""
    s = spec(row)
    p = ced.tile_pixels(s.d, tile)
    if s.f32:
        return [("1", 1), ("P-1", p - 1), ("0", p), ("1", p + 1)]
    if s.stem_run:
        return [(residue_class(b * s.d.hout ** 2, p), b) for b in STEM_BATCHES]
    classes = ced.edge_batches(s.d, tile, num_cus)
    out = [(c, b) for c, b in classes.items() if b is not None and plane_bytes(s, b) <= PLANE_BYTES_CAP]
    if classes["1"] is None and classes["P-1"] is None and ("0", 3) not in out:
        out.append((residue_class(3 * s.d.hout ** 2, p), 3))
    return out


def residue_class(m, p):
    return {1: "1", p - 1: "P-1", 0: "0"}.get(m % p, "ragged %d" % (m % p))


def classes_of_form(form, num_cus=ced.NUM_CUS, tile=None):
    """The residue classes a form must meet (tile: on that tile): every one some (row, tile) of it reaches."""
    return {c for row in FORMS if row.form == form for t in row.tiles if tile in (None, t) for c, _b in row_batches(row, t, num_cus)
            if c in ced.RESIDUES}


def holes(num_cus=ced.NUM_CUS):
    """{(form, layer, tile): classes that exist for the layer on that tile and that row_batches leaves out} -- KNOWN_HOLES, computed."""
    out = {}
    for row in FORMS:
        s = spec(row)
        if s.f32 or s.stem_run:
            continue
        for t in row.tiles:
            exist = {c for c, b in ced.edge_batches(s.d, t, num_cus).items() if b is not None}
            left = exist - {c for c, _b in row_batches(row, t, num_cus)}
            if left:
                out[row.form, row.name, t] = left
    return out


# ------------------------------------------------------------------------------------------------
# weights
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synthetic_state_dict(arch):
    from network_interpretation_imagenet_amd import synth
    return synth.make_state_dict(arch)


def quiet_channels(cout):
    return sorted(set(range(0, cout, 7)) | {cout - 1})


@functools.lru_cache(maxsize=None)
def quiet_state_dict(arch):
    """synth.make_state_dict(arch) with, for every layer of FORMS in this architecture, every seventh output channel and the last real one
    2^-8 of its neighbours: BatchNorm weight and bias times 2^-8 (scale and shift of the channel, exactly); on a layer without BatchNorm the
    weight row and the bias."""
    sd = {k: v.clone() for k, v in synthetic_state_dict(arch).items()}
    for s in SPECS.values():
        if s.arch != arch:
            continue
        ch = quiet_channels(s.d.cout)
        keys = [s.d.bn_name + ".weight", s.d.bn_name + ".bias"] if s.affine == "bn" else [s.d.name + ".weight", s.d.name + ".bias"]
        for k in keys:
            if k in sd:
                sd[k][ch] *= 2.0 ** -8
    return sd


def state_dict(kind, arch):
    return {"synthetic": synthetic_state_dict, "quiet": quiet_state_dict}[kind](arch)


def affine(sd, s):
    """fp64 (scale, shift) of the layer's epilogue as the packer folds it (include/mpx.h: shift = beta + (conv_bias - mean) gamma / sqrt(var + eps))."""
    d = s.d
    if s.affine == "none":
        return torch.ones(d.cout, dtype=torch.float64), torch.zeros(d.cout, dtype=torch.float64)
    if s.affine == "bias":
        return torch.ones(d.cout, dtype=torch.float64), sd[d.name + ".bias"].double()
    g = sd[d.bn_name + ".weight"].double() / torch.sqrt(sd[d.bn_name + ".running_var"].double() + s.eps)
    cb = sd[d.name + ".bias"].double() if d.name + ".bias" in sd else 0.0
    return g, sd[d.bn_name + ".bias"].double() + (cb - sd[d.bn_name + ".running_mean"].double()) * g


def weight(sd, s):
    d = s.d
    return sd[d.name + ".weight"].double().reshape(d.cout, d.cin, d.ksize, d.ksize)


def reference(sd, s, x):
    """conv_edge_draws.reference with the Spec's epilogue: (pre, want, B) fp64 [batch][hout][hout][cout] from the merged LOGICAL planes x."""
    d, dev = s.d, x.device
    w = weight(sd, s).to(dev)
    sc, shift = (t.to(dev) for t in affine(sd, s))
    pre = ced.conv64(x, w, d) * sc + shift
    b = ced.conv64(x.abs(), w.abs(), d) * sc.abs() + shift.abs()
    return pre, (torch.relu(pre) if d.relu else pre), b


def tol(b, s):
    return ced.tol(b, resplit=not s.f32)


# ------------------------------------------------------------------------------------------------
# draws
# ------------------------------------------------------------------------------------------------
def draws(row, batch, mixed, device=None):
    """-> (hi, lo, merged) LOGICAL planes [batch][hin][hin][cin] of the row's layer: conv_edge_draws.draws (image n seeded by (seed, n) alone;
    a layer without a ReLU gets its dimmed pixels, and a linear map layer dimmed rows on top).  A stem: tests/fused_edge_draws.py's recipe -- image 0 keeps every segment of the 14 x 14
    grid, image 1 none, the others about half; mixed = channel 0 x 1e-3, channel 1 x 8."""
    s = spec(row)
    if not s.stem_run:
        hi, lo, x = ced.draws(s.d, batch, draw_seed(row), mixed, device=device, with_res=False)[0]
        if not s.d.relu and not s.f32:
            # a linear map layer: conv_edge_draws' dimmed pixels leave |shift| (BatchNorm: 0.03 .. 0.15 against a largest output of 1 .. 3), and
            # under a 3 x 3 window nothing at all, so preconditions() fails on the reference.  The draw, not the threshold: the top quarter
            # of every image's rows (and the window's reach) times 2^-10, everything times 4, re-split.
            x = x * 4.0
            x[:, : -(-s.d.hin // 4) + s.d.ksize // 2] *= 2.0 ** -10
            hi, lo = ced.split(x)
            x = ced.merge(hi, lo)
        return hi, lo, x
    from network_interpretation_imagenet_amd import synth
    x = ced.draws(s.d, batch, draw_seed(row), False, device=device, with_res=False)[0][2].clone()
    if mixed:
        x[..., 0] *= 1e-3
        x[..., 1] *= 8.0
    seg = torch.from_numpy(synth.grid_segments().astype(np.int64))
    mask = torch.from_numpy(fed.stem_keep(batch))[:, seg]
    x = x * mask.to(x.device).unsqueeze(-1).to(x.dtype)
    hi, lo = ced.split(x)
    return hi, lo, ced.merge(hi, lo)


def in_columns(s):
    """Physical channel, within a pixel of x_pitch channels, of every logical input channel: behind the slice's offset, or the two-half map's
    l < bf at l, l >= bf at hp + l - bf (include/mpx.h)."""
    l = np.arange(s.d.cin)
    if s.bf:
        return np.where(l < s.bf, l, s.hp + l - s.bf)
    return s.x_offset + l


def physical(s, plane, fill=0.0):
    """A logical plane [..., cin] as the engine reads it: [..., x_pitch] with the pad channels the layer reads as exact zeros and, for an
    input-slice layer, `fill` in the channels in front of the slice (the half it must not read)."""
    out = torch.zeros(plane.shape[:-1] + (s.x_pitch,), dtype=plane.dtype, device=plane.device)
    if s.x_offset:
        out[..., :s.x_offset] = fill
    out[..., torch.from_numpy(in_columns(s)).to(plane.device)] = plane
    return out


def staging_patches(s, x):
    """A stem's input as the kernel walks it (include/mpx.h, mpx_pack_conv_weights): per output pixel and kernel row ky one run of stem_run
    pixels x 4 channels starting at the window's left edge, k = (ky stem_run + px) 4 + c, zeros outside the image (the staging's border) and in
    channel 3.  x: [B][224][224][3] numpy or torch -> [B][hout][hout][ksize stem_run 4]."""
    d, run = s.d, s.stem_run
    x = torch.as_tensor(x)
    reach = max(d.stride * (d.hout - 1) + max(d.ksize, run) + 1, d.hin)
    xp = torch.zeros((x.shape[0], d.pad + reach, d.pad + reach, 4), dtype=x.dtype)
    xp[:, d.pad:d.pad + d.hin, d.pad:d.pad + d.hin, :3] = x
    span = d.stride * (d.hout - 1) + 1
    runs = [xp[:, ky:ky + span:d.stride, px:px + span:d.stride, :] for ky in range(d.ksize) for px in range(run)]
    return torch.cat(runs, dim=-1)
