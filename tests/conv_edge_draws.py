"""The draws, bounds and tile geometry of the ResNet conv kernels' edge tests, in one place: tests/test_gpu_conv_edges.py runs them through
the kernels, tests/test_conv_bounds_cpu.py through a numpy emulation of the kernels' arithmetic, and the two cannot drift.  Nothing here
needs a GPU: a layer is described by its torchvision topology (resnet_layers), and the GPU test asserts that the engine's own descriptors
say the same.

Bound, per output element.  With s = gamma / sqrt(var + eps), shift = beta - mean * s and the layer's own conv (*):
    B   = |s| (|W| * |x|) + |shift| + |res|                      (the dual launch: summed over both branches)
    tol = C_TOL 2^-22 B + 2^-24
The dropped lo x lo product is at most 2^-22 |w| |x|, the weight split 2^-22 |w|, the output re-split 2^-22 |y| with half of lo's fp16
subnormal step (2^-25 <= 2^-24) as the absolute floor, and what is left is the fp32 accumulation.  C_TOL is 4 x the worst distance
r_ref = max err / (2^-22 B + 2^-24) of the numpy emulation of that arithmetic from fp64 (tests/test_conv_bounds_cpu.py measures it on these
draws and asserts that the constant below is what follows from it), rounded up to a power of two; the 4 is the margin this suite gives a
reference's own distance (tests/logits_lens.py: 4 d_L) and has to absorb the MFMA's internal order of summation.  fc writes fp32: the same
bound without the re-split's floor.

Draws.  Image n of a layer's draw is seeded by (seed, n) alone, so it is the same numbers at every batch size: the CPU test checks the
preconditions on images the GPU test uses, and "image 0 launched alone" is a prefix of every batch.  Every value is a valid (hi, lo) pair
and the merged hi + lo planes are the truth the reference starts from."""
import math
from collections import namedtuple

import torch
from gpu_common import merge, split

ALL_TILES = (0, 1, 2, 4, 6, 7, 9, 10, 12, 13, 14)
GENERIC_TILES = (0, 1, 2, 4, 7)
POINTWISE_TILES = (7, 9, 10, 13, 14)        # the 1x1 stride-1 forms of the position-independence check
BN_EPS = 1e-5
NUM_CUS = 256                               # an MI355X; the GPU test passes the engine's own count

# r_ref of tests/test_conv_bounds_cpu.py (numpy 2; per K chunk of 32 the products hi*lo, lo*hi, hi*hi, each summed exactly and rounded to fp32
# once, added to an fp32 accumulator in that order), layer / K: synthetic plain, synthetic mixed, trained-like plain, trained-like mixed
#   layer1.0.conv1         K =   64: 0.629 0.939 0.641 0.917
#   layer1.0.downsample.0  K =   64: 0.828 1.317 0.728 0.991      (no ReLU)
#   layer4.2.conv3         K =  512: 0.371 0.678 0.401 0.791      (residual)
#   layer1.0.conv2         K =  576: 0.380 0.701 0.433 0.631
#   layer4.1.conv1         K = 2048: 0.342 0.809 0.329 0.909
#   layer4.1.conv2         K = 4608: 0.398 0.557 0.312 0.448
#   fc                     K = 2048: 0.353 0.782 0.372 0.904      (fp32 output)
# The worst ones are the short sums on the mixed draws: a few products of the channels scaled by 8 carry the element, so |want| is close to B,
# and the dozen fp32 roundings of a K = 64 sum (two per MFMA in this emulation) walk 3 to 4 ulps of the result.
R_REF_MAX = 1.317
C_TOL = 8.0                                 # 4 x 1.317 = 5.3, rounded up to a power of two

FENCE_ROWS = 256                            # pixel rows of cout elements in front of and behind every output plane
SENTINEL_BITS = 0x7e00                      # an fp16 NaN no kernel produces (tests/test_gpu_squeezenet.py)

Desc = namedtuple("Desc", "name bn_name cin cout ksize stride pad hin hout relu residual")

_DEPTHS = {"resnet18": ("basic", (2, 2, 2, 2)), "resnet50": ("bottleneck", (3, 4, 6, 3)), "resnet101": ("bottleneck", (3, 4, 23, 3))}


def resnet_layers(arch):
    """The conv list of a torchvision ImageNet ResNet behind its stem, in forward order, and fc last (as a 1x1 conv on a 1x1 map)."""
    kind, depths = _DEPTHS[arch]
    exp = 4 if kind == "bottleneck" else 1
    out, cin, h = [], 64, 56
    for s, depth in enumerate(depths):
        w = 64 << s
        for b in range(depth):
            stride = 2 if (b == 0 and s > 0) else 1
            p = "layer%d.%d." % (s + 1, b)
            ds = b == 0 and (stride != 1 or cin != w * exp)
            ho = h // stride
            if kind == "basic":
                out.append(Desc(p + "conv1", p + "bn1", cin, w, 3, stride, 1, h, ho, 1, 0))
                if ds:
                    out.append(Desc(p + "downsample.0", p + "downsample.1", cin, w, 1, stride, 0, h, ho, 0, 0))
                out.append(Desc(p + "conv2", p + "bn2", w, w, 3, 1, 1, ho, ho, 1, 1))
            else:
                out.append(Desc(p + "conv1", p + "bn1", cin, w, 1, 1, 0, h, h, 1, 0))
                out.append(Desc(p + "conv2", p + "bn2", w, w, 3, stride, 1, h, ho, 1, 0))
                if ds:
                    out.append(Desc(p + "downsample.0", p + "downsample.1", cin, w * exp, 1, stride, 0, h, ho, 0, 0))
                out.append(Desc(p + "conv3", p + "bn3", w, w * exp, 1, 1, 0, ho, ho, 1, 1))
            cin, h = w * exp, ho
    out.append(Desc("fc", "", cin, 1000, 1, 1, 0, 1, 1, 0, 0))
    return out


def layer_desc(arch, name):
    return next(d for d in resnet_layers(arch) if d.name == name)


def as_desc(d):
    """An engine's ConvDesc (ctypes) as a Desc."""
    return Desc(d.name.decode(), d.bn_name.decode(), d.cin, d.cout, d.ksize, d.stride, d.pad, d.hin, d.hout, d.relu, d.residual)


def distinct_shapes(arch):
    """One layer per distinct (cin, cout, k, stride, map, residual), fc excluded: tools/stress_parity.distinct_shape_layers' rule."""
    seen, out = set(), []
    for d in resnet_layers(arch)[:-1]:
        key = (d.cin, d.cout, d.ksize, d.stride, d.hin, d.residual)
        if key not in seen:
            seen.add(key)
            out.append(d)
    return out


# ------------------------------------------------------------------------------------------------
# tile geometry: the pixel-tile size P of every kernel form, read off the kernels' configs
# ------------------------------------------------------------------------------------------------
TILE_PIXELS = {
    # tile id: (P, where it was read)
    0: (256, "csrc/mpx_conv.h:580  ConvTile0 = ConvCfg<128, 256, ...>: TP = 256"),
    1: (256, "csrc/mpx_conv.h:581  ConvTile1 = ConvCfg<64, 256, ...>: TP = 256"),
    2: (128, "csrc/mpx_conv.h:582  ConvTile2 = ConvCfg<128, 128, ...>: TP = 128"),
    4: (192, "csrc/mpx_conv.h:583  ConvTile4 = ConvCfg<64, 192, ...>: TP = 192"),
    7: (128, "csrc/mpx_conv.h:588  ConvTile7 = ConvCfg<128, 128, ...>: TP = 128"),
    9: (256, "csrc/mpx_conv256.h:27  Conv256: TP = 256"),
    10: (128, "csrc/mpx_convx.h:32  ConvX: TP = 128"),
    13: (256, "csrc/mpx_conv256p.h:28  Conv256P: TP = 256"),
    14: (64, "csrc/mpx_convw.h:113  ConvWK: TP = 64"),
    # 6 and 12 (csrc/mpx_conv3p.h, mpx_conv3pp.h): a tile is TP CONSECUTIVE output pixels (conv_tiles in csrc/mpx_api.hip counts
    # ceil(M / TP); the patch of a tile may span images, patch_rows_needed), and TP depends on which PatchCfg holds the layer: patch_tile()
}
# csrc/mpx_conv3p.h:340-342: name: (TC, TP, waves, XJP)
PATCH_TILES = {"PatchTile0": (128, 256, 8, 4), "PatchTile1": (64, 256, 4, 8), "PatchTile2": (128, 192, 8, 3)}
LDS_LIMIT = 160 * 1024                      # csrc/mpx_api.hip: kLdsLimit


def patch_rows_needed(h, tp):
    """csrc/mpx_api.hip patch_rows_needed: rows of the largest input patch any TP-pixel tile of an h x h map needs, rounded up to 16."""
    pw, pimg, howo = h + 2, (h + 2) * (h + 2), h * h

    def pb(m):
        n, rem = divmod(m, howo)
        return n * pimg + (rem // h) * pw + rem % h

    worst = max(pb(m0 + tp - 1) - pb(m0) + 2 * pw + 3 for m0 in range(0, tp * howo, tp))
    return (worst + 15) // 16 * 16


def _patch_fits(d, cfg, persistent):
    tc, tp, nw, xjp = PATCH_TILES[cfg]
    if not (d.ksize == 3 and d.stride == 1 and d.pad == 1 and d.cin % 64 == 0 and d.hin == d.hout):
        return False
    rows = patch_rows_needed(d.hin, tp)
    ring = 3 * tc * 128 + 2 * rows * 128 + nw * 1024
    if rows > 16 * nw * xjp or max(ring, tp * tc * 4) > LDS_LIMIT:
        return False
    return not persistent or (d.cout >= 128 and not d.residual and ring + tc * 8 <= LDS_LIMIT)


def patch_tile(d, tile):
    """The PatchCfg name tile 6 / 12 runs layer d on (launch_patch / launch_patchp), or None where the layer is not eligible."""
    if tile == 6 and d.cout <= 64:
        return "PatchTile1" if _patch_fits(d, "PatchTile1", False) else None
    for cfg in ("PatchTile0", "PatchTile2"):
        if _patch_fits(d, cfg, tile == 12):
            return cfg
    return None


def accepts(d, tile):
    """What mpx_set_conv_tile answers for a ResNet layer (the eligibility predicates of csrc/mpx_api.hip; fc runs the generic tiles only)."""
    if tile in GENERIC_TILES:
        return True
    if d.name == "fc":
        return False
    if tile in (6, 12):
        return patch_tile(d, tile) is not None
    c256 = d.ksize == 1 and d.stride == 1 and d.pad == 0 and d.cout % 256 == 0 and d.cin % 64 == 0
    return {9: c256, 10: c256 and d.cin >= 128, 13: c256 and not d.residual, 14: c256 and d.cin == 256}[tile]


def tile_pixels(d, tile):
    if tile in (6, 12):
        return PATCH_TILES[patch_tile(d, tile)][1]
    return TILE_PIXELS[tile][0]


def _tiles(m, cout, tc, tp):
    return -(-m // tp) * -(-cout // tc)


def _persistent_grid(tiles, n_tiles_c, num_cus):
    c = n_tiles_c
    unit = (8 if 8 % c == 0 else 8 * c) if 8 > c else (c if c % 8 == 0 else 8 * c)
    return min(num_cus, tiles) // unit * unit


def _kernels_one(d, tile, m, with_res, num_cus):
    """Bits of mpx_last_conv_kernels for ONE launch_tile over m pixels (the launchers of csrc/mpx_api.hip and their hand-overs)."""
    if tile in GENERIC_TILES or tile in (6, 9):
        return 1 << tile
    if tile == 13 and with_res:
        return 1 << 9
    if tile == 14 and not (d.relu and with_res):
        tile = 10
    if tile == 12:
        tc, tp = PATCH_TILES[patch_tile(d, 12)][:2]
        n_c = -(-d.cout // tc)
        tiles = _tiles(m, d.cout, tc, tp)
        padded = (m // (d.hin * d.hin) + 2) * (d.hin + 2) ** 2
        own = _persistent_grid(tiles, n_c, num_cus) > 0 and tiles >= num_cus and not with_res and padded < (1 << 23)
        return 1 << (12 if own else 6)
    tp = TILE_PIXELS[tile][0]
    tiles = _tiles(m, d.cout, 256, tp)
    own = _persistent_grid(tiles, d.cout // 256, num_cus) > 0 and tiles >= (2 if tile == 14 else 1) * num_cus
    return 1 << (tile if own else (2 if tile == 13 else 7))


def expected_kernels(d, tile, batch, with_res, num_cus=NUM_CUS):
    """Bits of mpx_last_conv_kernels after mpx_conv_bn_act on `tile`: launch_conv's split of the 256x256 rows (the images behind the last
    whole round of tiles go to tile 2) and each launcher's hand-over under its round(s) of tiles."""
    howo = d.hout * d.hout
    m = batch * howo
    if tile in (9, 13):
        tiles_c = -(-d.cout // 256)
        total = -(-m // 256) * tiles_c
        rounds, rest = divmod(total, num_cus)
        n_a = rounds * num_cus // tiles_c * 256 // howo
        if rounds >= 1 and rest > 0 and 2 * rest <= num_cus and 1 <= n_a < batch:
            return _kernels_one(d, tile, n_a * howo, with_res, num_cus) | 1 << 2
    return _kernels_one(d, tile, m, with_res, num_cus)


def expected_dual_kernels(d3, tile, batch, num_cus=NUM_CUS):
    """mpx_conv_dual_bn_act with the main layer d3 on `tile` (launch_conv_fused): the 256-row ids run the dual form of the persistent
    256x256 kernel (bit 13) from one round of tiles on, tile 7's dual kernel below; 2 and 7 their own dual kernels."""
    if tile in (9, 10, 13, 14):
        tiles = _tiles(batch * d3.hout * d3.hout, d3.cout, 256, 256)
        own = _persistent_grid(tiles, d3.cout // 256, num_cus) > 0 and tiles >= num_cus
        return 1 << (13 if own else 7)
    return 1 << (2 if tile == 2 else 7)


RESIDUES = ("1", "P-1", "0")


def edge_batches(d, tile, num_cus=NUM_CUS, with_res=None, dual=False, limit=8192):
    """{"1" / "P-1" / "0": batch}: per residue class of M = batch * hout^2 modulo the tile's pixel count P, the smallest batch that puts M one
    past a tile boundary, one short of it, or on it AND at which the kernel of `tile` itself runs the whole launch (the persistent forms need
    their round(s) of tiles; a split launch would hand the last tile to another kernel).  None where the class does not exist for the layer:
    gcd(hout^2, P) does not divide the residue."""
    with_res = bool(d.residual) if with_res is None else with_res
    if dual and tile in (9, 10, 13, 14):
        tile = 13
    p = tile_pixels(d, tile)
    howo = d.hout * d.hout
    out = {}
    for name, r in zip(RESIDUES, (1, p - 1, 0)):
        if r % math.gcd(howo, p):
            out[name] = None
            continue
        want = 1 << tile
        for b in range(1, limit + 1):
            if b * howo % p != r % p:
                continue
            ran = expected_dual_kernels(d, tile, b, num_cus) if dual else expected_kernels(d, tile, b, with_res, num_cus)
            if ran == want:
                out[name] = b
                break
        else:
            raise ValueError("%s tile %d: no batch up to %d reaches residue %s on the kernel itself" % (d.name, tile, limit, name))
    return out


# ------------------------------------------------------------------------------------------------
# draws
# ------------------------------------------------------------------------------------------------
def _images(shape, seed, batch, dim):
    """fp32 [batch] + shape, image n from a generator seeded by (seed, n) alone.  dim: an eighth of its pixels is multiplied by 2^-10."""
    out = torch.empty((batch,) + shape)
    g = torch.Generator()
    for n in range(batch):
        g.manual_seed(1000003 * seed + n)
        out[n] = torch.randn(shape, generator=g)
        if dim:
            out[n] *= torch.where(torch.rand(shape[:-1] + (1,), generator=g) < 0.125, 2.0 ** -10, 1.0)
    return out


def _draw_planes(shape, seed, batch, mixed, relu_like, dim, device):
    x = _images(shape, seed, batch, dim)
    if device is not None:
        x = x.to(device)                            # (what follows is elementwise IEEE arithmetic: the same bits on either device)
    if relu_like:
        x = x.clamp_min(-0.5) * 1.5                 # mostly post-ReLU-like, as tests/test_gpu_parity.py draws its inputs
    if mixed:
        c = shape[-1]
        x[..., : c // 4] *= 1e-3                    # a band whose lo plane lies in fp16's subnormals
        x[..., c // 4: c // 2] *= 8.0
    hi, lo = split(x)
    return hi, lo, merge(hi, lo)


def draws(d, batch, seed, mixed, device=None, with_res=None):
    """-> ((x_hi, x_lo, x), (r_hi, r_lo, r) or None): the split-fp16 input planes [batch][hin][hin][cin] of layer d with their merged value
    (fp32 holds hi + lo exactly; the references convert it to fp64), and the residual planes [batch][hout][hout][cout] where the layer
    takes one.  The plain form is randn.clamp_min(-0.5) * 1.5; mixed: a quarter of the input channels times 1e-3, another quarter times 8.
    A layer WITHOUT a ReLU (downsample.0, fc) has an eighth of its input pixels (fc: of its rows) dimmed by 2^-10: its output is Gaussian,
    of which only 4 % lie under 1 % of the maximum, and preconditions() asks for 5 % -- the dimmed pixels' outputs are the layer's shift."""
    with_res = bool(d.residual) if with_res is None else with_res
    x = _draw_planes((d.hin, d.hin, d.cin), 2 * seed, batch, mixed, True, not d.relu, device)
    res = _draw_planes((d.hout, d.hout, d.cout), 2 * seed + 1, batch, False, False, False, device) if with_res else None
    return x, res


def draw_seed(arch, name):
    """The seed of a layer's draw in both test files: its place in the network."""
    return [d.name for d in resnet_layers(arch)].index(name) + 1


# the layers on which every residue class that exists is run, per kernel form: the smallest that serve, and a 7 x 7 layer wherever the
# form accepts one (49 is coprime to every P, so all three classes exist there; on the larger maps only M = 0 mod P does)
FORM_LAYERS = {
    0: ("layer2.0.conv2", "layer4.1.conv2"),
    1: ("layer1.0.conv2", "layer4.1.conv1"),
    2: ("layer2.0.downsample.0", "layer4.1.conv1"),
    4: ("layer1.1.conv1", "layer4.1.conv1"),
    6: ("layer1.1.conv2", "layer4.1.conv2"),
    7: ("layer1.1.conv3", "layer4.2.conv3"),
    9: ("layer4.1.conv1",),
    10: ("layer2.1.conv3", "layer4.2.conv3"),
    12: ("layer2.1.conv2", "layer4.1.conv2"),
    13: ("layer4.1.conv1",),
    14: ("layer3.5.conv3",),
}
R18_RESIDUAL_LAYERS = ("layer1.0.conv2", "layer3.1.conv2")      # BasicBlock 3x3 layers that take a residual: tiles 0, 1, 2 and 6
R18_HANDOVER_LAYER = "layer3.1.conv1"                           # accepts tile 12; called WITH a residual operand it must run tile 6's kernel
QUIET_CHANNEL_LAYERS = ("layer1.0.downsample.0", "layer3.0.downsample.0")     # trained-like ResNet-101: channels with B under 1 % of the largest
DUAL_STAGES = (2, 4)
DUAL_TILES = (2, 7, 13)


# ------------------------------------------------------------------------------------------------
# fp64 reference and bound
# ------------------------------------------------------------------------------------------------
def bn_affine(sd, d):
    """fp64 (s, shift) of layer d: BatchNorm folded as the packer folds it; fc: (1, bias)."""
    if not d.bn_name:
        return torch.ones(d.cout, dtype=torch.float64), sd[d.name + ".bias"].double()
    s = sd[d.bn_name + ".weight"].double() / torch.sqrt(sd[d.bn_name + ".running_var"].double() + BN_EPS)
    return s, sd[d.bn_name + ".bias"].double() - sd[d.bn_name + ".running_mean"].double() * s


def conv64(x, w, d, chunk_elems=1 << 25):
    """The layer's own conv in fp64 as one matrix product per tap: x [B][hin][hin][cin] (any float type), w fp64 [cout][cin][k][k] ->
    fp64 [B][hout][hout][cout].  Works on the CPU and on the device alike (no conv library in between)."""
    b = x.shape[0]
    k, s, ho = d.ksize, d.stride, d.hout
    out = torch.empty((b, ho, ho, d.cout), dtype=torch.float64, device=x.device)
    step = max(1, chunk_elems // (d.hin * d.hin * d.cin))
    for n0 in range(0, b, step):
        xc = x[n0:n0 + step].double()
        if d.pad:
            xc = torch.nn.functional.pad(xc, (0, 0, d.pad, d.pad, d.pad, d.pad))
        acc = None
        for ky in range(k):
            for kx in range(k):
                tap = xc[:, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (ho - 1) + 1:s, :].reshape(-1, d.cin)
                y = tap @ w[:, :, ky, kx].t()
                acc = y if acc is None else acc + y
        out[n0:n0 + step] = acc.view(-1, ho, ho, d.cout)
    return out


def reference(sd, d, x, res):
    """-> (pre, want, bound): the fp64 pre-activation s conv(x) + shift (+ res), want = ReLU(pre) where the layer has one, and the
    per-element B of the module docstring.  x / res: merged planes, on whichever device they live."""
    dev = x.device
    w = sd[d.name + ".weight"].double().reshape(d.cout, d.cin, d.ksize, d.ksize).to(dev)
    s, shift = (t.to(dev) for t in bn_affine(sd, d))
    pre = conv64(x, w, d) * s + shift
    b = conv64(x.abs(), w.abs(), d) * s.abs() + shift.abs()
    if res is not None:
        pre = pre + res.double()
        b = b + res.double().abs()
    return pre, (torch.relu(pre) if d.relu else pre), b


def dual_reference(sd, d3, dd, t2, x):
    """mpx_conv_dual_bn_act: relu(bn3(conv3(t2)) + bn_ds(conv_ds(x))); B is the sum over both branches."""
    p3, _, b3 = reference(sd, d3._replace(relu=0), t2, None)
    pd, _, bd = reference(sd, dd, x, None)
    pre = p3 + pd
    return pre, torch.relu(pre), b3 + bd


def bound(sd, d, x64, res64):
    return reference(sd, d, x64, res64)[2]


def tol(b, resplit=True):
    return C_TOL * 2.0 ** -22 * b + (2.0 ** -24 if resplit else 0.0)


def max_norm_ok(got, want):
    """The suite's older check (tests/test_gpu_parity.py _check_layer): one number per tensor."""
    return (got - want).abs().max().item() <= 4e-6 * max(want.abs().max().item(), 1.0)


def preconditions(want):
    """On the reference alone: no hi plane can overflow fp16, and at least 5 % of the elements are small next to the largest one, so that the
    per-element bound has something the max norm does not see.  -> (max |want|, share of small elements)"""
    top = want.abs().max().item()
    small = (want.abs() < 1e-2 * top).double().mean().item()
    assert top < 3e4, "max |want| = %g: a hi plane could overflow" % top
    assert small >= 0.05, "only %.1f %% of the elements are under 1 %% of the largest" % (100 * small)
    return top, small
