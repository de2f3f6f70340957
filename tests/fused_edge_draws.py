"""The draws, batches, references and bounds of the fused launches' edge tests -- layer1's block tails (mpx_bottleneck_tail), layer2's pointwise
tails (mpx_pointwise_tail) and the ImageNet stem with and without its max pool -- in one place: tests/test_gpu_fused_edges.py runs them through
the kernels, tests/test_fused_bounds_cpu.py through the numpy emulation of tests/test_conv_bounds_cpu.py applied layer after layer.  Everything
a single layer needs (draws, fp64 reference, B, tol, preconditions) is conv_edge_draws'; this module adds the chains.  No GPU.

Bounds, all tol = c 2^-22 B + 2^-24 with B as in conv_edge_draws:
  * an output ONE layer away from planes the test can see takes c = ced.C_TOL unchanged: the pointwise tail's block output (from t2 and x, both
    inputs), either tail's next-conv1 output against the fp64 conv1' of the launch's OWN STORED block output (the kernel feeds conv1' exactly
    the hi / lo it stores), the stem conv;
  * the stem + pool output: max is 1-Lipschitz, so |got - want| <= the largest tol among the window's valid taps, and +0 where every valid
    tap's pre-activation is below -tol;
  * the block tail's block output has conv2's output (and, with t1 = NULL, conv1's) hidden in the launch: c = C_CHAIN against the fp64 chain
    whose intermediate tensors are rounded to hi + lo where the kernel re-splits them, B = the last layer's B3 (+ B_ds, + |identity|).

C_CHAIN follows 19's rule from the chain emulation of tests/test_fused_bounds_cpu.py: 4 x the worst r_chain = max err / (2^-22 B + 2^-24),
rounded up to a power of two; the CPU test asserts that the constant below is what it measures."""
from collections import namedtuple

import numpy as np
import torch

import conv_edge_draws as ced

ARCH = "resnet101"
STEM = ced.Desc("conv1", "bn1", 3, 64, 7, 2, 3, 224, 112, 1, 0)
IMG, IMG_PAD = 224, 230                     # the stem's input staging is [n][230][230][4]: a 3-pixel zero border, a zero 4th channel

# r_chain of tests/test_fused_bounds_cpu.py (the numpy emulation of the three or four layers of a tail, each fed the emulated hi / lo of the one
# before, against the fp64 chain), one image: synthetic plain, synthetic mixed, trained-like plain, trained-like mixed
#   layer1.0 whole (conv1 -> conv2 -> conv3 + downsample)   0.831 1.236 0.856 1.125
#   layer1.0 with t1 given (conv2 -> conv3 + downsample)    0.781 1.313 0.949 1.131
#   layer1.1 (conv2 -> conv3 + identity)                    0.758 0.982 0.976 1.173
#   layer1.2 (conv2 -> conv3 + identity)                    0.832 0.963 0.975 1.327
# The single layers of conv_edge_draws reach 1.317 (a K = 64 sum on the mixed draws): the chain's worst is no larger.  What t2's error becomes
# behind conv3 costs less than the last layer's own fp32 roundings (layer1.1 trained-like mixed: 0.74 with the reference's t2, 1.17 as a chain).
R_CHAIN_MAX = 1.327
C_CHAIN = 8.0                               # 4 x 1.327 = 5.3, rounded up to a power of two

# ------------------------------------------------------------------------------------------------
# geometry of the three launches, read off the code
# ------------------------------------------------------------------------------------------------
GEOMETRY = {
    "block tail": "csrc/mpx_btail.h:99  BT_TY = 8, BT_TX = 14: a tile is 8 x 14 pixels of one image; csrc/mpx_api.hip:2014-2023 launch_btail: "
                  "tiles_per_img = (56 / 8) * (56 / 14) = 28, grid = min(2 CUs / 8 * 8, ceil8(28 B)); mpx_btail.h:209-211: workgroup v walks tiles v, v + grid, ...",
    "pointwise tail": "csrc/mpx_btail.h:775  BtPwCfg::TP = 128 consecutive pixels; csrc/mpx_api.hip:2050-2055 launch_ptail: tiles = ceil(784 B / 128), "
                      "grid = min(2 CUs, tiles); mpx_btail.h:821: workgroup g walks tiles g, g + grid, ...",
    "stem + pool": "csrc/mpx_conv.h:148  POOL_PY = 7, POOL_PX = 8 pooled pixels per workgroup; csrc/mpx_api.hip:1928 launch_stem_pool: "
                   "B * (56 / 7) * (56 / 8) = 56 B workgroups, one tile each (not persistent)",
}
BT_TY, BT_TX, BT_MAP = 8, 14, 56
BT_TILES_PER_IMAGE = (BT_MAP // BT_TY) * (BT_MAP // BT_TX)          # 28
PT_TP, PT_MAP = 128, 28
PT_PIXELS = PT_MAP * PT_MAP                                         # 784
POOL_PY, POOL_PX = 7, 8
POOL_BLOCKS_PER_IMAGE = (56 // POOL_PY) * (56 // POOL_PX)           # 56
STEM_TILES = ced.GENERIC_TILES              # layer 0 runs the generic kernel only (csrc/mpx_api.hip eligible(): the other rows refuse a stem)


def tail_tiles(batch):
    return BT_TILES_PER_IMAGE * batch


def tail_grid(batch, num_cus=ced.NUM_CUS):
    return min(2 * num_cus // 8 * 8, -(-tail_tiles(batch) // 8) * 8)


def tail_batches(num_cus=ced.NUM_CUS):
    """One image (fewer tiles than the grid rounded up to 8: workgroups without a tile), the first batch at which a workgroup walks a second
    tile (the weight ring and the next-patch request cross a tile boundary), the first with a third."""
    resident = 2 * num_cus // 8 * 8
    return [1] + [next(b for b in range(1, 1 << 20) if tail_tiles(b) > k * resident) for k in (1, 2)]


def ptail_tiles(batch):
    return -(-PT_PIXELS * batch // PT_TP)


def ptail_grid(batch, num_cus=ced.NUM_CUS):
    return min(2 * num_cus, ptail_tiles(batch))


def ptail_ragged(batch):
    """Pixels of the launch's last tile where it is not whole; 0: the launch ends on a tile boundary."""
    return PT_PIXELS * batch % PT_TP


def ptail_batches(num_cus=ced.NUM_CUS):
    """The smallest batches with the smallest ragged last tile, the largest one, none at all (rows == TP in tile_rsrc), and with more tiles than
    workgroups (second tiles)."""
    sizes = sorted({ptail_ragged(b) for b in range(1, PT_TP + 1)} - {0})
    first = lambda ok: next(b for b in range(1, 1 << 20) if ok(b))
    return [first(lambda b: ptail_ragged(b) == sizes[0]), first(lambda b: ptail_ragged(b) == sizes[-1]), first(lambda b: ptail_ragged(b) == 0),
            first(lambda b: ptail_tiles(b) > 2 * num_cus)]


def stem_batches(tile):
    """One image, and the smallest batch that ends on a boundary of the tile's P pixels (112^2 = 49 * 256: one image wherever P divides 256)."""
    p = ced.TILE_PIXELS[tile][0]
    whole = next(b for b in range(1, p + 1) if b * STEM.hout * STEM.hout % p == 0)
    return sorted({1, whole})


# ------------------------------------------------------------------------------------------------
# the layers of a tail
# ------------------------------------------------------------------------------------------------
Tail = namedtuple("Tail", "k d1 d2 d3 dd dn")          # dd: the downsample conv (layer1.0) or None; dn: the next block's conv1


def block_tail(k, arch=ARCH):
    """The layers of layer1.k's tail: conv1 (run in the launch only when t1 = NULL), conv2, conv3 (+ downsample), the next block's conv1."""
    L = lambda n: ced.layer_desc(arch, n)
    p = "layer1.%d." % k
    nxt = "layer1.%d.conv1" % (k + 1) if k < 2 else "layer2.0.conv1"
    return Tail(k, L(p + "conv1"), L(p + "conv2"), L(p + "conv3"), L(p + "downsample.0") if k == 0 else None, L(nxt))


PTail = namedtuple("PTail", "k d3 dn")


def pointwise_tail(k, arch="resnet50"):
    """Pair k (1-based block index) of layer2: layer2.k.conv3 + layer2.(k+1).conv1."""
    return PTail(k, ced.layer_desc(arch, "layer2.%d.conv3" % k), ced.layer_desc(arch, "layer2.%d.conv1" % (k + 1)))


# ------------------------------------------------------------------------------------------------
# draws (all through ced.draws: image n is seeded by (seed, n) alone)
# ------------------------------------------------------------------------------------------------
def tail_draws(t, batch, mixed, device=None, arch=ARCH):
    """-> (t1, x): (hi, lo, merged) planes.  t1 [B][56][56][64] is conv2's draw; x is the downsample conv's draw [B][56][56][64] (layer1.0: the
    block input, which a launch with t1 = NULL also runs conv1 on) or conv3's residual draw [B][56][56][256]."""
    t1, _ = ced.draws(t.d2, batch, ced.draw_seed(arch, t.d2.name), mixed, device=device)
    if t.dd is not None:
        x, _ = ced.draws(t.dd, batch, ced.draw_seed(arch, t.dd.name), mixed, device=device)
    else:
        _, x = ced.draws(t.d3, batch, ced.draw_seed(arch, t.d3.name), mixed, device=device, with_res=True)
    return t1, x


def ptail_draws(t, batch, mixed, device=None, arch="resnet50"):
    """-> (t2, x): conv3's own draw, [B][28][28][128] and the identity [B][28][28][512]."""
    return ced.draws(t.d3, batch, ced.draw_seed(arch, t.d3.name), mixed, device=device, with_res=True)


def stem_keep(batch, seed=20):
    """bool [batch][196]: which segments of synth.grid_segments() image n keeps.  Image 0 keeps all, image 1 none, the others about half."""
    keep = np.ones((batch, 196), dtype=bool)
    for n in range(1, batch):
        keep[n] = np.random.default_rng((seed, n)).random(196) < 0.5 if n > 1 else False
    return keep


def stem_draws(batch, mixed, device=None):
    """-> (hi, lo, merged) [B][224][224][3]: conv_edge_draws' plain draw of the stem (mixed: channel 0 x 1e-3, channel 1 x 8 -- three channels
    have no quarters), the pixels of removed segments zeroed in all channels as K0 does, re-split."""
    from network_interpretation_imagenet_amd import synth
    x = ced.draws(STEM, batch, 0, False, device=device)[0][2].clone()
    if mixed:
        x[..., 0] *= 1e-3
        x[..., 1] *= 8.0
    seg = torch.from_numpy(synth.grid_segments().astype(np.int64))
    mask = torch.from_numpy(stem_keep(batch))[:, seg]                   # [B][224][224]
    x = x * mask.to(x.device).unsqueeze(-1).to(x.dtype)
    hi, lo = ced.split(x)
    return hi, lo, ced.merge(hi, lo)


# ------------------------------------------------------------------------------------------------
# fp64 references
# ------------------------------------------------------------------------------------------------
def round_split(x64):
    """What a tensor becomes where a kernel stores it as hi + lo fp16 planes (from its fp32 value) -> merged fp32."""
    return ced.merge(*ced.split(x64.float()))


def tail_reference(sd, t, t1, x, whole=False):
    """The block output of a tail: (pre, want, B) of relu(bn3(conv3(t2)) + identity) with t2 = relu(bn2(conv2(t1))) rounded to hi + lo and, for
    whole, t1 = relu(bn1(conv1(x))) rounded likewise.  t1 / x: merged planes.  B is the LAST layer's (both branches, or + |identity|)."""
    if whole:
        t1 = round_split(ced.reference(sd, t.d1, x, None)[1])
    t2 = round_split(ced.reference(sd, t.d2, t1, None)[1])
    if t.dd is not None:
        return ced.dual_reference(sd, t.d3, t.dd, t2, x)
    return ced.reference(sd, t.d3, t2, x)


def next_reference(sd, dn, out_merged):
    """The next block's conv1 on the launch's own stored block output (merged hi + lo, [B][h][h][cout])."""
    return ced.reference(sd, dn, out_merged, None)


def pool_reference(pre, want, b):
    """3x3 stride-2 pad-1 max pool of the stem conv's [B][112][112][64] reference -> (want, tol, surely_zero) [B][56][56][64]: the pooled value,
    the largest tol among the window's valid taps, and whether every valid tap's pre-activation is below -tol."""
    pool = lambda t: torch.nn.functional.max_pool2d(t.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)     # (pads with -inf)
    tol = ced.tol(b)
    return pool(want), pool(tol), pool(pre + tol) < 0


def tol_chain(b):
    return C_CHAIN * 2.0 ** -22 * b + 2.0 ** -24
