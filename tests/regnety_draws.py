"""The cases, draws and bound of the group-width-56 instantiation of the any-width grouped 3x3 kernel (csrc/mpx_gconvw.h, tile 18;
regnet_y_8gf's f.b), in one place, by tests/regnet_draws.py's rule: tests/test_gpu_regnety.py runs them through the stand-alone entry
mpx_gconvw3x3_bn_act, tests/test_regnety_cpu.py through the numpy emulation of tests/test_regnet_bounds_cpu.py, and the two cannot drift.
Nothing here needs a GPU.

For CG = 56 a group has RF = 4 row fragments of 16 channels -- one chunk; the rows 56 .. 63 of the last fragment are zero weights that are
never stored --, K = 9 * 56 = 504 is padded to 512, so that the last of the 16 K steps holds 8 padding elements behind tap 8, and a 32-wide K
step straddles taps (56 is no multiple of 32).

Bound, per output element (regnet_draws'): B = |s| (|W| * |x|)_grouped + |shift|, tol = C 2^-22 B + 2^-24, C = 4 x r_ref rounded up to a power of
two, r_ref = the distance of the emulated arithmetic from fp64 in units of 2^-22 B + 2^-24 on these draws; tests/test_regnety_cpu.py re-measures
r_ref on every run and holds it within a factor of two of the record below.  Draws: regnet_draws.draws, seeded by the case's place in CASES.
Weights: He-normal over the fan-in 9 * 56 and the synthetic BatchNorm of synth._bn, seeded by the case as well.

Cases (name: groups, width at pitch, input map, stride -> output map; batches):
  g1      1 group: ONE unit, so three of the workgroup's four waves exit; width 56 at pitch 64
  g3      3 groups, width 168 at pitch 192: a ragged last workgroup (the fourth wave exits), 24 pad channels written as +0
  y8-*    regnet_y_8gf's own group counts 4, 8, 16, 36 (widths 224 .. 2016, pitch = width) on its smallest maps: 7 x 7 stride 1 and
          14 -> 7 stride 2 (49 pixels per image: a wave's 32 pixels straddle images at batch 3)
  m5-*    a 5 x 5 output map at batch 3 (M = 75: 16-pixel tiles cross rows and images, the last tile is ragged), at stride 1 and from a
          9 x 9 map at stride 2 (an odd side)
"""
import math
from collections import OrderedDict

import torch

import regnet_draws as xgd
from network_interpretation_imagenet_amd import synth

CG = 56
TILE = xgd.TILE
FENCE_ROWS = xgd.FENCE_ROWS
SENTINEL_BITS = xgd.SENTINEL_BITS
GDesc = xgd.GDesc
ARCH = "cg56"       # GDesc.arch of a stand-alone case


def _case(name, groups, hin, stride):
    return GDesc(ARCH, name, name + ".bn", groups * CG, CG, groups, stride, hin, (hin - 1) // stride + 1)


CASES = [_case("g1", 1, 7, 1), _case("g3", 3, 7, 1)]
CASES += [_case("y8-g%d-%s" % (g, "7s1" if s == 1 else "14s2"), g, hin, s) for g in (4, 8, 16, 36) for hin, s in ((7, 1), (14, 2))]
CASES += [_case("m5-s1", 3, 5, 1), _case("m5-s2", 3, 9, 2)]
BATCHES = (1, 3)

# r_ref of tests/test_regnety_cpu.py at batch 3, per case
R_REF = {
    "g1": 0.525,
    "g3": 0.675,
    "y8-g4-7s1": 0.812,
    "y8-g4-14s2": 0.569,
    "y8-g8-7s1": 0.622,
    "y8-g8-14s2": 0.612,
    "y8-g16-7s1": 0.698,
    "y8-g16-14s2": 0.715,
    "y8-g36-7s1": 0.934,
    "y8-g36-14s2": 0.651,
    "m5-s1": 0.576,
    "m5-s2": 0.550,
}
# 4 x r_ref rounded up to a power of two
C_TOL = {k: 2.0 ** math.ceil(math.log2(4 * v)) for k, v in R_REF.items()}


def case(name):
    return next(d for d in CASES if d.name == name)


def pitch(width):
    return -(-width // 32) * 32


def draw_seed(d):
    return 9000 + CASES.index(d)


def weights(d):
    """The case's layer as a state_dict: <name>.weight [width][56][3][3] (He-normal over 9 * 56) and <name>.bn.* (synth._bn)."""
    g = torch.Generator().manual_seed(7000 + CASES.index(d))
    sd = OrderedDict()
    synth._conv(sd, d.name, d.cg, d.width, 3, g)
    synth._bn(sd, d.bn_name, d.width, g)
    return sd


def draws(d, batch, device=None):
    return xgd.draws(d, batch, seed=draw_seed(d), device=device)


def reference(sd, d, x):
    return xgd.reference(sd, d, x)


def tol(d, b):
    return C_TOL[d.name] * 2.0 ** -22 * b + 2.0 ** -24


preconditions = xgd.preconditions
