"""Draws, path classifier, exact emulation and per-element bounds for the stem by superposition (csrc/mpx_stemtab.h), shared by
tests/test_stemtab_bounds_cpu.py and tests/test_gpu_stem_table_edges.py so that the two cannot drift.

classify()   numpy restatement of st_tap_label / st_first_occurrences (the CSR table's off / lab) and of stem_pixel / stem_heavy: which of the
             apply launch's paths (I1 I2 I3 I4 I6 = stem_apply_fast<K, false>, B2 B4 = <K, true>, heavy = the streaming launch) a pooled
             pixel takes, with interior / kmax / n_e / n_empty.
emulate()    the header's arithmetic to the letter: K0's fp32 normalisation, one fp32 FMA chain per table entry over its taps in raster
             order (channels 0, 1, 2), v = v + R over a conv pixel's kept entries in entry order, y = max(fma(v, s, t), 0) with s / t computed
             in double and rounded once, the 3x3 stride-2 pool over the conv pixels inside the map, split_f32.  No path of the kernel
             computes anything else: the static paths multiply by 1.0 / 0.0 (exact), the streaming path's empty conv pixel is max(t, 0) =
             max(fma(0, s, t), 0).  The lo plane's -0 (a negative residual that underflows fp16) is stored as +0
             (stem_split_packed).  The result is compared BIT FOR BIT with the kernel's two planes.
reference()  fp64 normalise -> mask -> conv1 -> bn1 -> relu -> maxpool, with the per-element bound (u = 2^-24)
                 n_q   = 3 * (kept in-map taps of conv pixel q's window) + (kept entries of q) + 1
                 tol_q = 1.01 * n_q * u * (|s| * (|W| (*) |x * keep|) + |t|)
                 tol   = max over the window's valid conv pixels of tol_q  +  2^-22 * |want| + 2^-24
             Every product w * x * s passes one rounding per FMA of its entry's chain behind it (at most 3 per kept tap), one per
             add of a kept entry behind the first (the first add, to 0, is exact), the BatchNorm FMA's and the rounding of s to fp32: at most
             n_q, and gamma_n <= 1.01 * n * u for n <= 10^5.  t is rounded once and passes the BatchNorm FMA: 2 <= n_q.  max over a window is
             1-Lipschitz, so the pooled error is at most the largest tol_q; 2^-22 * |want| + 2^-24 is the hi + lo split (two fp16 roundings
             of an fp32 value, the second with fp16's subnormal spacing).  A worst-case count, not a fitted constant.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from network_interpretation_imagenet_amd import synth
from network_interpretation_imagenet_amd.engine import BN_EPS, MEAN, STD

ST_IN, ST_CONV, ST_POOLED, ST_TAPS, ST_C = 224, 112, 56, 49, 64
ST_NPIX = ST_CONV * ST_CONV
SA_CH = 32                      # entries per chunk of the streaming launch
U = 2.0 ** -24
SENTINEL = 0x7e00               # an fp16 NaN no kernel produces
PATHS = ("I1", "I2", "I3", "I4", "I6", "B2", "B4", "heavy")
f32, f64 = np.float32, np.float64


# ----------------------------------------------------------------------------------------------------------------------------------------
# the table's geometry: st_tap_label, st_first_occurrences, the CSR arrays
# ----------------------------------------------------------------------------------------------------------------------------------------
class Table:
    """tap_lab[q][t] (label or -1), tap_pix[q][t] (input pixel, 0 where the tap is in the padding), tap_ent[q][t] (CSR entry of the tap or
    -1), cnt[q], off[q + 1], lab[e], ent_q[e] (conv pixel of entry e), ent_k[e] (its rank under that pixel)."""


@functools.lru_cache(maxsize=8)
def _tap_geometry():
    q = np.arange(ST_NPIX)
    oy, ox = q // ST_CONV, q % ST_CONV
    t = np.arange(ST_TAPS)
    ky, kx = t // 7, t % 7
    iy = 2 * oy[:, None] - 3 + ky[None, :]
    ix = 2 * ox[:, None] - 3 + kx[None, :]
    inmap = (iy >= 0) & (iy < ST_IN) & (ix >= 0) & (ix < ST_IN)
    pix = np.where(inmap, iy * ST_IN + ix, 0)
    return inmap, pix


def build_table(seg, S):
    seg = np.asarray(seg, dtype=np.int64).reshape(-1)
    inmap, pix = _tap_geometry()
    l = seg[pix]
    tap_lab = np.where(inmap & (l >= 0) & (l < S), l, -1)                   # st_tap_label
    # st_first_occurrences: tap t is a first occurrence when its label is valid and occurs at no earlier tap
    eq = tap_lab[:, :, None] == tap_lab[:, None, :]                           # [q][t][t']
    t0 = eq.argmax(axis=2)                                                    # the first tap that carries tap t's label (eq[q][t][t] holds)
    first = (tap_lab >= 0) & (t0 == np.arange(ST_TAPS)[None, :])
    rank = np.cumsum(first, axis=1) - 1
    tb = Table()
    tb.S = int(S)
    tb.tap_lab, tb.tap_pix = tap_lab, pix
    tb.cnt = first.sum(axis=1).astype(np.int64)
    tb.off = np.concatenate([[0], np.cumsum(tb.cnt)]).astype(np.int64)
    tb.tap_ent = np.where(tap_lab >= 0, tb.off[:-1, None] + np.take_along_axis(rank, t0, axis=1), -1)
    qq, tt = np.nonzero(first)                                               # row-major: q ascending, taps in raster order = CSR order
    tb.lab = tap_lab[qq, tt]
    tb.ent_q = qq
    tb.ent_k = rank[qq, tt]
    return tb


# ----------------------------------------------------------------------------------------------------------------------------------------
# stem_pixel / stem_heavy per pooled pixel
# ----------------------------------------------------------------------------------------------------------------------------------------
def classify(tb):
    """dict of [56][56] arrays: path (index into PATHS), interior, kmax, n_e, n_empty, chunk_start (heavy: an entry at a stream position
    cb > 0, cb a multiple of 32, is the first of its conv pixel -- the `cb + i > 0` rule of stem_load_chunk at i = 0), and len9 [56][56][9]
    (entries of conv pixel 3 r + c of the window, 0 where absent) with qok [56][56][9]."""
    off = tb.off
    path = np.zeros((ST_POOLED, ST_POOLED), dtype=np.int64)
    out = {k: np.zeros((ST_POOLED, ST_POOLED), dtype=np.int64) for k in ("kmax", "n_e", "n_empty")}
    interior = np.zeros((ST_POOLED, ST_POOLED), dtype=bool)
    chunk_start = np.zeros((ST_POOLED, ST_POOLED), dtype=bool)
    len9 = np.zeros((ST_POOLED, ST_POOLED, 9), dtype=np.int64)
    qok9 = np.zeros((ST_POOLED, ST_POOLED, 9), dtype=bool)
    for py in range(ST_POOLED):
        for px in range(ST_POOLED):
            # stem_pixel: the three CSR row ranges, columns max(2px-1, 0) .. 2px+1
            cx0 = max(2 * px - 1, 0)
            ncol = 2 * px + 1 - cx0 + 1
            n_empty, lens_stream = 0, []
            rows = []
            for r, cy in enumerate((2 * py - 1, 2 * py, 2 * py + 1)):
                ok = cy >= 0
                q0 = (cy if ok else 0) * ST_CONV + cx0
                e = [int(off[q0]), int(off[q0 + 1]), int(off[q0 + 2]), int(off[q0 + ncol])]
                ln = e[3] - e[0] if ok else 0
                rows.append((e, ln, ok))
                if ok:
                    n_empty += (e[1] == e[0]) + (e[2] == e[1]) + (ncol == 3 and e[3] == e[2])
                    lens_stream += [e[j + 1] - e[j] for j in range(ncol)] if ncol == 3 else [e[1] - e[0], e[3] - e[1]]
            n_e = sum(ln for _e, ln, _ok in rows)
            col0_ok, row0_ok = px > 0, py > 0
            for r, (e, ln, ok) in enumerate(rows):
                e4 = [e[0], e[1], e[2], e[0] + ln]
                for c in range(3):
                    cok = col0_ok or c > 0
                    j = (c if col0_ok else c - 1) if cok else 0
                    qok = cok and (row0_ok or r > 0)
                    qok9[py, px, 3 * r + c] = qok
                    len9[py, px, 3 * r + c] = e4[j + 1] - e4[j] if qok else 0
            kmax = int(len9[py, px].max())
            inter = col0_ok and row0_ok
            heavy = not (kmax <= 6 and (kmax <= 4 or inter))                  # stem_heavy
            if heavy:
                p = PATHS.index("heavy")
                starts = np.cumsum([0] + [n for n in lens_stream if n > 0])[:-1]
                chunk_start[py, px] = bool(((starts > 0) & (starts % SA_CH == 0)).any())
            elif inter:
                p = PATHS.index("I1" if kmax <= 1 else "I2" if kmax <= 2 else "I3" if kmax <= 3 else "I4" if kmax <= 4 else "I6")
            else:
                p = PATHS.index("B2" if kmax <= 2 else "B4")
            path[py, px] = p
            interior[py, px] = inter
            out["kmax"][py, px], out["n_e"][py, px], out["n_empty"][py, px] = kmax, n_e, n_empty
    out.update(path=path, interior=interior, chunk_start=chunk_start, len9=len9, qok=qok9)
    return out


def populations(cl):
    """{class name: number of pooled pixels} for the classes the crafted map must populate."""
    path, kmax, n_e, n_empty, inter = cl["path"], cl["kmax"], cl["n_e"], cl["n_empty"], cl["interior"]
    heavy = path == PATHS.index("heavy")
    n_valid = cl["qok"].sum(axis=2)
    pop = {name: int((path == i).sum()) for i, name in enumerate(PATHS)}
    pop["I6 kmax=5"] = int(((path == PATHS.index("I6")) & (kmax == 5)).sum())
    pop["I6 kmax=6"] = int(((path == PATHS.index("I6")) & (kmax == 6)).sum())
    pop["B4 kmax=3"] = int(((path == PATHS.index("B4")) & (kmax == 3)).sum())
    pop["B4 kmax=4"] = int(((path == PATHS.index("B4")) & (kmax == 4)).sum())
    pop["heavy interior"] = int((heavy & inter).sum())
    pop["heavy border kmax>=7"] = int((heavy & ~inter & (kmax >= 7)).sum())
    pop["heavy border kmax 5..6"] = int((heavy & ~inter & (kmax >= 5) & (kmax <= 6)).sum())
    pop["heavy n_empty>0"] = int((heavy & (n_empty > 0)).sum())
    pop["heavy n_e<=32"] = int((heavy & (n_e <= 32)).sum())
    pop["heavy 32<n_e<=64"] = int((heavy & (n_e > 32) & (n_e <= 64)).sum())
    pop["heavy n_e>64"] = int((heavy & (n_e > 64)).sum())
    pop["heavy chunk start"] = int((heavy & cl["chunk_start"]).sum())
    pop["static some empty"] = int((~heavy & (n_empty > 0) & (n_empty < n_valid)).sum())
    pop["static n_e=0"] = int((~heavy & (n_e == 0)).sum())
    for i, name in enumerate(PATHS[:-1]):
        pop["%s some empty" % name] = int(((path == i) & (n_empty > 0)).sum())
    return pop


# what the CPU test asserts of the crafted map (pooled pixels per class)
CRAFTED_MIN = {"I1": 8, "I2": 8, "I3": 8, "I4": 8, "I6": 8, "B2": 8, "B4": 8, "I6 kmax=5": 8, "I6 kmax=6": 8, "B4 kmax=3": 8, "B4 kmax=4": 8,
               "heavy interior": 8, "heavy border kmax>=7": 8, "heavy border kmax 5..6": 4, "heavy n_empty>0": 4, "heavy n_e<=32": 8,
               "heavy 32<n_e<=64": 8, "heavy n_e>64": 8, "heavy chunk start": 8, "static some empty": 8, "static n_e=0": 8}


# ----------------------------------------------------------------------------------------------------------------------------------------
# label maps
# ----------------------------------------------------------------------------------------------------------------------------------------
NOISE_PATCH = (slice(0, 30), slice(58, 132))        # the pixel-noise patch on the top border (its labels: crafted_noise_labels())


@functools.lru_cache(maxsize=1)
def crafted_map():
    """(seg i32[224][224], S): one deterministic map that puts pooled pixels on every path of the apply launch (CRAFTED_MIN)."""
    rng = np.random.default_rng(2406)
    yy, xx = np.meshgrid(np.arange(ST_IN), np.arange(ST_IN), indexing="ij")
    raw = synth.grid_segments().astype(np.int64)                               # 16-pixel grid: 0 .. 195
    nxt = 1000

    def region(rs, cs, labels):
        nonlocal nxt
        raw[rs, cs] = nxt + labels
        nxt += int(labels.max()) + 1

    # 8 x 16 bricks, every other course shifted by 8
    rs, cs = slice(64, 128), slice(112, 224)
    course = (yy[rs, cs] - 64) // 8
    region(rs, cs, course * 16 + ((xx[rs, cs] - 112 + 8 * (course % 2)) // 16))
    # 5-pixel stripes, vertical then horizontal
    rs, cs = slice(128, 176), slice(0, 56)
    region(rs, cs, (xx[rs, cs] // 5))
    rs, cs = slice(128, 176), slice(56, 112)
    region(rs, cs, ((yy[rs, cs] - 128) // 5))
    # 5 x 7 blocks
    rs, cs = slice(128, 176), slice(112, 224)
    region(rs, cs, ((yy[rs, cs] - 128) // 5) * 16 + (xx[rs, cs] - 112) // 7)
    # 3 x 4 blocks in columns 0 .. 5: border pixels with 4 .. 6 entries under one conv pixel (no <6, true>: the streaming launch)
    rs, cs = slice(34, 126), slice(0, 6)
    region(rs, cs, ((yy[rs, cs] - 34) // 4) * 2 + xx[rs, cs] // 3)
    # 4-pixel vertical stripes on the top border (2 .. 3 entries under a border conv pixel), 4 x 8 blocks on the left border (2 or 4)
    rs, cs = slice(0, 10), slice(150, 210)
    region(rs, cs, (xx[rs, cs] - 150) // 4)
    rs, cs = slice(176, 224), slice(0, 8)
    region(rs, cs, ((yy[rs, cs] - 176) // 8) * 2 + xx[rs, cs] // 4)
    # pixel noise on the top border and in the bottom right corner
    rs, cs = NOISE_PATCH
    region(rs, cs, rng.integers(0, 160, size=(30, 74)))
    rs, cs = slice(196, 224), slice(196, 224)
    region(rs, cs, rng.integers(0, 90, size=(28, 28)))
    seg = np.unique(raw, return_inverse=True)[1].reshape(ST_IN, ST_IN).astype(np.int64)
    S = int(seg.max()) + 1
    # labels outside [0, S) on both sides: a 14 x 14 hole in the noise patch (heavy pixels over empty conv pixels), a 30 x 50 block in the grid
    # (static pixels with some and with all conv pixels empty), single pixels
    seg[8:22, 84:98] = -1
    seg[180:210, 120:170] = S
    seg[181:209:3, 121:169:5] = 1 << 30
    seg[140:162, 150:182] = S + 5                # ... in the 5 x 7 blocks, on the stripes of the top border, on the blocks of the left one
    seg[0:12, 168:186] = -7
    seg[196:212, 0:10] = S
    seg[90, 60] = -(1 << 31)
    seg[91, 61] = (1 << 31) - 1
    seg = seg.astype(np.int32)
    assert (seg == S - 1).any() and (seg == 0).any()
    return seg, S


def crafted_noise_labels():
    seg, S = crafted_map()
    l = np.unique(seg[NOISE_PATCH])
    return l[(l >= 0) & (l < S)]


def tiny_map_s1():
    """S = 1: label 0 and labels outside (the first index of the bit planes)."""
    seg = np.zeros((ST_IN, ST_IN), dtype=np.int32)
    seg[100:140, 30:90] = 1
    seg[0:9, 0:9] = -1
    return seg, 1


def map_s4096():
    """S = 4096 (the largest the table takes), labels 0 and 4095 present: 4 x 4 blocks cycling through 0 .. 4095 with a noise patch."""
    idx = np.arange(ST_IN) // 4
    seg = ((idx[:, None] * 56 + idx[None, :]) % 4096).astype(np.int32)
    seg[60:80, 60:80] = np.random.default_rng(77).integers(0, 4096, size=(20, 20))
    seg[0:4, 0:4] = 4095
    seg[220:224, 220:224] = 0
    seg[30:34, 30:38] = 4096
    assert (seg == 0).any() and (seg == 4095).any()
    return seg, 4096


def existing_maps(golden_dir):
    """The five label maps of tests/test_gpu_stem_table.py (its _segments kinds and the out-of-range grid), for the gap table."""
    import os
    felz = np.load(os.path.join(golden_dir, "segments_blobs.npz"))["segments"][0]
    felz = np.unique(felz, return_inverse=True)[1].reshape(ST_IN, ST_IN).astype(np.int32)
    oor = synth.grid_segments().copy()
    oor[40:90, 100:160] = 500
    oor[0:5, 0:5] = -3
    return [("grid", synth.grid_segments(), 196), ("felzenszwalb", felz, int(felz.max()) + 1),
            ("stripes", (np.arange(ST_IN)[None, :] // 2 + 0 * np.arange(ST_IN)[:, None]).astype(np.int32), 112),
            ("noise", np.random.default_rng(5).integers(0, 2000, size=(ST_IN, ST_IN)).astype(np.int32), 2000), ("grid, out of range", oor, 196)]


# ----------------------------------------------------------------------------------------------------------------------------------------
# images, weights, mask rows
# ----------------------------------------------------------------------------------------------------------------------------------------
def image_u8():
    img = synth.make_images(1, seed=2407, kind="noise")[0].copy()
    img[0, 0], img[0, 1], img[223, 223] = 0, 255, (0, 255, 0)
    img[100:110, 100:110] = 0
    img[110:120, 100:110] = 255
    return img


def image_f32():
    """f32[3][224][224] with exact zeros and both signs (a caller's own normalisation: the table takes it as it is)."""
    g = torch.Generator().manual_seed(2408)
    x = (torch.randn(3, ST_IN, ST_IN, generator=g) * 1.2).numpy().astype(f32)
    x[:, 50:70, 40:90] = 0.0
    x[1, ::7, ::5] = 0.0
    x[0, 0, 0], x[2, 223, 223] = -2.5, 2.5
    return x


EDIT_NEG = (3, 17, 42)                     # bn1.weight negated
EDIT_SHIFT = (3, 9, 17, 26, 42, 55)        # bn1.bias raised: a large positive shift


def weight_sets():
    """{'synthetic', 'trained-like', 'edited'}: resnet18 state dicts (only conv1 / bn1 matter to the stem)."""
    from oracle import trained_like
    syn = synth.make_state_dict("resnet18")
    ed = type(syn)(syn)
    g, b = ed["bn1.weight"].clone(), ed["bn1.bias"].clone()
    for c in EDIT_NEG:
        g[c] = -g[c]
    for c in EDIT_SHIFT:
        b[c] = b[c] + 1.5
    ed["bn1.weight"], ed["bn1.bias"] = g, b
    return {"synthetic": syn, "trained-like": trained_like.make_trained_like_state_dict("resnet18"), "edited": ed}


def mask_rows(S, noise_labels=None, seed=2409):
    """u8[M][S]: all kept, all removed, single superpixels (first, last, one in the middle), Bernoulli rows at 0.1 / 0.5 / 0.9, and rows that
    differ from the row before in one superpixel of the noise patch."""
    rng = np.random.default_rng(seed)
    rows = [np.ones(S, np.uint8), np.zeros(S, np.uint8)]
    for s in sorted({0, S // 2, S - 1}):
        r = np.zeros(S, np.uint8)
        r[s] = 1
        rows.append(r)
    for p in (0.1, 0.5, 0.9):
        for _ in range(3 if S > 1 else 1):
            rows.append((rng.random(S) < p).astype(np.uint8))
    if noise_labels is not None and len(noise_labels):
        for _ in range(6):
            r = rows[-1].copy()
            r[rng.choice(noise_labels)] ^= 1
            rows.append(r)
    return np.stack(rows)


# ----------------------------------------------------------------------------------------------------------------------------------------
# exact fp32 arithmetic in numpy
# ----------------------------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c) of fp32 arrays, exactly: the product is exact in fp64 and the fp64 sum s is within half an fp64 ulp of a * b + c, so
    rounding s to fp32 differs from rounding a * b + c only where s lies on an fp32 midpoint and the fp64 add was inexact -- there the
    two-sum error of the add says on which side of the midpoint a * b + c is."""
    p = a.astype(f64) * b.astype(f64)
    c = np.broadcast_to(c.astype(f64), p.shape)
    s = p + c
    r = s.astype(f32)
    mid = (s.view(np.int64) & 0x1FFFFFFF) == 0x10000000                        # normal range: the 29 bits fp32 drops are 1000...0
    small = np.abs(s) < 2.0 ** -126                                            # subnormal results: looked at one by one
    cand = np.nonzero(mid | (small & (s != 0)))
    if cand[0].size:
        pc, cc, sc, rc = p[cand], c[cand], s[cand], r[cand]
        bb = sc - pc
        err = (pc - (sc - bb)) + (cc - bb)                                     # two-sum: pc + cc = sc + err exactly
        d = sc - rc.astype(f64)
        other = np.nextafter(rc, np.where(d > 0, f32(np.inf), f32(-np.inf)).astype(f32))
        tie = (d != 0) & (np.abs(d) == np.abs(other.astype(f64) - sc))
        flip = tie & (err != 0) & (np.sign(err) == np.sign(d))
        r[cand] = np.where(flip, other, rc)
    return r


def split_f32(v):
    """split_f32 of csrc/mpx_conv.h: hi = (half) v, lo = (half) (v - (float) hi), as uint16 bit patterns."""
    hi = v.astype(np.float16)
    lo = (v - hi.astype(f32)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def normalise_k0(img):
    """[224 * 224][3] fp32: K0's arithmetic for a u8 HWC image (each step rounded in fp32), an f32 CHW image as it is."""
    if img.dtype == np.uint8:
        t = img.reshape(-1, 3).astype(f32) / f32(255.0)
        return (t - np.asarray(MEAN, dtype=f32)) / np.asarray(STD, dtype=f32)
    return np.ascontiguousarray(img.reshape(3, -1).T).astype(f32)


def bn_scale_shift(sd):
    """s, t as mpx_set_conv_weights computes them: in double, rounded to fp32 once; and the same in fp64."""
    g, b, m, v = (sd["bn1." + k].numpy().astype(f64) for k in ("weight", "bias", "running_mean", "running_var"))
    s = g / np.sqrt(v + float(f32(BN_EPS)))
    t = b - m * s
    return s.astype(f32), t.astype(f32), s, t


def entry_vectors(tb, img, sd):
    """vec[e][64]: stemtab_fill_kernel's fp32 FMA chain of every table entry (taps in raster order, channels 0, 1, 2)."""
    x = normalise_k0(img)
    w = sd["conv1.weight"].numpy().astype(f32)                                 # [64][3][7][7]
    vec = np.zeros((int(tb.off[-1]), ST_C), dtype=f32)
    for t in range(ST_TAPS):
        e = tb.tap_ent[:, t]
        sel = e >= 0
        es, ps = e[sel], tb.tap_pix[sel, t]
        for c in range(3):
            vec[es] = fma32(w[:, c, t // 7, t % 7][None, :], x[ps, c][:, None], vec[es])
    return vec


def emulate(tb, vec, sd, onoff, reverse=False):
    """(hi, lo) u16[M][56][56][64]: the bits mpx_stem_table_apply stores for the mask rows onoff u8[M][S].  reverse: a conv pixel's entries
    added last to first (what the kernel does NOT do; the CPU test measures what that changes)."""
    s32, t32, _s, _t = bn_scale_shift(sd)
    M = onoff.shape[0]
    keep = onoff[:, tb.lab] != 0                                              # [M][E]
    v = np.zeros((M, ST_NPIX, ST_C), dtype=f32)
    ks = range(int(tb.cnt.max()))
    for k in (reversed(ks) if reverse else ks):                                # v = v + R over the kept entries, in entry order
        e = np.nonzero(tb.ent_k == k)[0]
        q = tb.ent_q[e]
        v[:, q] = v[:, q] + np.where(keep[:, e, None], vec[e][None], f32(0))
    y = np.empty((M, ST_CONV + 1, ST_CONV + 1, ST_C), dtype=f32)              # row / column 0 = conv row / column -1: outside the map
    y[:, 0], y[:, :, 0] = -np.inf, -np.inf
    for m in range(M):
        z = fma32(v[m], s32[None, :], t32[None, :])
        y[m, 1:, 1:] = (np.maximum(z, f32(0)) + f32(0)).reshape(ST_CONV, ST_CONV, ST_C)      # fmaxf(z, 0.f): -0 never comes out of v_max
    best = y[:, 0:111:2, 0:111:2]
    for r in range(3):
        for c in range(3):
            if r or c:
                best = np.maximum(best, y[:, r:r + 111:2, c:c + 111:2])
    hi, lo = split_f32(np.ascontiguousarray(best))
    return hi, np.where(lo == 0x8000, np.uint16(0), lo)                      # stem_split_packed: an underflowed negative residual is stored as +0


# ----------------------------------------------------------------------------------------------------------------------------------------
# fp64 reference and bound
# ----------------------------------------------------------------------------------------------------------------------------------------
def reference(tb, seg, S, img, sd, onoff):
    """fp64 normalise -> mask -> conv1 -> bn1 -> relu -> maxpool (test_gpu_stem_table._oracle_pooled) with the per-element bound.
    Returns dict: want, tol [M][56][56][64]; y, tolq [M][112][112][64] (post-ReLU value and bound per conv pixel); zero [M][56][56][64]
    (every valid conv pixel's pre-activation below -tol_q: the output is exactly +0)."""
    x = torch.from_numpy(normalise_k0(img).T.reshape(3, ST_IN, ST_IN).copy()).double()
    segl = np.asarray(seg, dtype=np.int64)
    inr = (segl >= 0) & (segl < S)
    M = onoff.shape[0]
    keep = np.where(inr[None], onoff[:, np.where(inr, segl, 0)] != 0, False).astype(f64)          # [M][224][224]
    keep_t = torch.from_numpy(keep)
    w = sd["conv1.weight"].double()
    _s32, _t32, s, t = bn_scale_shift(sd)
    s_t, t_t = torch.from_numpy(s).view(1, -1, 1, 1), torch.from_numpy(t).view(1, -1, 1, 1)
    xb = x[None] * keep_t[:, None]
    z = F.conv2d(xb, w, None, 2, 3) * s_t + t_t
    mag = F.conv2d(xb.abs(), w.abs(), None, 2, 3) * s_t.abs() + t_t.abs()
    taps = F.conv2d(keep_t[:, None], torch.ones(1, 1, 7, 7, dtype=torch.float64), None, 2, 3)     # [M][1][112][112]
    kept_e = np.zeros((M, ST_NPIX))
    ke = (onoff[:, tb.lab] != 0).astype(f64)
    for m in range(M):
        kept_e[m] = np.bincount(tb.ent_q, weights=ke[m], minlength=ST_NPIX)
    n_q = 3.0 * taps + torch.from_numpy(kept_e).view(M, 1, ST_CONV, ST_CONV) + 1.0
    tolq = 1.01 * n_q * U * mag
    want = F.max_pool2d(F.relu(z), 3, 2, 1)
    tol = F.max_pool2d(tolq, 3, 2, 1) + 2.0 ** -22 * want.abs() + 2.0 ** -24
    zero = F.max_pool2d(z + tolq, 3, 2, 1) < 0                                  # max over the valid conv pixels (the padding is -inf)
    nhwc = lambda a: a.permute(0, 2, 3, 1).contiguous().numpy()
    return {"want": nhwc(want), "tol": nhwc(tol), "zero": nhwc(zero), "y": nhwc(F.relu(z)), "tolq": nhwc(tolq), "t": t}


def precondition_counts(tb, cl, ref):
    """On the reference alone.  border: (row, border pooled pixel, channel) elements where every valid conv pixel's value lies below
    relu(shift) by more than the bound -- a border pool that admits an absent conv pixel (which computes relu(shift)) shows there.
    empty_is_max / empty_is_not: elements of heavy pooled pixels over an empty conv pixel where relu(shift), the empty pixel's value, exceeds
    every other conv pixel's by more than the bound / is exceeded by one of them by more than the bound."""
    rt = np.maximum(ref["t"], 0.0)[None, None, None, :]
    border = ~cl["interior"]
    n_border = int(((rt - ref["want"] > ref["tol"]) & border[None, :, :, None]).sum())
    y_ne = np.where((tb.cnt > 0).reshape(1, ST_CONV, ST_CONV, 1), ref["y"], -np.inf)
    w_ne = F.max_pool2d(torch.from_numpy(y_ne).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).numpy()
    he = ((cl["path"] == PATHS.index("heavy")) & (cl["n_empty"] > 0))[None, :, :, None]
    return {"border": n_border, "empty_is_max": int(((rt - w_ne > ref["tol"]) & he).sum()), "empty_is_not": int(((w_ne - rt > ref["tol"]) & he).sum())}


def planes_value(hi, lo):
    """fp64 value of a pair of u16 planes."""
    return hi.view(np.float16).astype(f64) + lo.view(np.float16).astype(f64)


def per_path_ratios(cl, got, ref):
    """{path: worst |got - want| / tol over the pooled pixels on that path}."""
    r = (np.abs(got - ref["want"]) / ref["tol"]).max(axis=(0, 3))
    return {name: float(r[cl["path"] == i].max()) for i, name in enumerate(PATHS) if (cl["path"] == i).any()}


def mismatch_report(cl, got_hi, got_lo, want_hi, want_lo):
    """'' when both planes agree bit for bit; else per path class the number of differing elements and the first of them."""
    bad = (got_hi != want_hi) | (got_lo != want_lo)
    if not bad.any():
        return ""
    lines = []
    for i, name in enumerate(PATHS):
        sel = bad & (cl["path"] == i)[None, :, :, None]
        if sel.any():
            m, py, px, c = (int(a[0]) for a in np.nonzero(sel))
            lines.append("%s: %d elements differ; first row %d pooled (%d, %d) channel %d: got hi %04x lo %04x, want hi %04x lo %04x "
                         "(kmax %d, n_e %d, n_empty %d)" % (name, int(sel.sum()), m, py, px, c, got_hi[m, py, px, c], got_lo[m, py, px, c],
                                                            want_hi[m, py, px, c], want_lo[m, py, px, c], cl["kmax"][py, px],
                                                            cl["n_e"][py, px], cl["n_empty"][py, px]))
    return "\n".join(lines)
