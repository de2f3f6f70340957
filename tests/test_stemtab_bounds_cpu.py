"""CPU side of tests/test_gpu_stem_table_edges.py (no GPU): the conditions on the draws of tests/stemtab_draws.py, its exact emulation
of csrc/mpx_stemtab.h against the fp64 reference within the counted-roundings bound, the fp32 FMA helper against libm's fmaf, and what the
older max norm of tests/test_gpu_stem_table.py cannot see."""
import ctypes
import ctypes.util
import functools

import numpy as np
import pytest

import stemtab_draws as D

CPU_ROWS = 10           # mask rows per case here (the GPU file emulates every row of mask_rows)


@functools.lru_cache(maxsize=None)
def crafted():
    seg, S = D.crafted_map()
    tb = D.build_table(seg, S)
    return seg, S, tb, D.classify(tb)


@functools.lru_cache(maxsize=None)
def weights():
    return D.weight_sets()


@functools.lru_cache(maxsize=None)
def images():
    return {"u8": D.image_u8(), "f32": D.image_f32()}


def crafted_rows():
    seg, S, _tb, _cl = crafted()
    rows = D.mask_rows(S, D.crafted_noise_labels())
    return rows[[0, 1, 2, 4, 5, 8, 11, 14, 15, 16][:CPU_ROWS]]               # kept, removed, singles, one per density, a neighbouring pair


@functools.lru_cache(maxsize=None)
def case(wname, iname):
    seg, S, tb, cl = crafted()
    sd, img, onoff = weights()[wname], images()[iname], crafted_rows()
    vec = D.entry_vectors(tb, img, sd)
    hi, lo = D.emulate(tb, vec, sd, onoff)
    return vec, hi, lo, D.reference(tb, seg, S, img, sd, onoff)


def _print_table(title, pops):
    names = list(pops[0][1])
    print("\n%s\n%-26s" % (title, "class") + "".join("%20s" % n for n, _p in pops))
    for k in names:
        print("%-26s" % k + "".join("%20d" % p[k] for _n, p in pops))


def test_crafted_map_populates_every_path_class():
    seg, S, tb, cl = crafted()
    pop = D.populations(cl)
    _print_table("crafted map, S = %d, %d table entries, up to %d under one conv pixel" % (S, tb.off[-1], tb.cnt.max()), [("crafted", pop)])
    for k, n in D.CRAFTED_MIN.items():
        assert pop[k] >= n, "%s: %d pooled pixels, %d wanted" % (k, pop[k], n)
    assert (seg == S - 1).any() and (seg == 0).any()
    assert (seg == -1).any() and (seg == S).any() and (seg < -1).any() and (seg > 1 << 20).any()       # outside [0, S) on both sides
    assert 600 <= S <= 1500
    assert len(D.crafted_noise_labels()) >= 100
    for fn, s_want in ((D.tiny_map_s1, 1), (D.map_s4096, 4096)):
        sg, s = fn()
        assert s == s_want and (sg == 0).any() and (sg == s - 1).any() and ((sg < 0) | (sg >= s)).any()


def test_path_classes_of_the_older_tests_maps(golden_dir):
    """The gap: which classes the five label maps of tests/test_gpu_stem_table.py reach (pooled pixels per class)."""
    pops = [(name, D.populations(D.classify(D.build_table(seg, S)))) for name, seg, S in D.existing_maps(golden_dir)]
    _print_table("label maps of tests/test_gpu_stem_table.py", pops)
    for name, pop in pops:
        assert pop["heavy n_empty>0"] == 0, name            # the n_empty > 0 initialisation of the streaming launch: run by none
        assert pop["heavy border kmax 5..6"] == 0, name     # the `|| g.interior` half of stem_heavy: run by none
        if not name.startswith("grid"):
            assert sum(pop["%s some empty" % p] for p in D.PATHS[:-1]) == 0, name
    by = dict(pops)
    assert by["grid"]["I3"] == by["grid"]["I6"] == by["stripes"]["I3"] == by["stripes"]["I6"] == by["noise"]["I3"] == by["noise"]["I6"] == 0
    assert by["felzenszwalb"]["I3"] > 0 and by["felzenszwalb"]["I6"] > 0        # <3, .> and <6, .> run on the felzenszwalb fixture alone


def test_fma32_is_fmaf():
    """The emulation's fp32 FMA against libm's fmaf: random operands over many binades, sums that cancel, and products that lie exactly on
    an fp32 midpoint with an addend far below fp64's last bit (where rounding the fp64 sum to fp32 rounds twice), subnormal results."""
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(2410)
    n = 30000
    sets = []
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)).astype(np.float32)
    sets.append((a, b, c))
    sets.append((a, b, (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32)))           # cancellation
    j, k = 2 * rng.integers(0, 1024, n) + 1, 2 * rng.integers(0, 1024, n) + 1                            # (1 + j 2^-12)(1 + k 2^-12): bit 2^-24 set
    scale = 2.0 ** rng.integers(-40, 40, n)
    am, bm = ((1 + j * 2.0 ** -12) * scale).astype(np.float32), (1 + k * 2.0 ** -12).astype(np.float32)
    tiny = (rng.choice([-1.0, 1.0], n) * scale * 2.0 ** -rng.integers(55, 100, n)).astype(np.float32)
    sets.append((am, bm, tiny))
    sets.append((am, -bm, tiny))
    sets.append(((a * np.float32(2.0 ** -70)), (b * np.float32(2.0 ** -62)), (c * np.float32(2.0 ** -140)).astype(np.float32)))   # subnormal results
    ties = 0
    for a, b, c in sets:
        got = D.fma32(a, b, c)
        want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
        ties += int((naive.view(np.uint32) != want.view(np.uint32)).sum())
    print("fma32 == fmaf on %d operand triples; rounding the fp64 sum to fp32 differs from fmaf on %d of them" % (5 * n, ties))
    assert ties >= 1000         # the draws do contain the double-rounding cases


CASES = [(w, i) for w in ("synthetic", "trained-like", "edited") for i in ("u8", "f32")]


@pytest.mark.parametrize("wname,iname", CASES)
def test_emulation_within_the_fp64_bound(wname, iname):
    _seg, _S, _tb, cl = crafted()
    _vec, hi, lo, ref = case(wname, iname)
    got = D.planes_value(hi, lo)
    ratios = D.per_path_ratios(cl, got, ref)
    kept = D.per_path_ratios(cl, got[:1], {k: ref[k][:1] for k in ("want", "tol")})
    print("emulation vs fp64, %s / %s: worst err / tol %.3f; per path %s; the all-kept row alone %s" % (
        wname, iname, max(ratios.values()), " ".join("%s %.3f" % kv for kv in ratios.items()), " ".join("%s %.3f" % kv for kv in kept.items())))
    assert np.isfinite(got).all()
    assert max(ratios.values()) <= 1.0
    assert float(np.abs(got - ref["want"]).max()) <= 1e-6 * float(np.abs(ref["want"]).max())
    assert ref["zero"].sum() > 1000 and not hi[ref["zero"]].any() and not lo[ref["zero"]].any()          # exactly +0 in both planes
    assert not (hi == 0x8000).any() and not (lo == 0x8000).any()
    # the all-removed row: split(relu(t)) everywhere, borders included
    s32, t32, _s, _t = D.bn_scale_shift(weights()[wname])
    h1, l1 = D.split_f32(np.maximum(t32, np.float32(0)))
    l1 = np.where(l1 == 0x8000, np.uint16(0), l1)
    assert (hi[1] == h1).all() and (lo[1] == l1).all()


@pytest.mark.parametrize("which", ["S=1", "S=4096"])
def test_emulation_at_the_ends_of_s(which):
    seg, S = D.tiny_map_s1() if which == "S=1" else D.map_s4096()
    tb = D.build_table(seg, S)
    cl = D.classify(tb)
    sd, img = weights()["synthetic"], images()["u8"]
    onoff = D.mask_rows(S)[:5]
    hi, lo = D.emulate(tb, D.entry_vectors(tb, img, sd), sd, onoff)
    ref = D.reference(tb, seg, S, img, sd, onoff)
    ratios = D.per_path_ratios(cl, D.planes_value(hi, lo), ref)
    print("emulation vs fp64, %s: %s" % (which, " ".join("%s %.3f" % kv for kv in ratios.items())))
    assert max(ratios.values()) <= 1.0


@pytest.mark.parametrize("iname", ["u8", "f32"])
def test_reference_shows_what_a_wrong_pool_would_change(iname):
    """Conditions on the draw, from the fp64 reference alone (edited weights: bn1.weight negated on channels EDIT_NEG, bn1.bias + 1.5 on
    EDIT_SHIFT)."""
    _seg, _S, tb, cl = crafted()
    n = D.precondition_counts(tb, cl, case("edited", iname)[3])
    print("edited / %s: %s" % (iname, n))
    assert n["border"] >= 200 and n["empty_is_max"] >= 50 and n["empty_is_not"] >= 50


def test_what_the_max_norm_sees_and_what_it_does_not():
    """Two changes to the emulation, measured against the fp64 reference on the crafted map (synthetic weights, u8 image, the CPU_ROWS rows).
    (a) stem_apply_fast<6, false> summing five slots: the sixth entry of every conv pixel under an I6 pooled pixel is left out.  19657 elements
    leave their bound (by up to 1.4e6 x) -- and the max norm of the tensor is 0.29, not under 1e-6: where the path runs and the entry is kept,
    the pool does not hide a missing entry from the max norm (the same change on the older test's felzenszwalb draw: 3424 elements, max
    norm 0.19).  What the older test lacked there is the path, not the norm: 17 of its pooled pixels have a sixth entry, none of them on
    another weight set or image.
    (b) a conv pixel's entries added last to first (rounding only): no element leaves its bound and the max norm stays at 4e-7 of 1e-6, while
    1.2e5 elements change their bits.  Only the comparison with the emulation sees a change of this kind."""
    seg, S, tb, cl = crafted()
    sd, onoff = weights()["synthetic"], crafted_rows()
    vec, hi, lo, ref = case("synthetic", "u8")
    scale = float(np.abs(ref["want"]).max())
    vec5 = vec.copy()
    vec5[tb.off[:-1][tb.cnt == 6] + 5] = 0.0                                   # adding +0 changes no sum: the entry is dropped
    hi5, lo5 = D.emulate(tb, vec5, sd, onoff)
    i6 = (cl["path"] == D.PATHS.index("I6"))[None, :, :, None]
    got = np.where(i6, D.planes_value(hi5, lo5), D.planes_value(hi, lo))
    err = np.abs(got - ref["want"])
    out = err > ref["tol"]
    print("(a) sixth entry of the I6 pixels dropped: %d elements outside their bound (worst err / tol %.3g), max norm of the tensor %.2e" % (
        int(out.sum()), float((err / ref["tol"]).max()), float(err.max()) / scale))
    print("    per row (elements outside their bound, max norm): " + " ".join(
        "%d:(%d, %.1e)" % (m, int(out[m].sum()), float(err[m].max()) / scale) for m in range(onoff.shape[0])))
    assert out.sum() > 1000 and not out[~np.broadcast_to(i6, out.shape)].any()
    hir, lor = D.emulate(tb, vec, sd, onoff, reverse=True)
    errr = np.abs(D.planes_value(hir, lor) - ref["want"])
    changed = int(((hir != hi) | (lor != lo)).sum())
    print("(b) entries added last to first: %d elements change their bits, %d outside their bound (worst err / tol %.3f), max norm %.2e" % (
        changed, int((errr > ref["tol"]).sum()), float((errr / ref["tol"]).max()), float(errr.max()) / scale))
    assert changed > 1000 and not (errr > ref["tol"]).any() and float(errr.max()) <= 1e-6 * scale
