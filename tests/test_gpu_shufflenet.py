"""The ShuffleNetV2 family on the MI355X (pytest -m gpu), through the C-ABI as tests/test_gpu_mobilenet.py does: the channel shuffle bit for
bit against the index formula, the linear depthwise 3x3 + BN kernel against fp64 with a bound derived from its roundings, every distinct
conv shape -- the input-slice, output-slice and two-half-map layers among them -- on every tile it accepts against an fp64 conv +
BatchNorm of the same split inputs, topology and defaults of all four widths, x1_0 and x0_5 end to end against the batch-1 fp32 CPU loop
and the fp64 restatement (tests/shufflenet_ref.py), position independence of a mask row, the reference-named API, the profile and the
error paths.

Bounds.
  Shuffle: pure data movement, torch.equal on the int16 views of both planes.
  Linear depthwise, per element: |err| <= 2^-19 (|s| sum|w_i x_i| + |t|) + 2^-24, the bound of tests/test_gpu_mobilenet.py restated without
  clamps.  An unfused nine-tap sum makes up to 9 products + 8 adds, the BatchNorm two more roundings, each 2^-24 relative to a partial
  result that sum|w_i x_i| (times |s|, plus |t|) bounds, and the re-split 2^-22: 23 x 2^-24 < 2^-19.  Outputs below -tol and above 6 + tol
  must exist and come back UNCLIPPED (within the same bound of the fp64 value): that is what separates this kernel from MobileNetV2's.
  Per conv layer: 4e-6 sqrt(max(K, 4608) / 4608) of max(|want|, 1), the project's per-layer bound (every K here is <= 2048: 4e-6).
  End to end: the fp32 batch-1 CPU loop is the yardstick.  With d = max |fp32 loop - fp64| over the scored rows, the bound on |engine - fp64|
  and |engine - fp32 loop| is the project's 2e-5 when 4 d < 2e-5, else 4 d rounded up to one digit and never above 1e-4 (the rule of
  tests/test_gpu_mobilenet.py).  Measured over the 28 rows of shufflenet_ref.E2E_CASES by this test's own fp32 loop on the host of an
  MI355X: d = 5.7e-07 (shufflenet_v2_x1_0), 6.1e-07 (shufflenet_v2_x0_5); 4 d < 2e-05, so the bound is 2e-05 for both.  The same argmax on EVERY row (tests/test_shufflenet_cpu.py
  asserts a top-two fp64 margin >= 1e-3 on exactly these rows).  The test prints every figure before it asserts."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import shufflenet_ref as ref
from gpu_common import accepted_tiles, dev, FALLBACK, GENERIC, merge, pitch_of, ptr, SCORE_TOL, split  # noqa: F401  (dev is a fixture)
from net_harness import assert_layer_close, check_api, check_end_to_end, check_position_independence, conv_tile, e2e_rows, Reference, stage_stem_input
from network_interpretation_imagenet_amd import _lib, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine
from oracle import scorer

pytestmark = pytest.mark.gpu

EPS = 1e-5
X10, X05 = "shufflenet_v2_x1_0", "shufflenet_v2_x0_5"


@pytest.fixture(scope="module")
def sds():
    return {a: synth.make_state_dict(a) for a in ref.ARCHS}


@pytest.fixture(scope="module")
def small_engines(mpx_lib, dev, sds):
    """A small workspace per width, for everything that hands the kernels device pointers of its own."""
    es = {a: MaskedForwardEngine(a, max_batch=4, device=0).load_state_dict(sds[a]) for a in ref.ARCHS}
    yield es
    for e in es.values():
        e.close()


@pytest.fixture(scope="module")
def engines(mpx_lib, dev, sds):
    es = {a: MaskedForwardEngine(a, device=0).load_state_dict(sds[a]) for a in ref.E2E_ARCHS}        # the default max_batch
    yield es
    for e in es.values():
        e.close()


def _ints(eng, fn, k, n):
    v = [C.c_int() for _ in range(n)]
    assert fn(eng._h, k, *[C.byref(x) for x in v]) == 0
    return [int(x.value) for x in v]


# ------------------------------------------------------------------------------------------------
# channel shuffle, bit for bit
# ------------------------------------------------------------------------------------------------
def _rand_planes(shape, gen, dev):
    """Two planes of random fp16 bit patterns (any pair of bit patterns is a value to a kernel that only moves data)."""
    bits = torch.randint(-32768, 32768, shape, generator=gen, dtype=torch.int32).to(torch.int16)
    bits2 = torch.randint(-32768, 32768, shape, generator=gen, dtype=torch.int32).to(torch.int16)
    return bits.view(torch.float16).to(dev), bits2.view(torch.float16).to(dev)


def _shuffle_case(eng, dev, bf, hp, batch, hw, mode, seed):
    """mode "sep": a and b are planes of pitch hp of their own; "mixed": a is the first half of a two-half map (pitch 2 hp) whose other half
    is garbage, b has pitch hp (a stride-1 block); "map": a and b are the two halves of ONE map of pitch 2 hp (a stride-2 block).  Every
    pad channel of the sources is NaN; a NaN sentinel sits behind y."""
    gen = torch.Generator().manual_seed(seed)
    npix = batch * hw * hw
    nan = float("nan")
    if mode == "sep":
        ah, al = _rand_planes((npix, hp), gen, dev)
        bh, bl = _rand_planes((npix, hp), gen, dev)
        for t in (ah, al, bh, bl):
            t[:, bf:] = nan
        a_ptr, b_ptr, a_pitch, b_pitch = (ah, al, 0), (bh, bl, 0), hp, hp
        a_real, b_real = (ah[:, :bf], al[:, :bf]), (bh[:, :bf], bl[:, :bf])
    else:
        mh, ml = _rand_planes((npix, 2 * hp), gen, dev)             # the second half of a "mixed" map: garbage, NaN among it
        for t in (mh, ml):
            t[:, bf:hp] = nan
            t[:, hp + bf:] = nan
        a_real = (mh[:, :bf], ml[:, :bf])
        if mode == "mixed":
            mh[:, hp::3] = nan
            bh, bl = _rand_planes((npix, hp), gen, dev)
            for t in (bh, bl):
                t[:, bf:] = nan
            b_ptr, b_pitch, b_real = (bh, bl, 0), hp, (bh[:, :bf], bl[:, :bf])
        else:
            b_ptr, b_pitch, b_real = (mh, ml, hp), 2 * hp, (mh[:, hp:hp + bf], ml[:, hp:hp + bf])
        a_ptr, a_pitch = (mh, ml, 0), 2 * hp
    n_out = npix * 2 * hp
    guard = 64
    yh = torch.full((n_out + guard,), nan, dtype=torch.float16, device=dev)
    yl = torch.full_like(yh, nan)
    rc = eng._lib.mpx_shuffle2_concat(eng._h, ptr(a_ptr[0], a_ptr[2]), ptr(a_ptr[1], a_ptr[2]), a_pitch, ptr(b_ptr[0], b_ptr[2]), ptr(b_ptr[1], b_ptr[2]),
                                      b_pitch, ptr(yh), ptr(yl), batch, hw, bf, hp, eng._stream())
    _lib.check(eng._h, rc, "mpx_shuffle2_concat")
    torch.cuda.synchronize()
    assert torch.isnan(yh[n_out:]).all() and torch.isnan(yl[n_out:]).all()          # the sentinel behind y is intact
    which, idx = ref.shuffle_source(bf, hp)
    which_t, idx_t = torch.from_numpy(which).to(dev), torch.from_numpy(idx).to(dev)
    for got, a, b in ((yh[:n_out].view(npix, 2 * hp), a_real[0], b_real[0]), (yl[:n_out].view(npix, 2 * hp), a_real[1], b_real[1])):
        want = torch.where((which_t == 1)[None, :], b.view(torch.int16)[:, idx_t], a.view(torch.int16)[:, idx_t])
        want = torch.where((which_t < 0)[None, :], torch.zeros_like(want), want)
        assert torch.equal(got.view(torch.int16), want), (bf, hp, batch, hw, mode)
        pads = got.view(torch.int16)[:, which_t < 0]
        assert pads.numel() == npix * 2 * (hp - bf) and (pads == 0).all()            # every output pad channel: zero bits


SHUFFLE_HALVES = ((24, 32), (58, 64), (116, 128), (96, 96), (122, 128))


@pytest.mark.parametrize("bf,hp", SHUFFLE_HALVES)
@pytest.mark.parametrize("batch,hw", [(1, 1), (3, 7)])
@pytest.mark.parametrize("mode", ["sep", "mixed", "map"])
def test_shuffle_is_bit_exact(small_engines, dev, bf, hp, batch, hw, mode):
    _shuffle_case(small_engines[X10], dev, bf, hp, batch, hw, mode, seed=bf * 100 + hw + len(mode))


@pytest.mark.parametrize("bf,hp", [(58, 64), (96, 96)])
def test_shuffle_past_a_round_of_the_capped_grid(small_engines, dev, bf, hp):
    """The grid is capped at 8 blocks of 256 units per CU; 12 x 56 x 56 pixels x (2 hp / 8) units is more than one round of it (602112 and
    903168 units against 524288 on 256 CUs), on both load widths."""
    eng = small_engines[X10]
    assert 12 * 56 * 56 * (2 * hp // 8) > eng.num_cus * 8 * 256
    _shuffle_case(eng, dev, bf, hp, 12, 56, "mixed", seed=bf)


# ------------------------------------------------------------------------------------------------
# linear depthwise 3x3 + BN
# ------------------------------------------------------------------------------------------------
def _dw_inputs(c, pitch, hin, batch, seed, corner, dev, phys=None):
    """Planes with values of both signs well beyond [0, 6], exact zeros and small magnitudes; weights [c][3][3] (all the weight on one corner
    tap when `corner` is (ky, kx)); BatchNorm with both signs of gamma.  `phys`: the physical channel of every logical one (None: the first
    c).  Every other channel of the pitch carries finite garbage on the input side: its weights, scale and shift are zero."""
    g = torch.Generator().manual_seed(seed)
    phys = torch.arange(c) if phys is None else torch.as_tensor(phys)
    x = torch.randn(batch, hin, hin, pitch, generator=g) * 3.0
    x[torch.rand(x.shape, generator=g) < 0.15] = 0.0
    x[torch.rand(x.shape, generator=g) < 0.10] *= 3.0
    x[..., phys[: max(1, c // 4)]] *= 1e-3                                   # lo in fp16's subnormals
    w = torch.randn(c, 3, 3, generator=g) * (2.0 / 9) ** 0.5
    if corner is not None:
        w = torch.zeros(c, 3, 3)
        w[:, corner[0], corner[1]] = torch.randn(c, generator=g) + 2.0
    gamma = torch.empty(c).uniform_(0.5, 2.5, generator=g) * torch.where(torch.rand(c, generator=g) < 0.2, -1.0, 1.0)
    beta = torch.randn(c, generator=g) * 0.5
    mean = torch.randn(c, generator=g) * 0.3
    var = torch.empty(c).uniform_(0.3, 2.0, generator=g)
    s64 = gamma.double() / torch.sqrt(var.double() + EPS)
    t64 = beta.double() - mean.double() * s64
    wt = torch.zeros(9, pitch)
    wt[:, phys] = w.reshape(c, 9).t()
    sc = torch.zeros(pitch)
    sh = torch.zeros(pitch)
    sc[phys] = s64.float()
    sh[phys] = t64.float()
    return x.to(dev), wt.contiguous().to(dev), sc.to(dev), sh.to(dev), phys.to(dev)


def _dw_check(eng, xh, xl, wt, sc, sh, phys, pitch, hin, stride, what, images=None):
    """Runs mpx_dwconv3x3_bn on the planes and checks `images` (all by default) against fp64, WITHOUT clamps.  -> worst err / bound."""
    dev = xh.device
    batch = xh.shape[0]
    c = phys.numel()
    ho = (hin - 1) // stride + 1
    guard = 64
    n_out = batch * ho * ho * pitch
    oh = torch.full((n_out + guard,), float("nan"), dtype=torch.float16, device=dev)
    ol = torch.full_like(oh, float("nan"))
    rc = eng._lib.mpx_dwconv3x3_bn(eng._h, ptr(xh), ptr(xl), ptr(wt), ptr(sc), ptr(sh), ptr(oh), ptr(ol), batch, hin, pitch, stride, eng._stream())
    _lib.check(eng._h, rc, "mpx_dwconv3x3_bn")
    torch.cuda.synchronize()
    assert torch.isnan(oh[n_out:]).all() and torch.isnan(ol[n_out:]).all()              # the neighbours behind the planes are untouched
    yh, yl = oh[:n_out].view(batch, ho, ho, pitch), ol[:n_out].view(batch, ho, ho, pitch)
    pad = torch.ones(pitch, dtype=torch.bool, device=dev)
    pad[phys] = False
    worst, below, above = 0.0, 0, 0
    for n in (range(batch) if images is None else images):
        got = merge(yh[n], yl[n]).double()
        assert not torch.isnan(got).any()
        if pad.any():                                                                   # pad outputs: exact zeros, both planes
            assert (yh[n][..., pad].view(torch.int16) == 0).all() and (yl[n][..., pad].view(torch.int16) == 0).all(), what
        x64 = merge(xh[n][..., phys], xl[n][..., phys]).double().permute(2, 0, 1)[None]
        w64 = wt[:, phys].double().t().reshape(c, 1, 3, 3)
        s64, t64 = sc[phys].double()[None, :, None, None], sh[phys].double()[None, :, None, None]
        acc = F.conv2d(x64, w64, None, stride, 1, 1, c)
        mag = F.conv2d(x64.abs(), w64.abs(), None, stride, 1, 1, c)
        want = (s64 * acc + t64)[0].permute(1, 2, 0)
        tol = (2.0 ** -19 * (s64.abs() * mag + t64.abs()) + 2.0 ** -24)[0].permute(1, 2, 0)
        g = got[..., phys]
        err = (g - want).abs()
        worst = max(worst, (err / tol).max().item())
        lo_m, hi_m = want < -tol, want > 6.0 + tol
        below += int(lo_m.sum())
        above += int(hi_m.sum())
        # unclipped: a negative value comes back negative, a value above 6 above 6, each within its bound of the fp64 value
        assert (g[lo_m] < 0).all() and (g[hi_m] > 6.0).all(), what
        assert (err[lo_m] <= tol[lo_m]).all() and (err[hi_m] <= tol[hi_m]).all(), what
    print("%s: worst err / bound %.3f, %d outputs below -tol, %d above 6 + tol" % (what, worst, below, above))
    assert below > 0 and above > 0, what
    assert worst <= 1.0, (what, worst)
    return worst


DW_CASES = [(c, pitch, hin, stride, batch) for (c, pitch) in ((24, 32), (58, 64), (96, 96)) for hin in (4, 5, 7, 14) for stride in (1, 2)
            for batch in (1, 3)]


@pytest.mark.parametrize("c,pitch,hin,stride,batch", DW_CASES)
def test_linear_depthwise_against_fp64(small_engines, dev, c, pitch, hin, stride, batch):
    x, wt, sc, sh, phys = _dw_inputs(c, pitch, hin, batch, seed=1000 * c + 10 * hin + stride + 7 * batch, corner=None, dev=dev)
    xh, xl = split(x)
    _dw_check(small_engines[X10], xh, xl, wt, sc, sh, phys, pitch, hin, stride,
              "linear depthwise C %d pitch %d %dx%d stride %d batch %d" % (c, pitch, hin, hin, stride, batch))


@pytest.mark.parametrize("c,pitch,hin,stride,batch,corner", [(24, 32, 5, 2, 1, (0, 0)), (24, 32, 4, 2, 3, (2, 2)), (58, 64, 5, 1, 1, (2, 2)),
                                                             (58, 64, 7, 2, 3, (0, 0)), (96, 96, 4, 1, 3, (0, 0)), (96, 96, 14, 2, 1, (2, 2))])
def test_linear_depthwise_single_corner_tap(small_engines, dev, c, pitch, hin, stride, batch, corner):
    """All the weight on the top-left or the bottom-right tap: at 4 -> 2 the bottom-right tap of the last output falls outside the map."""
    x, wt, sc, sh, phys = _dw_inputs(c, pitch, hin, batch, seed=77 * c + hin + stride, corner=corner, dev=dev)
    xh, xl = split(x)
    _dw_check(small_engines[X10], xh, xl, wt, sc, sh, phys, pitch, hin, stride,
              "linear depthwise C %d pitch %d %dx%d stride %d batch %d corner %s" % (c, pitch, hin, hin, stride, batch, corner))


@pytest.mark.parametrize("hin,stride,batch", [(14, 2, 3), (7, 1, 1)])
def test_linear_depthwise_on_a_two_half_pitch(small_engines, dev, hin, stride, batch):
    """2 x 58 channels at pitch 128, the second half at 64 (shufflenet_v2_x1_0's stage3.0.branch1.0 reads such a map): zero weights, scale
    and shift on the gaps [58, 64) and [122, 128), exact zeros out."""
    phys = ref.two_half_index(58, 64)
    x, wt, sc, sh, phys = _dw_inputs(116, 128, hin, batch, seed=hin, corner=None, dev=dev, phys=phys)
    xh, xl = split(x)
    _dw_check(small_engines[X10], xh, xl, wt, sc, sh, phys, 128, hin, stride, "linear depthwise 2 x 58 at 128 %dx%d stride %d" % (hin, hin, stride))


DW_RUN_W = {1: 4, 2: 2}         # output pixels per thread of the run form (csrc/mpx_dw.h, DwRun<K, STRIDE>::W)
DW_GRID_CAP = {1: 8, 2: 2}      # blocks of 256 units per CU the host caps the grid at (launch_dwconv)


def _dw_units(batch, hin, stride, pitch):
    """Units of one launch: a unit is 8 channels of a run of W output pixels of one output row."""
    ho = (hin - 1) // stride + 1
    return batch * ho * -(-ho // DW_RUN_W[stride]) * (pitch // 8)


@pytest.mark.parametrize("stride,batch", [(1, 60), (2, 32)])
def test_linear_depthwise_past_a_round_of_the_capped_grid(small_engines, dev, stride, batch):
    """More units than one round of the capped grid, counted as the launch counts them (runs of W output pixels, not pixels), so that threads
    re-enter the grid-stride loop: 56x56 x 96 at stride 1, batch 60, is 60 x 56 x 14 x 12 = 564480 units against 8 x 256 x 256 = 524288 on 256
    CUs; at stride 2, batch 32, 32 x 28 x 14 x 12 = 150528 against 2 x 256 x 256 = 131072.  The first image, one in the middle and the last --
    the one whose units lie past the first round -- are checked against fp64."""
    eng = small_engines[X10]
    units, round_units = _dw_units(batch, 56, stride, 96), eng.num_cus * DW_GRID_CAP[stride] * 256
    assert round_units < units < 2 * round_units
    first_past = round_units // (units // batch)                   # the image that holds the first unit of the second round
    assert first_past < batch - 1
    x, wt, sc, sh, phys = _dw_inputs(96, 96, 56, batch, seed=5 + stride, corner=None, dev=dev)
    xh, xl = split(x)
    _dw_check(eng, xh, xl, wt, sc, sh, phys, 96, 56, stride, "linear depthwise 96 56x56 stride %d batch %d" % (stride, batch),
              images=(0, first_past, batch - 1))


def test_engine_layer_parameters_of_a_depthwise_layer_on_a_two_half_map(small_engines, dev, sds):
    """The device vectors mpx_load_dwconv made for a layer on a two-half map (stage3.0.branch1.0 of x1_0: 116 channels at pitch 128)."""
    eng = small_engines[X10]
    names = [d.name.decode() for d in eng.dwconvs]
    k = names.index("stage3.0.branch1.0")
    d = eng.dwconvs[k]
    assert (d.channels, d.pitch, d.stride, d.hin, d.clamp_in) == (116, 128, 2, 28, 0)
    assert _ints(eng, eng._lib.mpx_dwconv_layout, k, 3) == [1, 58, 64]
    pw, ps, pt = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert eng._lib.mpx_dwconv_params(eng._h, k, C.byref(pw), C.byref(ps), C.byref(pt)) == 0

    def view(ptr, n):
        class _V:
            __cuda_array_interface__ = {"data": (ptr.value, False), "shape": (n,), "typestr": "<f4", "version": 2}
        return torch.as_tensor(_V(), device=dev).clone().cpu()

    got_w, got_s, got_t = view(pw, 9 * 128).view(9, 128), view(ps, 128), view(pt, 128)
    sd = sds[X10]
    at = torch.from_numpy(ref.two_half_index(58, 64))
    gap = torch.ones(128, dtype=torch.bool)
    gap[at] = False
    assert torch.equal(got_w[:, at], sd["stage3.0.branch1.0.weight"].reshape(116, 9).t()) and (got_w[:, gap] == 0).all()
    s64 = sd["stage3.0.branch1.1.weight"].double() / torch.sqrt(sd["stage3.0.branch1.1.running_var"].double() + EPS)
    assert torch.equal(got_s[at], s64.float())
    assert torch.equal(got_t[at], (sd["stage3.0.branch1.1.bias"].double() - sd["stage3.0.branch1.1.running_mean"].double() * s64).float())
    assert (got_s[gap] == 0).all() and (got_t[gap] == 0).all() and int(gap.sum()) == 12


# ------------------------------------------------------------------------------------------------
# topology and defaults
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ref.ARCHS)
def test_topology_and_defaults(mpx_lib, dev, sds, arch):
    eng = MaskedForwardEngine(arch, max_batch=2, device=0)
    try:
        convs, dws = ref.topology(arch)
        assert len(eng.layers) == 38 and len(eng.dwconvs) == 19 and eng._lib.mpx_num_shuffles(eng._h) == 16
        assert [(d.name.decode(), d.bn_name.decode(), d.cin, d.cout, d.ksize, d.stride, d.pad, d.hin, d.hout, d.relu, d.residual) for d in eng.layers] == convs
        assert [(d.name.decode(), d.bn_name.decode(), d.channels, d.stride, d.hin) for d in eng.dwconvs] == dws
        assert all(d.clamp_in == 0 for d in eng.dwconvs)
        assert eng.flops_per_forward == 2.0 * ref.MACS[arch]
        halves = ref.HALVES[arch]
        in_slices = out_slices = whole_maps = 0
        for i, d in enumerate(eng.layers):
            name = d.name.decode()
            pitch, off, bf, hp = _ints(eng, eng._lib.mpx_conv_in_slice, i, 4)
            ypitch, yoff = _ints(eng, eng._lib.mpx_conv_out_slice, i, 2)
            assert d.cout_pad == -(-max(d.cout, _layout(eng, i)[1][2]) // 128) * 128       # rows up to the stored width, in 128s
            if name in ("conv1.0", "fc"):
                assert (pitch, off, bf, hp) == ((4, 0, 0, 0) if name == "conv1.0" else (d.cin, 0, 0, 0))
                assert d.k_packed == (96 if name == "conv1.0" else d.cin)
                continue
            stage = 2 if name == "conv5.0" else int(name[5]) - 2          # index into halves of the stage whose LAYOUT the layer reads / writes
            if name == "conv5.0":
                assert (pitch, off, bf, hp) == (2 * halves[2][1], 0) + halves[2] and d.k_packed == pitch and (ypitch, yoff) == (d.cout, 0)
                whole_maps += 1
                continue
            sbf, shp = halves[stage]
            block0 = name.split(".")[1] == "0"
            if name.endswith("branch2.0") and not block0:                   # the second half of the stage map, in place
                assert (pitch, off, bf, hp) == (2 * shp, shp, 0, 0) and d.k_packed == shp and (ypitch, yoff) == (shp, 0)
                in_slices += 1
            elif block0 and name.endswith(("branch1.2", "branch2.0")):      # the whole input map of the stage
                if stage == 0:
                    assert (pitch, off, bf, hp) == (32, 0, 0, 0) and d.k_packed == 32
                else:
                    assert (pitch, off, bf, hp) == (2 * halves[stage - 1][1], 0) + halves[stage - 1] and d.k_packed == pitch
                    whole_maps += 1
                if name.endswith("branch1.2"):
                    assert (ypitch, yoff) == (2 * shp, 0)
                    out_slices += 1
                else:
                    assert (ypitch, yoff) == (shp, 0)
            else:                                                           # branch2.5
                assert (pitch, off, bf, hp) == (shp, 0, 0, 0) and d.k_packed == shp
                if block0:
                    assert (ypitch, yoff) == (2 * shp, shp)
                    out_slices += 1
                else:
                    assert (ypitch, yoff) == (shp, 0)
            if (pitch, off) != (d.cin, 0) or ypitch != d.cout:              # slices and padded layers: the generic tiles only
                accepted = set(accepted_tiles(eng, i))
                assert accepted == GENERIC, (name, accepted)
            assert eng._lib.mpx_get_conv_tile(eng._h, i) in GENERIC | {10, 13, 9}
        assert (in_slices, out_slices, whole_maps) == (13, 6, 5)
        for k, d in enumerate(eng.dwconvs):
            linear, bf, hp = _ints(eng, eng._lib.mpx_dwconv_layout, k, 3)
            name = d.name.decode()
            stage = int(name[5]) - 2
            assert linear == 1
            if name.endswith("branch1.0") and stage > 0:
                assert (bf, hp) == halves[stage - 1] and (d.channels, d.pitch) == (2 * bf, 2 * hp)
            else:
                assert (bf, hp) == (0, 0) and d.pitch == pitch_of(d.channels)
        sh = [_ints(eng, eng._lib.mpx_shuffle_info, k, 5) for k in range(16)]
        want_sh = []
        for s, reps in enumerate((4, 8, 4)):
            bf, hp = halves[s]
            side = 28 >> s
            want_sh += [[side, bf, hp, 2 * hp, 2 * hp]] + [[side, bf, hp, 2 * hp, hp]] * (reps - 1)
        assert sh == want_sh
        geo = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        assert eng._lib.mpx_geometry(eng._h, *[C.byref(v) for v in geo]) == 0 and [v.value for v in geo] == [224, 3, 1000, 1000]
        assert eng.stem == "conv" and not eng.has_stem_table and eng._lib.mpx_weights_complete(eng._h) == 0
        assert eng._lib.mpx_num_bottleneck_tails(eng._h) == 0 and eng._lib.mpx_num_norms(eng._h) == 0 and eng._lib.mpx_num_clip_pools(eng._h) == 0
        eng.load_state_dict(sds[arch])
        assert eng._lib.mpx_weights_complete(eng._h) == 1
        # per slot: three 112x112x32 split-fp16 buffers and the NHWC4 staging, whatever the width
        per_slot = 3 * 2 * 112 * 112 * 32 * 2 + 2 * 230 * 230 * 4 * 2
        w = sum(2 * d.cout_pad * d.k_packed * 2 for d in eng.layers)
        assert per_slot * 2 + w < eng.workspace_bytes < per_slot * 2 + w + (16 << 20)
        # a forward of the unmasked picture agrees with the fp32 restatement on the class
        img = synth.make_images(1)[0]
        label, prob = ref.predict(sds[arch], arch, scorer.to_tensor_normalize(img))
        p_label, p_prob = eng.predict(img)
        print("%s: unmasked peak %.4f (engine %.4f)" % (arch, prob.max(), p_prob.max()))
        assert p_label == label and abs(float(p_prob.max()) - float(prob.max())) <= SCORE_TOL
    finally:
        eng.close()


def test_default_max_batch_and_workspace(engines):
    eng = engines[X10]
    assert eng.max_batch == 512
    per_slot = 3 * 2 * 112 * 112 * 32 * 2 + 2 * 230 * 230 * 4 * 2
    w = sum(2 * d.cout_pad * d.k_packed * 2 for d in eng.layers)
    assert per_slot * 512 + w < eng.workspace_bytes < per_slot * 512 + w + (16 << 20)
    print("%s: %.2f MB per slot, workspace %.2f GB at max_batch 512" % (X10, per_slot / 1e6, eng.workspace_bytes / 1e9))


# ------------------------------------------------------------------------------------------------
# per conv layer
# ------------------------------------------------------------------------------------------------
def _ref_layer(sd, d, x64):
    """fp64 conv + BatchNorm + ReLU (fc: + bias) on the device: [B][cout][ho][ho]."""
    name, bn = d.name.decode(), d.bn_name.decode()
    dev = x64.device
    y = F.conv2d(x64, sd[name + ".weight"].double().reshape(d.cout, d.cin, d.ksize, d.ksize).to(dev), None, d.stride, d.pad)
    if bn:
        g, b, m, v = (sd["%s.%s" % (bn, k)].double().to(dev)[None, :, None, None] for k in ("weight", "bias", "running_mean", "running_var"))
        y = (y - m) / torch.sqrt(v + EPS) * g + b
    else:
        y = y + sd[name + ".bias"].double().to(dev)[None, :, None, None]
    return F.relu(y) if d.relu else y


def _layout(eng, i):
    """Where layer i reads and writes: (input pitch, physical input channel of every logical one, channels [lo, hi) it may read), (output
    pitch, offset, stored width)."""
    d = eng.layers[i]
    pitch, off, bf, hp = _ints(eng, eng._lib.mpx_conv_in_slice, i, 4)
    ypitch, yoff = _ints(eng, eng._lib.mpx_conv_out_slice, i, 2)
    kk = d.k_packed // (d.ksize * d.ksize)
    phys = torch.from_numpy(ref.two_half_index(bf, hp)) if hp else off + torch.arange(d.cin)
    sliced = ypitch == 2 * pitch_of(d.cout)             # a stride-2 block's last convs: half of a two-half map, hp channels stored
    return (pitch, phys, off, off + kk), (ypitch, yoff, ypitch // 2 if sliced else ypitch)


def _run_layer(eng, sd, i, batch, seed):
    d = eng.layers[i]
    dev = eng.device
    last = i == len(eng.layers) - 1
    g = torch.Generator().manual_seed(seed)
    nan = float("nan")
    x = torch.randn(batch, d.hin, d.hin, d.cin, generator=g).clamp_min(-0.5) * 1.5
    if i == 0:      # the stem reads the engine's padded NHWC4 staging: write the interior, zero border and 4th channel
        xh, xl = split(x.to(dev))
        stage_stem_input(eng, xh, xl, batch)
        in_h = in_l = None
        (ypitch, yoff, stored) = _layout(eng, i)[1]
    else:
        (pitch, phys, lo, hi), (ypitch, yoff, stored) = _layout(eng, i)
        full = torch.full((batch, d.hin, d.hin, pitch), nan)            # what the layer must never read: NaN (the other half of a stage map)
        full[..., lo:hi] = 0.0                                           # the pads of what it reads: exact zeros
        full[..., phys] = x
        in_h, in_l = split(full.to(dev))
        xh, xl = in_h[..., phys.to(dev)], in_l[..., phys.to(dev)]
    if last:
        out = torch.full((batch, d.cout), nan, dtype=torch.float32, device=dev)
        rc = eng._lib.mpx_conv_bn_act(eng._h, i, ptr(in_h), ptr(in_l), None, None, None, None, ptr(out), batch, eng._stream())
        _lib.check(eng._h, rc, "mpx_conv_bn_act")
        got = out.double().view(batch, 1, 1, d.cout)
    else:
        oh = torch.full((batch, d.hout, d.hout, ypitch), nan, dtype=torch.float16, device=dev)
        ol = torch.full_like(oh, nan)
        rc = eng._lib.mpx_conv_bn_act(eng._h, i, ptr(in_h), ptr(in_l), None, None, ptr(oh), ptr(ol), None, batch, eng._stream())
        _lib.check(eng._h, rc, "mpx_conv_bn_act")
        torch.cuda.synchronize()
        for t in (oh, ol):
            assert (t[..., yoff + d.cout:yoff + stored].view(torch.int16) == 0).all(), d.name       # the pads it stores: exact zeros
            assert torch.isnan(t[..., :yoff]).all() and torch.isnan(t[..., yoff + stored:]).all(), d.name     # the other half: untouched
        got = merge(oh, ol).double()[..., yoff:yoff + d.cout]
    torch.cuda.synchronize()
    x64 = merge(xh, xl).double().permute(0, 3, 1, 2)
    want = _ref_layer(sd, d, x64).permute(0, 2, 3, 1)
    return got, want


def _check(eng, sd, i, batch, tile=-1):
    with conv_tile(eng, i, tile):
        got, want = _run_layer(eng, sd, i, batch, seed=1000 * i + batch)
        ran = eng._lib.mpx_last_conv_kernels(eng._h)
    d = eng.layers[i]
    assert not torch.isnan(got).any(), (d.name, tile)
    return assert_layer_close(d, got, want, tile, batch, ran, "%d->%d k%d h%d K %d " % (d.cin, d.cout, d.ksize, d.hin, d.k_packed))


@pytest.mark.parametrize("arch", ref.ARCHS)
def test_every_distinct_conv_shape_on_every_accepted_tile(small_engines, sds, arch):
    """Every distinct (cin, cout, ksize, hin, where it reads, where it writes) of the network at batch 3 on every tile it accepts: conv1 (3x3
    stride 2 pad 1 on the NHWC4 staging, 24 channels stored at pitch 32), the input-slice layers (a NaN first half proves they never touch
    x1), the output-slice layers (a NaN other half proves they write their own half only, pads as zeros), the layers that read a whole
    two-half map (their weight columns sit at the physical channels), conv5 and fc."""
    eng, sd = small_engines[arch], sds[arch]
    seen, count, in_slices, out_slices, whole = set(), 0, 0, 0, 0
    for i, d in enumerate(eng.layers):
        pitch, off, bf, hp = _ints(eng, eng._lib.mpx_conv_in_slice, i, 4)
        ypitch, yoff = _ints(eng, eng._lib.mpx_conv_out_slice, i, 2)
        key = (d.cin, d.cout, d.ksize, d.hin, pitch, off, bf, hp, ypitch, yoff)
        if key in seen:
            continue
        seen.add(key)
        accepted = accepted_tiles(eng, i)
        default = eng._lib.mpx_get_conv_tile(eng._h, i)
        assert default in accepted and GENERIC <= set(accepted), (d.name, accepted)
        in_slices += off > 0
        out_slices += ypitch == 2 * pitch_of(d.cout)
        whole += hp > 0
        if off > 0 or ypitch == 2 * pitch_of(d.cout) or (hp > bf):
            assert set(accepted) == GENERIC, (d.name, accepted)
        for t in accepted:
            ran = _check(eng, sd, i, 3, tile=t)
            assert ran & ((1 << t) | (1 << FALLBACK.get(t, t))), (d.name, t, ran)
            if t not in FALLBACK:
                assert ran == 1 << t, (d.name, t, ran)
        count += 1
    print("%s: distinct conv shapes checked: %d (input slices %d, output slices %d, whole two-half maps %d)" % (arch, count, in_slices, out_slices, whole))
    assert count >= 18 and in_slices >= 3 and out_slices >= 6 and whole >= 5


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ref.E2E_ARCHS)
def test_end_to_end(engines, sds, golden_dir, arch):
    """Logits lens (tests/logits_lens.py): all 1000 logits of every row against fp64, bound 4 d_L with d_L = the fp32 CPU loop's distance.  Measured on one MI355X: shufflenet_v2_x1_0 d_L 6.14e-06, engine 1.01e-05 (1.65); shufflenet_v2_x0_5 d_L 5.61e-06, engine 9.00e-06 (1.60)."""
    r = Reference(ref, sds[arch], arch)
    check_end_to_end(engines[arch], arch, r, e2e_rows(r, ref.E2E_CASES, golden_dir),
                     "%(arch)s: yardstick distance %(d).3e over the 28 rows -> end-to-end bound %(bound).1e")


def test_a_mask_row_scores_the_same_bits_wherever_it_sits(engines, golden_dir):
    check_position_independence(engines[X10], *ref.e2e_inputs(golden_dir, "felz"), (8, ((1, 0, (0,)), (37, 41, (0, 5, 36)), (700, 44, (3, 511, 512, 699)))))


# ------------------------------------------------------------------------------------------------
# API, profile and errors
# ------------------------------------------------------------------------------------------------
def test_api_on_a_shufflenet_engine(engines, sds, golden_dir):
    check_api(engines[X10], Reference(ref, sds[X10], X10), *ref.e2e_inputs(golden_dir, "felz"), heatmaps=1, table_step=23)


def test_profile_lists_the_depthwise_and_shuffle_launches(engines, dev):
    eng = engines[X10]
    img = torch.from_numpy(synth.make_images(1, kind="noise")[0]).to(dev)
    seg = torch.from_numpy(synth.grid_segments()).to(dev)
    onoff = torch.from_numpy(synth.random_onoff(4, 196)).to(dev)
    labels = torch.zeros(4, dtype=torch.int32, device=dev)
    eng.profile(True)
    eng.stage_masks(img, seg, onoff, 0)
    eng.forward(4, labels)
    eng.profile(False)
    prof = eng.collect_profile()
    assert len(prof["per_dw_ms"]) == len(eng.dwconvs) == 19 and all(ms > 0 for ms in prof["per_dw_ms"])
    assert len(prof["per_shuffle_ms"]) == 16 and all(ms > 0 for ms in prof["per_shuffle_ms"])
    assert prof["per_norm_ms"] == [] and prof["avgpool2_ms"] == 0 and prof["per_clip_pool_ms"] == []
    assert prof["launches"]["pool"] == 19 + 16 + 2          # every depthwise layer, every shuffle, the max pool and the global pool
    assert prof["launches"]["conv"] == len(eng.layers) == 38
    assert prof["launches"]["head"] == 1 and prof["launches"]["mask_apply_normalize"] == 1
    assert sum(prof["launches"][k] for k in ("conv", "pool", "head")) == 76        # launches per forward batch


def test_error_paths(small_engines, mpx_lib, dev, sds):
    eng = small_engines[X10]
    z = torch.zeros(8192, dtype=torch.float16, device=dev)
    f = torch.zeros(2048, dtype=torch.float32, device=dev)
    a, b = ptr(z), ptr(f)
    odd = C.c_void_p(z.data_ptr() + 2)
    sh = eng._lib.mpx_shuffle2_concat
    assert sh(eng._h, a, a, 64, a, a, 64, ptr(z, 4096), ptr(z, 4096), 1, 2, 58, 64, None) == 0
    torch.cuda.synchronize()
    assert sh(eng._h, None, a, 64, a, a, 64, a, a, 1, 2, 58, 64, None) == -1            # null planes
    assert sh(eng._h, a, a, 64, a, a, 64, a, None, 1, 2, 58, 64, None) == -1
    assert sh(eng._h, a, a, 64, a, a, 64, a, a, 0, 2, 58, 64, None) == -1               # B <= 0
    assert sh(eng._h, a, a, 64, a, a, 64, a, a, 1, 0, 58, 64, None) == -1               # map <= 0
    assert sh(eng._h, a, a, 64, a, a, 64, a, a, 1, 2, 57, 64, None) == -1               # odd bf
    assert sh(eng._h, a, a, 64, a, a, 64, a, a, 1, 2, 66, 64, None) == -1               # hp < bf
    assert sh(eng._h, a, a, 64, a, a, 64, a, a, 1, 2, 58, 72, None) == -1               # hp no multiple of 32: a unit would straddle the halves
    assert sh(eng._h, a, a, 56, a, a, 64, a, a, 1, 2, 58, 64, None) == -1               # a pitch below bf
    assert sh(eng._h, a, a, 64, a, a, 56, a, a, 1, 2, 58, 64, None) == -1
    assert sh(eng._h, a, a, 60, a, a, 64, a, a, 1, 2, 58, 64, None) == -1               # a pitch that is no multiple of 8
    assert sh(eng._h, a, a, 64, a, a, 60, a, a, 1, 2, 58, 64, None) == -1
    assert sh(eng._h, odd, a, 64, a, a, 64, a, a, 1, 2, 58, 64, None) == -1             # misaligned planes
    assert sh(eng._h, a, a, 64, a, a, 64, a, odd, 1, 2, 58, 64, None) == -1
    dw = eng._lib.mpx_dwconv3x3_bn
    assert dw(eng._h, a, a, b, b, b, ptr(z, 4096), ptr(z, 4096), 1, 4, 8, 1, None) == 0
    torch.cuda.synchronize()
    assert dw(eng._h, None, a, b, b, b, a, a, 1, 4, 8, 1, None) == -1                   # null planes
    assert dw(eng._h, a, a, None, b, b, a, a, 1, 4, 8, 1, None) == -1                   # null weights
    assert dw(eng._h, a, a, b, b, b, a, a, 0, 4, 8, 1, None) == -1                      # B <= 0
    assert dw(eng._h, a, a, b, b, b, a, a, 1, 0, 8, 1, None) == -1                      # map <= 0
    assert dw(eng._h, a, a, b, b, b, a, a, 1, 4, 12, 1, None) == -1                     # pitch % 8
    assert dw(eng._h, a, a, b, b, b, a, a, 1, 4, 8, 3, None) == -1                      # a stride other than 1 or 2
    assert dw(eng._h, a, a, b, b, b, a, a, 1, 4, 8, 0, None) == -1
    assert dw(eng._h, odd, a, b, b, b, a, a, 1, 4, 8, 1, None) == -1                    # misaligned planes
    i = C.c_int()
    assert eng._lib.mpx_shuffle_info(eng._h, 16, C.byref(i), None, None, None, None) == -1
    assert eng._lib.mpx_dwconv_layout(eng._h, 19, C.byref(i), None, None) == -1
    assert eng._lib.mpx_conv_in_slice(eng._h, 38, C.byref(i), None, None, None) == -1
    # staging goes through K0 only
    with pytest.raises(ValueError):
        MaskedForwardEngine(X10, max_batch=2, device=0, stem="table")
    zi = torch.zeros(224, 224, dtype=torch.int32, device=dev)
    im = torch.zeros(224, 224, 3, dtype=torch.uint8, device=dev)
    on = torch.ones(1, 1, dtype=torch.uint8, device=dev)
    mean = (C.c_float * 3)(*scorer.MEAN)
    std = (C.c_float * 3)(*scorer.STD)
    assert eng._lib.mpx_stem_table_build(eng._h, ptr(im), None, ptr(zi), 1, mean, std, None) == -2
    assert eng._lib.mpx_stem_table_apply(eng._h, ptr(on), 1, 1, 0, None) == -2
    buf = torch.zeros(64, dtype=torch.float16, device=dev)
    assert eng._lib.mpx_stem_conv_maxpool(eng._h, ptr(buf), ptr(buf), 1, None) == -2
    for bad in (9000, 9001, 9011, 9999):
        h = C.c_void_p()
        assert mpx_lib.mpx_create(bad, 2, 0, C.byref(h)) == -1 and not h.value
    # a ResNet engine has no shuffles, and its depthwise list is empty
    r = MaskedForwardEngine("resnet18", max_batch=2, device=0)
    try:
        assert r._lib.mpx_num_shuffles(r._h) == 0 and r.collect_profile()["per_shuffle_ms"] == []
        assert _ints(r, r._lib.mpx_conv_in_slice, 1, 4) == [64, 0, 0, 0]
    finally:
        r.close()
    # a MobileNetV2 depthwise layer is not linear
    m = MaskedForwardEngine("mobilenet_v2", max_batch=2, device=0)
    try:
        assert _ints(m, m._lib.mpx_dwconv_layout, 0, 3) == [0, 0, 0]
    finally:
        m.close()
    # the depthwise layers load with the convs, and a forward without them is refused
    fresh = MaskedForwardEngine(X05, max_batch=2, device=0)
    try:
        fresh.load_state_dict(sds[X05], only=[d.name.decode() for d in fresh.layers])
        assert fresh._lib.mpx_weights_complete(fresh._h) == 0
        fresh.stage_masks(im, zi, on, 0)
        labels = torch.zeros(1, dtype=torch.int32, device=dev)
        score = torch.zeros(1, device=dev)
        pred = torch.zeros(1, dtype=torch.int32, device=dev)
        assert fresh._lib.mpx_forward(fresh._h, ptr(labels), ptr(score), ptr(pred), None, 1, None) == -2
        with pytest.raises((KeyError, ValueError)):
            fresh.load_state_dict(sds[X10])
        fresh.load_state_dict(sds[X05], only=[d.name.decode() for d in fresh.dwconvs])
        assert fresh._lib.mpx_weights_complete(fresh._h) == 1
    finally:
        fresh.close()
