"""SqueezeNet 1.1 on the MI355X (pytest -m gpu), through the C-ABI as tests/test_gpu_mobilenet.py does: the topology, where every layer
writes (mpx_conv_out_slice) and its default tile, every distinct conv shape on every tile it accepts against an fp64 conv + bias + ReLU of
the same split inputs, the SLICE form of the generic kernel against sentinel-filled concatenated planes, the average pool that writes the
logits against fp64, the whole network against the batch-1 fp32 CPU loop and the fp64 restatement (tests/squeezenet_ref.py), position
independence of a mask row, the reference-named API and the error paths.

Bounds.
  Per conv layer: 4e-6 sqrt(max(K, 4608) / 4608) of max(|want|, 1), the project's per-layer bound (every K here is <= 576: 4e-6).
  Average pool, per element: (hw 2^-24 + 2^-22) mean|x_i| + 2^-24, the error model of test_clamped_global_pool_against_fp64 -- hw - 1
  sequential fp32 adds and the division (2^-24 each, relative to at most sum|.|); its re-split term (2^-22) has no counterpart in a kernel
  that writes fp32 and is kept as slack, not tuned away.
  End to end: the fp32 batch-1 CPU loop is the yardstick.  With d = max |fp32 loop - fp64| over the 28 rows, the bound on |engine - fp64|
  and |engine - fp32 loop| is the project's 2e-5 when 4 d < 2e-5, else 4 d rounded up to one digit and never above 1e-4 (the AlexNet
  precedent).  The same argmax on EVERY row (tests/test_squeezenet_cpu.py asserts a top-two fp64 margin >= 1e-3 on exactly these rows).

End-to-end figures (rows of squeezenet_ref.E2E_CASES: 20 felzenszwalb + 8 grid masks): NOT YET MEASURED -- this file has not run on an
MI355X (DESIGN.md 14 says why); the test prints d, the bound and the three distances on every run, and DESIGN.md 14 is where they go."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import squeezenet_ref
from gpu_common import accepted_tiles, bits, dev, FALLBACK, GENERIC, layer_bound, merge, pitch_of, ptr, split  # noqa: F401  (dev is a fixture)
from net_harness import assert_layer_close, check_api, check_end_to_end, check_position_independence, conv_tile, e2e_rows, Reference, stage_stem_input
from network_interpretation_imagenet_amd import _lib, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine, MpxError
from oracle import scorer

pytestmark = pytest.mark.gpu

ARCH = "squeezenet1_1"
SENTINEL = 0x7e00           # an fp16 NaN bit pattern no kernel here produces from finite inputs
TAIL = 64


@pytest.fixture(scope="module")
def sd():
    return synth.make_state_dict(ARCH)


@pytest.fixture(scope="module")
def small_engine(mpx_lib, dev, sd):
    """A small workspace, for everything that hands the kernels device pointers of its own."""
    e = MaskedForwardEngine(ARCH, max_batch=8, device=0).load_state_dict(sd)
    yield e
    e.close()


@pytest.fixture(scope="module")
def engine(mpx_lib, dev, sd):
    e = MaskedForwardEngine(ARCH, device=0).load_state_dict(sd)            # the default max_batch
    yield e
    e.close()


def out_slice(eng, i):
    pitch, off = C.c_int(-1), C.c_int(-1)
    assert eng._lib.mpx_conv_out_slice(eng._h, i, C.byref(pitch), C.byref(off)) == 0
    return pitch.value, off.value


# ------------------------------------------------------------------------------------------------
# topology
# ------------------------------------------------------------------------------------------------
def _expected_default_tile(d, sliced):
    if d.cout <= 64:
        return 1 if d.ksize >= 3 else 4             # the stem, the squeeze convs, the 64-channel expands
    if sliced:
        return 0 if d.ksize == 3 else 7             # default_tile's rules restricted to the generic tiles
    return 7 if d.cout > d.cin else 2               # classifier.1: 512 -> 1000


def test_squeezenet_topology_slices_and_default_tiles(small_engine):
    eng = small_engine
    convs = squeezenet_ref.topology()
    assert len(convs) == 26 == len(eng.layers)
    assert [(d.name.decode(), d.bn_name.decode(), d.cin, d.cout, d.ksize, d.stride, d.pad, d.hin, d.hout, d.relu, d.residual) for d in eng.layers] == convs
    for d in eng.layers:
        assert d.cout_pad == -(-d.cout // 128) * 128
        assert d.k_packed == (96 if d.cin == 3 else d.ksize * d.ksize * pitch_of(d.cin))
    assert sorted({d.k_packed for d in eng.layers if b"expand1x1" in d.name}) == [32, 64]
    assert sorted({d.k_packed for d in eng.layers if b"expand3x3" in d.name}) == [288, 576]
    # where every layer writes: all 26
    want = squeezenet_ref.out_slices()
    got = [out_slice(eng, i) for i in range(26)]
    assert got == want
    for d, (pitch, off) in zip(eng.layers, got):
        if b"expand" in d.name:
            assert pitch == 2 * d.cout and off == (d.cout if b"expand3x3" in d.name else 0)
        else:
            assert off == 0 and pitch == (1000 if d.name == b"classifier.1" else pitch_of(d.cout))
    a, b = C.c_int(), C.c_int()
    assert eng._lib.mpx_conv_out_slice(eng._h, 26, C.byref(a), C.byref(b)) == -1 and eng._lib.mpx_conv_out_slice(eng._h, -1, C.byref(a), C.byref(b)) == -1
    assert eng._lib.mpx_conv_out_slice(eng._h, 0, None, C.byref(b)) == -1
    assert eng.flops_per_forward == 2.0 * squeezenet_ref.MACS
    geo = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert eng._lib.mpx_geometry(eng._h, *[C.byref(v) for v in geo]) == 0 and [v.value for v in geo] == [224, 3, 1000, 1000]
    for i, d in enumerate(eng.layers):
        t = eng._lib.mpx_get_conv_tile(eng._h, i)
        assert t == _expected_default_tile(d, b"expand" in d.name), (d.name, t)
    assert eng.stem == "conv" and not eng.has_stem_table and eng._lib.mpx_weights_complete(eng._h) == 1
    assert eng._lib.mpx_num_bottleneck_tails(eng._h) == 0 and eng._lib.mpx_num_norms(eng._h) == 0 and eng._lib.mpx_num_dwconvs(eng._h) == 0


def test_an_ordinary_engine_reports_whole_rows(mpx_lib, dev):
    r = MaskedForwardEngine("resnet18", max_batch=2, device=0)
    try:
        for i, d in enumerate(r.layers):
            assert out_slice(r, i) == (d.cout, 0)
    finally:
        r.close()


def test_squeezenet_default_max_batch_and_workspace(engine):
    eng = engine
    assert eng.max_batch == 512
    # per slot: three 111x111x64 split-fp16 buffers and the NHWC4 staging: 10.3 MB
    per_slot = 3 * 2 * 111 * 111 * 64 * 2 + 2 * 230 * 230 * 4 * 2
    w = sum(2 * d.cout_pad * d.k_packed * 2 for d in eng.layers)
    assert per_slot * 512 + w < eng.workspace_bytes < per_slot * 512 + w + (16 << 20)
    print("squeezenet1_1: %.2f MB per slot, workspace %.2f GB at max_batch 512" % (per_slot / 1e6, eng.workspace_bytes / 1e9))


# ------------------------------------------------------------------------------------------------
# per conv layer
# ------------------------------------------------------------------------------------------------
def _ref_layer(sd, d, x64):
    """fp64 conv + bias + ReLU on the device: [B][ho][ho][cout]."""
    name = d.name.decode()
    dev = x64.device
    y = F.conv2d(x64, sd[name + ".weight"].double().to(dev), sd[name + ".bias"].double().to(dev), d.stride, d.pad)
    return F.relu(y).permute(0, 2, 3, 1).contiguous()


class _Layer:
    """Inputs of layer i at `batch` images (drawn once) and its fp64 output (computed once); run(tile) launches it into fresh
    sentinel-filled planes of the layer's pitch plus a tail and returns (hi, lo) views [B][h][h][pitch], the tails, and the kernel mask."""

    def __init__(self, eng, sd, i, batch, seed):
        self.eng, self.i, self.batch = eng, i, batch
        d = self.d = eng.layers[i]
        dev = eng.device
        self.pitch, self.off = out_slice(eng, i)
        cin_p = d.cin if d.cin == 3 else pitch_of(d.cin)
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(batch, d.hin, d.hin, cin_p, generator=g).clamp_min(-0.5) * 1.5
        x[..., d.cin:] = 0.0                                    # padded channels hold exact zeros wherever they are read
        self.xh, self.xl = split(x.to(dev))
        x64 = merge(self.xh, self.xl).double()[..., :d.cin].permute(0, 3, 1, 2)
        self.want = _ref_layer(sd, d, x64)
        self.bound = layer_bound(d, self.want.abs().max().item())

    def run(self, tile):
        eng, d, i, batch = self.eng, self.d, self.i, self.batch
        dev = eng.device
        with conv_tile(eng, i, tile):
            if i == 0:
                stage_stem_input(eng, self.xh, self.xl, batch)
                in_h = in_l = None
            else:
                in_h, in_l = self.xh, self.xl
            n = batch * d.hout * d.hout * self.pitch
            oh = torch.full((n + TAIL,), SENTINEL, dtype=torch.int16, device=dev).view(torch.float16)
            ol = torch.full((n + TAIL,), SENTINEL, dtype=torch.int16, device=dev).view(torch.float16)
            rc = eng._lib.mpx_conv_bn_act(eng._h, i, ptr(in_h), ptr(in_l), None, None, ptr(oh), ptr(ol), None, batch, eng._stream())
            _lib.check(eng._h, rc, "mpx_conv_bn_act")
            torch.cuda.synchronize()
            ran = eng._lib.mpx_last_conv_kernels(eng._h)
        shape = (batch, d.hout, d.hout, self.pitch)
        return oh[:n].view(shape), ol[:n].view(shape), (oh[n:], ol[n:]), ran

    def check(self, oh, ol, tile, ran):
        """Channels [off, off + cout) against fp64."""
        d = self.d
        got = merge(oh[..., self.off:self.off + d.cout], ol[..., self.off:self.off + d.cout]).double()
        assert not torch.isnan(got).any(), d.name
        fields = "%d->%d k%d h%d K %d pitch %d offset %d " % (d.cin, d.cout, d.ksize, d.hin, d.k_packed, self.pitch, self.off)
        assert_layer_close(d, got, self.want, tile, self.batch, ran, fields)


def test_every_distinct_conv_shape_on_every_accepted_tile(small_engine, sd):
    """All 18 distinct (cin, cout, ksize, hin) of the network at batch 3 (M = 36963, 9075, 2187 and 507 output pixels: a ragged last tile on
    every tile size) on every tile mpx_set_conv_tile accepts: the stem (3x3 stride 2 pad 0 on the NHWC4 staging), the 8 squeeze convs (16
    and 48 channels stored with pitch 32 and 64: exact zeros behind them), the 4 + 4 expand convs (output slices: the generic tiles only;
    everything outside the slice keeps its sentinel) and classifier.1 (planes of pitch 1000, not an fc layer)."""
    eng = small_engine
    seen, padded, sliced = set(), 0, 0
    for i, d in enumerate(eng.layers):
        key = (d.cin, d.cout, d.ksize, d.hin)
        if key in seen:
            continue
        seen.add(key)
        accepted = accepted_tiles(eng, i)
        default = eng._lib.mpx_get_conv_tile(eng._h, i)
        assert default in accepted and GENERIC <= set(accepted), (d.name, accepted)
        is_slice = b"expand" in d.name
        if is_slice or d.cin % 32 or d.cout % 32 or i == 0:
            assert set(accepted) == GENERIC, (d.name, accepted)             # slices, padded layers and the stem: the generic tiles only
        layer = _Layer(eng, sd, i, 3, seed=1000 * i + 3)
        for t in accepted:
            oh, ol, (th, tl), ran = layer.run(t)
            assert ran & ((1 << t) | (1 << FALLBACK.get(t, t))), (d.name, t, ran)
            if t not in FALLBACK:
                assert ran == 1 << t, (d.name, t, ran)
            layer.check(oh, ol, t, ran)
            assert (bits(th) == SENTINEL).all() and (bits(tl) == SENTINEL).all(), (d.name, t)          # nothing behind the planes
            if is_slice:
                other = slice(d.cout, 2 * d.cout) if layer.off == 0 else slice(0, d.cout)
                assert (bits(oh[..., other]) == SENTINEL).all() and (bits(ol[..., other]) == SENTINEL).all(), (d.name, t)
            elif layer.pitch > d.cout:                                                                  # padded squeeze channels: exact zeros
                assert (bits(oh[..., d.cout:]) == 0).all() and (bits(ol[..., d.cout:]) == 0).all(), (d.name, t)
        padded += (not is_slice) and layer.pitch > d.cout
        sliced += is_slice
    print("distinct conv shapes checked: %d (padded: %d, output slices: %d)" % (len(seen), padded, sliced))
    assert len(seen) == 18 and padded == 4 and sliced == 8
    # a slice layer takes no residual operand and no fp32 output
    z = torch.zeros(3 * 55 * 55 * 128 + TAIL, dtype=torch.float16, device=eng.device)
    f = torch.zeros(16, dtype=torch.float32, device=eng.device)
    assert eng._lib.mpx_conv_bn_act(eng._h, 2, ptr(z), ptr(z), ptr(z), ptr(z), ptr(z), ptr(z), None, 1, None) == -1
    assert eng._lib.mpx_conv_bn_act(eng._h, 2, ptr(z), ptr(z), None, None, ptr(z), ptr(z), ptr(f), 1, None) == -1
    # classifier.1 is the last entry but writes planes: an fp32 output is refused, and so are missing planes
    assert eng._lib.mpx_conv_bn_act(eng._h, 25, ptr(z), ptr(z), None, None, None, None, ptr(f), 1, None) == -1
    assert eng._lib.mpx_conv_bn_act(eng._h, 25, ptr(z), ptr(z), None, None, ptr(z), ptr(z), ptr(f), 1, None) == -1


@pytest.mark.parametrize("fire,e,h", [(3, 64, 55), (9, 192, 13)])
def test_expand_convs_fill_their_halves_of_one_buffer_and_nothing_else(small_engine, sd, fire, e, h):
    """Concatenated planes [3][h][h][2e] plus a 64-element tail, prefilled with a NaN bit pattern.  After expand1x1 alone channels [0, e) pass
    the layer bound and channels [e, 2e) and the tail still hold the sentinel bits; the same the other way round for expand3x3; after both
    launches into ONE buffer no sentinel is left inside the planes and the tail is intact.  On every tile the layers accept."""
    eng = small_engine
    names = [d.name.decode() for d in eng.layers]
    i1, i3 = names.index("features.%d.expand1x1" % fire), names.index("features.%d.expand3x3" % fire)
    assert (eng.layers[i1].cout, eng.layers[i1].hin) == (e, h) and out_slice(eng, i1) == (2 * e, 0) and out_slice(eng, i3) == (2 * e, e)
    l1, l3 = _Layer(eng, sd, i1, 3, seed=fire), _Layer(eng, sd, i3, 3, seed=fire)      # the same seed: the same squeeze map
    assert torch.equal(l1.xh, l3.xh) and torch.equal(l1.xl, l3.xl)
    accepted = accepted_tiles(eng, i1)
    assert set(accepted) == GENERIC == set(accepted_tiles(eng, i3))
    n = 3 * h * h * 2 * e
    for t in accepted:
        for layer, mine, other in ((l1, slice(0, e), slice(e, 2 * e)), (l3, slice(e, 2 * e), slice(0, e))):
            oh, ol, (th, tl), ran = layer.run(t)
            assert ran == 1 << t
            layer.check(oh, ol, t, ran)
            assert (bits(oh[..., other]) == SENTINEL).all() and (bits(ol[..., other]) == SENTINEL).all(), (layer.d.name, t)
            assert (bits(th) == SENTINEL).all() and (bits(tl) == SENTINEL).all(), (layer.d.name, t)
            assert not (bits(oh[..., mine]) == SENTINEL).any() and not (bits(ol[..., mine]) == SENTINEL).any()
        # both launches into one buffer
        bh = torch.full((n + TAIL,), SENTINEL, dtype=torch.int16, device=eng.device).view(torch.float16)
        bl = torch.full((n + TAIL,), SENTINEL, dtype=torch.int16, device=eng.device).view(torch.float16)
        for i in (i1, i3):
            with conv_tile(eng, i, t):
                _lib.check(eng._h, eng._lib.mpx_conv_bn_act(eng._h, i, ptr(l1.xh), ptr(l1.xl), None, None, ptr(bh), ptr(bl), None, 3, eng._stream()), "mpx_conv_bn_act")
        torch.cuda.synchronize()
        assert not (bits(bh[:n]) == SENTINEL).any() and not (bits(bl[:n]) == SENTINEL).any(), t
        assert (bits(bh[n:]) == SENTINEL).all() and (bits(bl[n:]) == SENTINEL).all(), t
        cat = merge(bh[:n], bl[:n]).double().view(3, h, h, 2 * e)
        want = torch.cat([l1.want, l3.want], 3)
        assert (cat - want).abs().max().item() <= max(l1.bound, l3.bound), t


# ------------------------------------------------------------------------------------------------
# the average pool that writes the logits
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,c,batch,pitch", [(169, 1000, 3, 1000), (169, 1000, 67, 1016), (49, 16, 5, 40)])
def test_global_avgpool_logits_against_fp64(small_engine, dev, hw, c, batch, pitch):
    eng = small_engine
    g = torch.Generator().manual_seed(hw + c)
    x = torch.randn(batch, hw, c, generator=g).clamp_min(-0.25) * 4.0     # post-ReLU-like with a few negatives: the kernel must not care
    x[..., : c // 4] *= 1e-3                                               # lo in fp16's subnormals
    xh, xl = split(x.to(dev))
    out = torch.full((batch * pitch + TAIL,), float("nan"), dtype=torch.float32, device=dev)
    _lib.check(eng._h, eng._lib.mpx_global_avgpool_logits(eng._h, ptr(xh), ptr(xl), ptr(out), batch, hw, c, pitch, eng._stream()), "mpx_global_avgpool_logits")
    torch.cuda.synchronize()
    rows = out[: batch * pitch].view(batch, pitch)
    assert torch.isnan(out[batch * pitch:]).all() and torch.isnan(rows[:, c:]).all()          # pitch padding and tail untouched
    x64 = merge(xh, xl).double()
    want = x64.mean(1)
    tol = (hw * 2.0 ** -24 + 2.0 ** -22) * x64.abs().mean(1) + 2.0 ** -24
    got = rows[:, :c].double()
    err = (got - want).abs()
    print("average pool -> logits %d x %d batch %d pitch %d: max err %.3e, worst err / bound %.3f" % (hw, c, batch, pitch, err.max().item(), (err / tol).max().item()))
    assert not torch.isnan(got).any() and (err <= tol).all()
    # what the kernel states: the exact sum (fp64 holds it: every value is a multiple of 2^-24 below 2^16), divided in fp64, rounded to fp32
    x64c = x64.cpu()
    assert (x64c.abs().max() < 2.0 ** 16) and torch.equal(x64c * 2.0 ** 24, (x64c * 2.0 ** 24).round())
    assert torch.equal(rows[:, :c].cpu(), (x64c.sum(1) / float(hw)).float())
    assert (err <= 2.0 ** -24 * (1 + 2.0 ** -20) * want.abs() + 2.0 ** -149).all()             # ... which is within one fp32 rounding of the mean
    z, o = ptr(xh), ptr(out)
    call = eng._lib.mpx_global_avgpool_logits
    assert call(eng._h, None, z, o, 1, hw, c, pitch, None) == -1           # null planes
    assert call(eng._h, z, None, o, 1, hw, c, pitch, None) == -1
    assert call(eng._h, z, z, None, 1, hw, c, pitch, None) == -1           # null output
    assert call(eng._h, z, z, o, 0, hw, c, pitch, None) == -1              # B <= 0
    assert call(eng._h, z, z, o, -3, hw, c, pitch, None) == -1
    assert call(eng._h, z, z, o, 1, hw, 12, pitch, None) == -1             # c not a multiple of 8
    assert call(eng._h, z, z, o, 1, hw, c, c - 8, None) == -1              # out_pitch < c


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
def test_squeezenet_end_to_end(engine, sd, golden_dir):
    """Logits lens (tests/logits_lens.py): all 1000 logits of every row against fp64, bound 4 d_L with d_L = the fp32 CPU loop's distance.
    Measured on one MI355X: squeezenet1_1 d_L 2.53e-06, engine 3.94e-06 (1.55).  With the single fp32 accumulator that
    mpx_global_avgpool_logits had before, the engine was at 1.09e-05 (4.30) and this assertion failed: partial sums near 3000 have an fp32
    step of 2.4e-4, and 169 of them walk 5e-6 .. 1e-5 in the mean.  The pool now sums in fp64, exactly."""
    ref = Reference(squeezenet_ref, sd)
    check_end_to_end(engine, ARCH, ref, e2e_rows(ref, squeezenet_ref.E2E_CASES, golden_dir),
                     "%(arch)s: yardstick distance d = %(d).3e over the 28 rows -> end-to-end bound %(bound).1e")


def test_a_mask_row_scores_the_same_bits_wherever_it_sits(engine, golden_dir):
    check_position_independence(engine, *squeezenet_ref.e2e_inputs(golden_dir, "felz"), (8, ((1, 0, (0,)), (37, 41, (0, 5, 36)), (700, 44, (3, 511, 512, 699)))))


# ------------------------------------------------------------------------------------------------
# API and errors
# ------------------------------------------------------------------------------------------------
def test_api_on_a_squeezenet_engine(engine, sd, golden_dir):
    check_api(engine, Reference(squeezenet_ref, sd), *squeezenet_ref.e2e_inputs(golden_dir, "felz"))


def test_profile_lists_the_average_pool_launch(engine, dev):
    eng = engine
    img = torch.from_numpy(synth.make_images(1, kind="noise")[0]).to(dev)
    seg = torch.from_numpy(synth.grid_segments()).to(dev)
    onoff = torch.from_numpy(synth.random_onoff(4, 196)).to(dev)
    labels = torch.zeros(4, dtype=torch.int32, device=dev)
    eng.profile(True)
    eng.stage_masks(img, seg, onoff, 0)
    eng.forward(4, labels)
    eng.profile(False)
    prof = eng.collect_profile()
    assert prof["per_dw_ms"] == [] and prof["per_norm_ms"] == [] and prof["avgpool2_ms"] == 0
    assert prof["launches"]["pool"] == 3 + 1                # the three max pools and the average pool that writes the logits
    assert prof["launches"]["conv"] == len(eng.layers) == 26 and all(ms > 0 for ms in prof["per_conv_ms"])
    assert prof["launches"]["head"] == 1 and prof["launches"]["mask_apply_normalize"] == 1
    assert sum(prof["launches"].values()) == 32             # K0 + the 31 launches of a forward batch
    assert prof["ms"]["pool"] > 0


def test_squeezenet_error_paths(small_engine, mpx_lib, dev, sd):
    eng = small_engine
    with pytest.raises(ValueError):
        MaskedForwardEngine(ARCH, max_batch=2, device=0, stem="table")
    with pytest.raises(ValueError):
        eng.score_masks(synth.make_images(1)[0], synth.grid_segments(), synth.random_onoff(2, 196), 0, stem="table")
    with pytest.raises(ValueError, match="AlexNet"):
        MaskedForwardEngine("squeezenet1_0", max_batch=2, device=0)
    z = torch.zeros(224, 224, dtype=torch.int32, device=dev)
    im = torch.zeros(224, 224, 3, dtype=torch.uint8, device=dev)
    on = torch.ones(1, 1, dtype=torch.uint8, device=dev)
    mean = (C.c_float * 3)(*scorer.MEAN)
    std = (C.c_float * 3)(*scorer.STD)
    assert eng._lib.mpx_stem_table_build(eng._h, ptr(im), None, ptr(z), 1, mean, std, None) == -2
    assert eng._lib.mpx_stem_table_apply(eng._h, ptr(on), 1, 1, 0, None) == -2
    buf = torch.zeros(64, dtype=torch.float16, device=dev)
    assert eng._lib.mpx_stem_conv_maxpool(eng._h, ptr(buf), ptr(buf), 1, None) == -2
    for bad in (7000, 7010, 7012, 7999):
        h = C.c_void_p()
        assert mpx_lib.mpx_create(bad, 2, 0, C.byref(h)) == -1 and not h.value
    fresh = MaskedForwardEngine(ARCH, max_batch=2, device=0)
    try:
        assert fresh._lib.mpx_weights_complete(fresh._h) == 0
        fresh.stage_masks(im, z, on, 0)
        labels = torch.zeros(1, dtype=torch.int32, device=dev)
        with pytest.raises(MpxError):
            fresh.forward(1, labels)                                        # no weights yet
        with pytest.raises((KeyError, ValueError)):
            fresh.load_state_dict(synth.make_state_dict("vgg11"))           # a VGG state_dict: features.3.squeeze.* is missing
        assert fresh._lib.mpx_weights_complete(fresh._h) == 0
        with pytest.raises(KeyError):
            fresh.load_state_dict(sd, only=["features.3.expand5x5"])
        fresh.load_state_dict(sd)
        assert fresh._lib.mpx_weights_complete(fresh._h) == 1
        score, pred = fresh.forward(1, labels)[:2]
        torch.cuda.synchronize()
        assert 0.0 <= float(score[0]) <= 1.0
    finally:
        fresh.close()
