"""GoogLeNet on the MI355X (pytest -m gpu), through the C-ABI as tests/test_gpu_squeezenet.py does: the clipped-window 3x3 max pool bit for
bit against F.max_pool2d(ceil_mode=True), the topology and where every layer writes, the four-way concatenation through the SLICE form of
the generic kernel against sentinel-filled planes, every distinct conv shape on every tile it accepts against an fp64 conv + BatchNorm
(eps 1e-3) + ReLU of the same split inputs, the whole network against the batch-1 fp32 CPU loop and the fp64 restatement
(tests/googlenet_ref.py), position independence of a mask row, the reference-named API, the profile's pool launches and the error paths.

Bounds.
  Pool: none -- torch.equal, and the (hi, lo) bits of the output equal the split of the expected values.
  Per conv layer: 4e-6 sqrt(max(K, 4608) / 4608) of max(|want|, 1), the project's per-layer bound (every K here is <= 1728: 4e-6).
  End to end: the fp32 batch-1 CPU loop is the yardstick.  With d = max |fp32 loop - fp64| over the 28 rows, the bound on |engine - fp64|
  and |engine - fp32 loop| is the project's 2e-5 when 4 d < 2e-5, else 4 d rounded up to one digit and never above 1e-4 (the rule of
  tests/test_gpu_squeezenet.py).  The same argmax on EVERY row (tests/test_googlenet_cpu.py asserts a top-two fp64 margin >= 1e-3 on
  exactly these rows).

End-to-end figures (rows of googlenet_ref.E2E_CASES: 20 felzenszwalb + 8 grid masks): NOT YET MEASURED -- of this file only the first pool
case has run on an MI355X (DESIGN.md 15 says why); the test prints d, the bound and the three distances on every run, and DESIGN.md 15 is
where they go."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import googlenet_ref
from gpu_common import accepted_tiles, bits, dev, FALLBACK, GENERIC, layer_bound, merge, pitch_of, ptr, split  # noqa: F401  (dev is a fixture)
from net_harness import assert_layer_close, check_api, check_end_to_end, check_position_independence, conv_tile, e2e_rows, Reference, stage_stem_input
from network_interpretation_imagenet_amd import _lib, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine, MpxError
from oracle import scorer

pytestmark = pytest.mark.gpu

ARCH = "googlenet"
SENTINEL = 0x7e00           # an fp16 NaN bit pattern no kernel here produces from finite inputs
TAIL = 64
SLICE_SUFFIXES = (b"branch1.conv", b"branch2.1.conv", b"branch3.1.conv", b"branch4.1.conv")      # the last conv of each Inception branch


def sentinel_planes(n, dev):
    return (torch.full((n + TAIL,), SENTINEL, dtype=torch.int16, device=dev).view(torch.float16),
            torch.full((n + TAIL,), SENTINEL, dtype=torch.int16, device=dev).view(torch.float16))


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
# the clipped-window 3x3 max pool
# ------------------------------------------------------------------------------------------------
POOL_CASES = ((4, 2, 0, 2), (8, 2, 0, 4),           # the last window is clipped
              (7, 2, 0, 3), (3, 2, 0, 1),           # nothing is clipped
              (1, 1, 1, 1), (2, 1, 1, 2),           # every window is clipped on both sides
              (7, 1, 1, 7), (14, 1, 1, 14))


def fixed_point_split(x):
    """(hi, lo) with split(hi + lo) == (hi, lo).  split(x) alone is not always one: where lo is rounded coarsely (fp16 subnormals) hi + lo can
    sit on the other side of a rounding tie of hi.  The kernel hands on the PAIR of the winning element, so its output equals the split of
    the expected VALUE only for pairs that are such fixed points; re-splitting the merged value gets there in a step or two."""
    hi, lo = split(x)
    for _ in range(4):
        h2, l2 = split(merge(hi, lo))
        if torch.equal(bits(h2), bits(hi)) and torch.equal(bits(l2), bits(lo)):
            return hi, lo
        hi, lo = h2, l2
    raise AssertionError("split did not reach a fixed point")


def _run_pool(eng, x, stride, pad):
    """x: f32 [B][hin][hin][pitch] on the CPU.  Runs the kernel into sentinel-filled planes with a tail; checks the output bit for bit against
    F.max_pool2d(ceil_mode=True) of the merged planes and the tail; returns the merged output (CPU)."""
    dev = eng.device
    B, hin, _w, pitch = x.shape
    xh, xl = fixed_point_split(x.to(dev))
    want = F.max_pool2d(merge(xh, xl).cpu().permute(0, 3, 1, 2), 3, stride, pad, 1, ceil_mode=True).permute(0, 2, 3, 1).contiguous()
    ho = want.shape[1]
    assert ho == googlenet_ref.pool_side(hin, 3, stride, pad)
    n = B * ho * ho * pitch
    oh, ol = sentinel_planes(n, dev)
    rc = eng._lib.mpx_maxpool3x3_clip(eng._h, ptr(xh), ptr(xl), ptr(oh), ptr(ol), B, hin, stride, pad, pitch, eng._stream())
    _lib.check(eng._h, rc, "mpx_maxpool3x3_clip")
    torch.cuda.synchronize()
    assert (bits(oh[n:]) == SENTINEL).all() and (bits(ol[n:]) == SENTINEL).all(), "wrote past the end"
    gh, gl = oh[:n].view(B, ho, ho, pitch).cpu(), ol[:n].view(B, ho, ho, pitch).cpu()
    got = merge(gh, gl)
    assert torch.equal(got, want), (hin, stride, pad, pitch, B, (got - want).abs().max().item())
    wh, wl = split(want)
    assert torch.equal(bits(gh), bits(wh)) and torch.equal(bits(gl), bits(wl)), (hin, stride, pad, pitch, B)
    return got


@pytest.mark.parametrize("hin,stride,pad,ho", POOL_CASES)
def test_clipped_pool_is_max_pool2d_ceil_mode_bit_for_bit(small_engine, hin, stride, pad, ho):
    """Pitches 8, 96 and 544, batches 1 and 3, signed data with lo parts down to fp16's subnormals."""
    g = torch.Generator().manual_seed(100 * hin + 10 * stride + pad)
    for pitch in (8, 96, 544):
        for B in (1, 3):
            x = torch.randn(B, hin, hin, pitch, generator=g) * 3.0
            x[..., : pitch // 4] *= 1e-3
            got = _run_pool(small_engine, x, stride, pad)
            assert got.shape[1] == ho


def test_clipped_pool_strides_over_a_capped_grid(small_engine):
    """B = 3, hin = 56, pitch 544, stride 1: 10.2 MB per plane.  A thread takes 8 channels of a run of 4 output pixels, so the launch has
    3 * 56 * 14 * 68 = 159,936 units; the grid is capped at two 256-thread workgroups per CU (131,072 threads on 256 CUs, fewer on a
    partitioned device), so the stride loop takes a second round."""
    eng = small_engine
    assert 3 * 56 * 14 * 68 > eng.num_cus * 2 * 256
    g = torch.Generator().manual_seed(56)
    x = torch.randn(3, 56, 56, 544, generator=g) * 2.0
    _run_pool(eng, x, 1, 1)


@pytest.mark.parametrize("stride,pad,hin", [(1, 1, 7), (2, 0, 8)])
def test_clipped_pool_keeps_an_all_negative_map_negative(small_engine, stride, pad, hin):
    """A kernel that read clipped taps as zero would write zeros along the border."""
    g = torch.Generator().manual_seed(stride)
    x = -(torch.rand(3, hin, hin, 96, generator=g) * 4.0 + 0.25)
    got = _run_pool(small_engine, x, stride, pad)
    assert (got < 0).all()


@pytest.mark.parametrize("stride,pad,hin", [(1, 1, 14), (2, 0, 8)])
def test_clipped_pool_on_a_map_with_ties(small_engine, stride, pad, hin):
    g = torch.Generator().manual_seed(7 + stride)
    x = torch.randint(-2, 3, (3, hin, hin, 96), generator=g).float() * 0.5            # five values: nearly every window has a tie
    _run_pool(small_engine, x, stride, pad)


# ------------------------------------------------------------------------------------------------
# topology
# ------------------------------------------------------------------------------------------------
def _expected_default_tile(d, sliced):
    if d.cout <= 64:
        return 1 if d.ksize >= 3 else 4
    if sliced:
        return 0 if d.ksize == 3 else (7 if d.cout > d.cin else 2)     # default_tile's rules restricted to the generic tiles
    return None                                                        # an ordinary layer: whatever default_tile says of its descriptor


def test_googlenet_topology_slices_pools_and_default_tiles(small_engine):
    eng = small_engine
    convs = googlenet_ref.topology()
    assert len(convs) == 58 == len(eng.layers)
    assert [(d.name.decode(), d.bn_name.decode(), d.cin, d.cout, d.ksize, d.stride, d.pad, d.hin, d.hout, d.relu, d.residual) for d in eng.layers] == convs
    want = googlenet_ref.out_slices()
    for i, (d, (pitch, off, store)) in enumerate(zip(eng.layers, want)):
        assert out_slice(eng, i) == (pitch, off), d.name
        assert d.cout_pad == -(-max(d.cout, store) // 128) * 128, d.name
        assert d.k_packed == (224 if d.cin == 3 else d.ksize * d.ksize * pitch_of(d.cin)), d.name
        sliced = d.name.endswith(SLICE_SUFFIXES)
        assert sliced or (off == 0 and pitch == (1000 if d.name == b"fc" else pitch_of(d.cout)) == store), d.name
        t = eng._lib.mpx_get_conv_tile(eng._h, i)
        exp = _expected_default_tile(d, sliced)
        assert exp is None or t == exp, (d.name, t)
        if sliced:
            assert t in GENERIC
    names = [d.name.decode() for d in eng.layers]
    k = names.index("inception4e.branch1.conv")
    assert [eng.layers[k + j].k_packed for j in (0, 1, 3, 5)] == [544] * 4         # inception4e's 1x1 convs read inception4d's pitch
    assert out_slice(eng, names.index("inception4d.branch4.1.conv")) == (544, 464)
    a, b = C.c_int(), C.c_int()
    assert eng._lib.mpx_conv_out_slice(eng._h, 58, C.byref(a), C.byref(b)) == -1
    # the clipped pools of the forward
    assert eng._lib.mpx_num_clip_pools(eng._h) == 12
    got = []
    for k in range(12):
        v = [C.c_int() for _ in range(4)]
        assert eng._lib.mpx_clip_pool_info(eng._h, k, *[C.byref(q) for q in v]) == 0
        got.append(tuple(q.value for q in v))
    assert got == googlenet_ref.clip_pools()
    assert eng._lib.mpx_clip_pool_info(eng._h, 12, None, None, None, None) == -1
    assert eng.flops_per_forward == 2.0 * googlenet_ref.MACS
    geo = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert eng._lib.mpx_geometry(eng._h, *[C.byref(v) for v in geo]) == 0 and [v.value for v in geo] == [224, 3, 1000, 1000]
    assert eng.stem == "conv" and not eng.has_stem_table and eng._lib.mpx_weights_complete(eng._h) == 1
    assert eng._lib.mpx_num_bottleneck_tails(eng._h) == 0 and eng._lib.mpx_num_norms(eng._h) == 0 and eng._lib.mpx_num_dwconvs(eng._h) == 0


def test_other_engines_have_no_clipped_pools(mpx_lib, dev):
    r = MaskedForwardEngine("resnet18", max_batch=2, device=0)
    try:
        assert r._lib.mpx_num_clip_pools(r._h) == 0 and r._lib.mpx_clip_pool_info(r._h, 0, None, None, None, None) == -1
    finally:
        r.close()


def test_googlenet_default_max_batch_and_workspace(engine):
    eng = engine
    assert eng.max_batch == 512
    # per slot: three 112x112x64 split-fp16 buffers and the NHWC4 staging: 10.5 MB
    per_slot = 3 * 2 * 112 * 112 * 64 * 2 + 2 * 230 * 230 * 4 * 2
    w = sum(2 * d.cout_pad * d.k_packed * 2 for d in eng.layers)
    assert per_slot * 512 + w < eng.workspace_bytes < per_slot * 512 + w + (16 << 20)
    print("googlenet: %.2f MB per slot, workspace %.2f GB at max_batch 512" % (per_slot / 1e6, eng.workspace_bytes / 1e9))


# ------------------------------------------------------------------------------------------------
# per conv layer
# ------------------------------------------------------------------------------------------------
def _ref_layer(sd, d, x64):
    """fp64 conv + BatchNorm (eps 1e-3) + ReLU on the device: [B][ho][ho][cout]."""
    name, bn = d.name.decode(), d.bn_name.decode()
    dev = x64.device
    t = {k: sd["%s.%s" % (bn, k)].double().to(dev) for k in ("weight", "bias", "running_mean", "running_var")}
    y = F.conv2d(x64, sd[name + ".weight"].double().to(dev), None, d.stride, d.pad)
    y = F.batch_norm(y, t["running_mean"], t["running_var"], t["weight"], t["bias"], False, 0.0, googlenet_ref.BN_EPS)
    return F.relu(y).permute(0, 2, 3, 1).contiguous()


class _Layer:
    """Inputs of layer i at `batch` images (drawn once) and its fp64 output (computed once); run(tile) launches it into fresh
    sentinel-filled planes of the layer's pitch plus a tail and returns (hi, lo) views [B][h][h][pitch], the tails, and the kernel mask."""

    def __init__(self, eng, sd, i, batch, seed):
        self.eng, self.i, self.batch = eng, i, batch
        d = self.d = eng.layers[i]
        dev = eng.device
        self.pitch, self.off, self.store = googlenet_ref.out_slices()[i]
        assert out_slice(eng, i) == (self.pitch, self.off)
        cin_p = d.cin if d.cin == 3 else pitch_of(d.cin)
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(batch, d.hin, d.hin, cin_p, generator=g).clamp_min(-0.5) * 1.5
        x[..., d.cin:] = 0.0                                    # padded channels hold exact zeros wherever they are read
        self.xh, self.xl = split(x.to(dev))
        x64 = merge(self.xh, self.xl).double()[..., :d.cin].permute(0, 3, 1, 2)
        self.want = _ref_layer(sd, d, x64)
        self.bound = layer_bound(d, self.want.abs().max().item())

    def run(self, tile, out=None):
        """out: (hi, lo) planes to write into instead of fresh sentinel-filled ones."""
        eng, d, i, batch = self.eng, self.d, self.i, self.batch
        dev = eng.device
        with conv_tile(eng, i, tile):
            if i == 0:
                stage_stem_input(eng, self.xh, self.xl, batch)
                in_h = in_l = None
            else:
                in_h, in_l = self.xh, self.xl
            n = batch * d.hout * d.hout * self.pitch
            oh, ol = out if out is not None else sentinel_planes(n, dev)
            rc = eng._lib.mpx_conv_bn_act(eng._h, i, ptr(in_h), ptr(in_l), None, None, ptr(oh), ptr(ol), None, batch, eng._stream())
            _lib.check(eng._h, rc, "mpx_conv_bn_act")
            torch.cuda.synchronize()
            ran = eng._lib.mpx_last_conv_kernels(eng._h)
        shape = (batch, d.hout, d.hout, self.pitch)
        return oh[:n].view(shape), ol[:n].view(shape), (oh[n:], ol[n:]), ran

    def check(self, oh, ol, tile, ran):
        """Channels [off, off + cout) against fp64; [off + cout, off + store) exact zeros; everything else of the pixel rows and the tail
        untouched (call with fresh sentinel-filled planes)."""
        d = self.d
        mine = slice(self.off, self.off + d.cout)
        got = merge(oh[..., mine], ol[..., mine]).double()
        assert not torch.isnan(got).any(), d.name
        fields = "%d->%d k%d h%d K %d pitch %d offset %d stored %d " % (d.cin, d.cout, d.ksize, d.hin, d.k_packed, self.pitch, self.off, self.store)
        assert_layer_close(d, got, self.want, tile, self.batch, ran, fields)
        pad = slice(self.off + d.cout, self.off + self.store)
        assert (bits(oh[..., pad]) == 0).all() and (bits(ol[..., pad]) == 0).all(), (d.name, tile)      # pad channels: exact zeros
        for other in (slice(0, self.off), slice(self.off + self.store, self.pitch)):
            assert (bits(oh[..., other]) == SENTINEL).all() and (bits(ol[..., other]) == SENTINEL).all(), (d.name, tile, other)


_GROUPS = ("conv",) + tuple(m[0] for m in googlenet_ref.MODULES)
def _first_of_each_shape():
    """layer index -> True for the first layer of the conv list with its (cin, cout, ksize, hin): the 49 layers the per-shape test runs."""
    seen, first = set(), set()
    for i, c in enumerate(googlenet_ref.topology()[:-1]):
        key = (c[2], c[3], c[4], c[7])
        if key not in seen:
            seen.add(key)
            first.add(i)
    return first


@pytest.mark.parametrize("group", _GROUPS)
def test_every_distinct_conv_shape_on_every_accepted_tile(small_engine, sd, group):
    """The 49 distinct (cin, cout, ksize, hin) of the network, one group of layers per case (the three convs in front, then each Inception
    module; a shape an earlier layer of the list already has is that layer's to check), at batch 3 (M = 37632, 9408, 2352, 588 and 147 output pixels: a ragged
    last tile on every tile size) on every tile mpx_set_conv_tile accepts.  Slices and layers with padded channels accept the generic
    tiles only.  Everything a layer must not write keeps its sentinel; pad channels are exact zeros."""
    eng = small_engine
    checked = 0
    first = _first_of_each_shape()
    assert len(first) == 49
    for i, d in enumerate(eng.layers[:-1]):
        if not d.name.decode().startswith(group) or i not in first:
            continue
        accepted = accepted_tiles(eng, i)
        default = eng._lib.mpx_get_conv_tile(eng._h, i)
        assert default in accepted and GENERIC <= set(accepted), (d.name, accepted)
        layer = _Layer(eng, sd, i, 3, seed=1000 * i + 3)
        is_slice = d.name.endswith(SLICE_SUFFIXES)
        if is_slice or d.cin % 32 or i == 0:
            assert set(accepted) == GENERIC, (d.name, accepted)
        for t in accepted:
            oh, ol, (th, tl), ran = layer.run(t)
            assert ran & ((1 << t) | (1 << FALLBACK.get(t, t))), (d.name, t, ran)
            if t not in FALLBACK:
                assert ran == 1 << t, (d.name, t, ran)
            layer.check(oh, ol, t, ran)
            assert (bits(th) == SENTINEL).all() and (bits(tl) == SENTINEL).all(), (d.name, t)          # nothing behind the planes
        checked += 1
    print("%s: %d distinct conv shapes checked" % (group, checked))
    assert checked >= 1


@pytest.mark.parametrize("module,h,pitch,offsets,stores", [("inception3a", 28, 256, (0, 64, 192, 224), (64, 128, 32, 32)),
                                                           ("inception4d", 14, 544, (0, 112, 400, 464), (112, 288, 64, 80))])
def test_branch_convs_fill_their_ranges_of_one_buffer_and_nothing_else(small_engine, sd, module, h, pitch, offsets, stores):
    """Concatenated planes [3][h][h][pitch] plus a tail, prefilled with a NaN bit pattern.  Each of the four slice convs alone, on every tile
    it accepts: inside its range the layer bound, outside it the sentinel (_Layer.check).  Then all four into ONE buffer: no sentinel is left,
    the tail is intact, the concatenation passes the bound, and inception4d's channels 528 .. 543 are exact zeros."""
    eng = small_engine
    names = [d.name.decode() for d in eng.layers]
    idx = [names.index("%s.%s.conv" % (module, br)) for br in ("branch1", "branch2.1", "branch3.1", "branch4.1")]
    layers = [_Layer(eng, sd, i, 3, seed=17 * i) for i in idx]
    assert [(l.pitch, l.off, l.store) for l in layers] == [(pitch, o, s) for o, s in zip(offsets, stores)]
    assert all(l.d.hin == h for l in layers)
    tiles = None
    for l in layers:
        accepted = accepted_tiles(eng, l.i)
        assert set(accepted) == GENERIC, (l.d.name, accepted)
        tiles = accepted
        for t in accepted:
            oh, ol, (th, tl), ran = l.run(t)
            assert ran == 1 << t
            l.check(oh, ol, t, ran)
            assert (bits(th) == SENTINEL).all() and (bits(tl) == SENTINEL).all(), (l.d.name, t)
    n = 3 * h * h * pitch
    width = sum(l.d.cout for l in layers)
    for t in tiles:
        bh, bl = sentinel_planes(n, eng.device)
        for l in layers:
            l.run(t, out=(bh, bl))
        assert not (bits(bh[:n]) == SENTINEL).any() and not (bits(bl[:n]) == SENTINEL).any(), t
        assert (bits(bh[n:]) == SENTINEL).all() and (bits(bl[n:]) == SENTINEL).all(), t
        cat = merge(bh[:n], bl[:n]).double().view(3, h, h, pitch)
        want = torch.cat([l.want for l in layers], 3)
        assert (cat[..., :width] - want).abs().max().item() <= max(l.bound for l in layers), t
        assert (bits(bh[:n].view(3, h, h, pitch)[..., width:]) == 0).all() and (bits(bl[:n].view(3, h, h, pitch)[..., width:]) == 0).all(), t
    assert (width, pitch) in ((256, 256), (528, 544))


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
def test_googlenet_end_to_end(engine, sd, golden_dir):
    """Logits lens (tests/logits_lens.py): all 1000 logits of every row against fp64, bound 4 d_L with d_L = the fp32 CPU loop's distance.  Measured on one MI355X: googlenet d_L 9.11e-06, engine 1.54e-05 (1.69)."""
    ref = Reference(googlenet_ref, sd)
    check_end_to_end(engine, ARCH, ref, e2e_rows(ref, googlenet_ref.E2E_CASES, golden_dir),
                     "%(arch)s: yardstick distance d = %(d).3e over the 28 rows -> end-to-end bound %(bound).1e")


def test_a_mask_row_scores_the_same_bits_wherever_it_sits(engine, golden_dir):
    check_position_independence(engine, *googlenet_ref.e2e_inputs(golden_dir, "felz"), (8, ((1, 0, (0,)), (37, 41, (0, 5, 36)), (700, 44, (3, 511, 512, 699)))))


# ------------------------------------------------------------------------------------------------
# API, profile and errors
# ------------------------------------------------------------------------------------------------
def test_api_on_a_googlenet_engine(engine, sd, golden_dir):
    check_api(engine, Reference(googlenet_ref, sd), *googlenet_ref.e2e_inputs(golden_dir, "felz"), heatmaps=1, table_step=None)


def test_profile_times_every_pool_launch(engine, dev):
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
    assert len(prof["per_clip_pool_ms"]) == 12 and all(ms > 0 for ms in prof["per_clip_pool_ms"])
    assert prof["launches"]["pool"] == 12 + 1 + 1           # the clipped pools, maxpool4 and the global average pool
    assert prof["launches"]["conv"] == len(eng.layers) == 58 and all(ms > 0 for ms in prof["per_conv_ms"])
    assert prof["launches"]["head"] == 1 and prof["launches"]["mask_apply_normalize"] == 1
    assert sum(prof["launches"].values()) == 74             # K0 + the 73 launches of a forward batch
    assert sum(prof["per_clip_pool_ms"]) < prof["ms"]["pool"]


def test_googlenet_error_paths(small_engine, mpx_lib, dev, sd):
    eng = small_engine
    with pytest.raises(ValueError):
        MaskedForwardEngine(ARCH, max_batch=2, device=0, stem="table")
    with pytest.raises(ValueError, match="transform_input"):
        MaskedForwardEngine(ARCH, max_batch=2, device=0, transform_input=True)
    z = torch.zeros(224, 224, dtype=torch.int32, device=dev)
    im = torch.zeros(224, 224, 3, dtype=torch.uint8, device=dev)
    on = torch.ones(1, 1, dtype=torch.uint8, device=dev)
    mean = (C.c_float * 3)(*scorer.MEAN)
    std = (C.c_float * 3)(*scorer.STD)
    assert eng._lib.mpx_stem_table_build(eng._h, ptr(im), None, ptr(z), 1, mean, std, None) == -2
    assert eng._lib.mpx_stem_table_apply(eng._h, ptr(on), 1, 1, 0, None) == -2
    buf = torch.zeros(64, dtype=torch.float16, device=dev)
    assert eng._lib.mpx_stem_conv_maxpool(eng._h, ptr(buf), ptr(buf), 1, None) == -2
    for bad in (8001, 8999):
        h = C.c_void_p()
        assert mpx_lib.mpx_create(bad, 2, 0, C.byref(h)) == -1 and not h.value
    # a slice layer takes no residual operand and no fp32 output
    names = [d.name.decode() for d in eng.layers]
    i = names.index("inception3a.branch1.conv")
    zz = torch.zeros(28 * 28 * 256 + TAIL, dtype=torch.float16, device=dev)
    f = torch.zeros(16, dtype=torch.float32, device=dev)
    assert eng._lib.mpx_conv_bn_act(eng._h, i, ptr(zz), ptr(zz), ptr(zz), ptr(zz), ptr(zz), ptr(zz), None, 1, None) == -1
    assert eng._lib.mpx_conv_bn_act(eng._h, i, ptr(zz), ptr(zz), None, None, ptr(zz), ptr(zz), ptr(f), 1, None) == -1
    # the pool entry: stride 1 or 2, pad 0 or 1, a pitch that is a multiple of 8, a map the window fits
    call = eng._lib.mpx_maxpool3x3_clip
    assert call(eng._h, ptr(zz), ptr(zz), ptr(zz), ptr(zz), 1, 14, 3, 0, 64, None) == -1       # stride 3
    assert call(eng._h, ptr(zz), ptr(zz), ptr(zz), ptr(zz), 1, 14, 0, 0, 64, None) == -1       # stride 0
    assert call(eng._h, ptr(zz), ptr(zz), ptr(zz), ptr(zz), 1, 14, 1, 2, 64, None) == -1       # pad 2
    assert call(eng._h, ptr(zz), ptr(zz), ptr(zz), ptr(zz), 1, 14, 1, -1, 64, None) == -1      # pad -1
    assert call(eng._h, ptr(zz), ptr(zz), ptr(zz), ptr(zz), 1, 14, 1, 1, 12, None) == -1       # pitch not a multiple of 8
    assert call(eng._h, ptr(zz), ptr(zz), ptr(zz), ptr(zz), 1, 14, 1, 1, 0, None) == -1
    assert call(eng._h, ptr(zz), ptr(zz), ptr(zz), ptr(zz), 1, 2, 2, 0, 64, None) == -1        # a 3x3 window does not fit an unpadded 2x2 map
    assert call(eng._h, ptr(zz), ptr(zz), ptr(zz), ptr(zz), 0, 14, 1, 1, 64, None) == -1       # B <= 0
    assert call(eng._h, None, ptr(zz), ptr(zz), ptr(zz), 1, 14, 1, 1, 64, None) == -1         # null planes
    assert call(eng._h, ptr(zz), ptr(zz), ptr(zz), None, 1, 14, 1, 1, 64, None) == -1
    assert call(eng._h, ptr(zz[4:]), ptr(zz), ptr(zz), ptr(zz), 1, 14, 1, 1, 64, None) == -1   # planes that are not 16-byte aligned
    fresh = MaskedForwardEngine(ARCH, max_batch=2, device=0)
    try:
        assert fresh._lib.mpx_weights_complete(fresh._h) == 0
        fresh.stage_masks(im, z, on, 0)
        labels = torch.zeros(1, dtype=torch.int32, device=dev)
        with pytest.raises(MpxError):
            fresh.forward(1, labels)                                        # no weights yet
        with pytest.raises((KeyError, ValueError)):
            fresh.load_state_dict(synth.make_state_dict("resnet18"))        # a ResNet state_dict: conv1.conv.weight is missing
        assert fresh._lib.mpx_weights_complete(fresh._h) == 0
        # torchvision's checkpoint carries the aux classifiers: accepted and ignored
        with_aux = dict(sd)
        with_aux["aux1.conv.conv.weight"] = torch.randn(128, 512, 1, 1)
        with_aux["aux2.fc2.bias"] = torch.randn(1000)
        fresh.load_state_dict(with_aux)
        assert fresh._lib.mpx_weights_complete(fresh._h) == 1
        score, pred = fresh.forward(1, labels)[:2]
        torch.cuda.synchronize()
        assert 0.0 <= float(score[0]) <= 1.0
        # eps: the default is googlenet's 1e-3 -- the same bits as passing it, other bits than BatchNorm2d's 1e-5
        fresh.load_state_dict(sd, eps=1e-3)
        s3 = float(fresh.forward(1, labels)[0][0])
        assert s3 == float(score[0])
        fresh.load_state_dict(sd, eps=1e-5)
        assert float(fresh.forward(1, labels)[0][0]) != s3
    finally:
        fresh.close()
