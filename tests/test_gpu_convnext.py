"""ConvNeXt-Tiny / -Small on the MI355X (pytest -m gpu), through the C-ABI as tests/test_gpu_efficientnet.py does: the topology, the
depthwise 7x7 + LayerNorm launch, the stand-alone and the pooled LayerNorm against fp64 under the per-element bounds of
tests/cnext_draws.py (behind fenced sentinel rows, at any position of a batch, on a capped grid), GELU in the MFMA epilogue and every other
distinct conv shape on every tile it accepts under the per-layer rule, the whole networks against the batch-1 fp32 CPU loop and the fp64
restatement (tests/convnext_ref.py), position independence of a mask row, the reference-named API, the profile and the error paths.

Bounds.  Kernels 1-3: tol = C_f 2^-22 B + 2^-24 per element (tests/cnext_draws.py has B, C_f and r_ref).  Per conv layer: 4e-6
sqrt(max(K, 4608) / 4608) of max(|want|, 1), the project's per-layer bound.  End to end: scores within SCORE_BOUND = 2e-5 of fp64 under
SCORE_TOL = 1e-4, every argmax equal, all logits within 4 d_L (tests/logits_lens.py).
Measured on one MI355X: DESIGN.md 22 has the figures; the tests print them on every run."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnext_draws as draws
import convnext_ref as ref
from gpu_common import accepted_tiles, dev, dev_view, FALLBACK, FencedPair, GENERIC, merge, ptr, SCORE_BOUND, SCORE_TOL, split  # noqa: F401  (dev is a fixture)
from net_harness import check_api, check_conv_layer, check_position_independence, Reference
from network_interpretation_imagenet_amd import _lib, synth
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine
from logits_lens import LogitsLens
from oracle import scorer

pytestmark = pytest.mark.gpu

EPS = 1e-6
@pytest.fixture(scope="module")
def sds():
    return {a: synth.make_state_dict(a) for a in ref.ARCHS}


@pytest.fixture(scope="module")
def engines(mpx_lib, dev, sds):
    """Small workspaces: everything that hands the kernels device pointers of its own, and the end-to-end rows."""
    es = {a: MaskedForwardEngine(a, max_batch=8, device=0).load_state_dict(sds[a]) for a in ref.ARCHS}
    yield es
    for e in es.values():
        e.close()


@pytest.fixture(scope="module")
def tiny(engines):
    return engines["convnext_tiny"]


# ------------------------------------------------------------------------------------------------
# topology
# ------------------------------------------------------------------------------------------------
def _expected_default_tile(d, act):
    """The unchanged default_tile rules, spelled out for the ConvNeXt shapes; a GELU layer's own default."""
    if act:
        return 7
    if d.ksize == 1 and d.stride == 1 and d.cout % 256 == 0 and d.cin % 64 == 0 and d.cout <= d.cin:
        return 9 if d.residual else 13              # stage 3's block.5, 3072 -> 768 with its residual
    if d.ksize == 1 and d.stride == 1 and d.cout > d.cin:
        return 7                                    # classifier.2
    return 2                                        # the stem, the 2x2 convs, the other block.5 layers


@pytest.mark.parametrize("arch,n_conv,n_dw", [("convnext_tiny", 41, 18), ("convnext_small", 77, 36)])
def test_convnext_topology_and_default_tiles(engines, arch, n_conv, n_dw):
    eng = engines[arch]
    convs, dws, lnorms = ref.topology(arch)
    assert (len(convs), len(dws), len(lnorms)) == (n_conv, n_dw, 5) == (len(eng.layers), len(eng.dwconvs), len(eng.lnorms))
    got = [(d.name.decode(), d.bn_name.decode(), d.cin, d.cout, d.ksize, d.stride, d.hin, d.hout, d.residual, a) for d, a in zip(eng.layers, eng.epilogue_acts)]
    assert got == convs and all(d.relu == 0 and d.pad == 0 for d in eng.layers)
    assert sum(eng.epilogue_acts) == n_dw
    for i, d in enumerate(eng.layers):
        a = C.c_int(-1)
        assert eng._lib.mpx_conv_consumer_act(eng._h, i, C.byref(a)) == 0 and a.value == 0      # the layer applies its activation itself
        assert d.cout_pad == -(-d.cout // 128) * 128
        assert d.k_packed == (128 if d.cin == 3 else d.ksize * d.ksize * d.cin)
        assert eng._lib.mpx_get_conv_tile(eng._h, i) == _expected_default_tile(d, eng.epilogue_acts[i]), d.name
        assert eng.groups[i] == 1
    shapes = []
    for k, d in enumerate(eng.dwconvs):
        v = C.c_int(), C.c_int(), C.c_int()
        assert eng._lib.mpx_dwconv_shape(eng._h, k, *[C.byref(x) for x in v]) == 0 and [x.value for x in v] == [7, 0, 0]
        ln, e = C.c_int(), C.c_float()
        assert eng._lib.mpx_dwconv_ln(eng._h, k, C.byref(ln), None, C.byref(e)) == 0 and ln.value == 1 and e.value == np.float32(EPS)
        assert d.pitch == d.channels and d.stride == 1 and d.clamp_in == 0
        shapes.append((d.name.decode(), d.bn_name.decode(), d.channels, d.hin))
    assert shapes == dws and set(eng.dw_ksizes) == {7} and set(eng.dw_ln) == {1}
    assert [(d.name.decode(), d.channels, d.hw) for d in eng.lnorms] == lnorms
    assert eng.flops_per_forward == 2.0 * ref.MACS[arch] == 2.0 * ref.macs(arch)
    geo = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert eng._lib.mpx_geometry(eng._h, *[C.byref(v) for v in geo]) == 0 and [v.value for v in geo] == [224, 3, 1000, 1000]
    assert eng.stem == "conv" and not eng.has_stem_table and eng._lib.mpx_weights_complete(eng._h) == 1
    assert eng._lib.mpx_num_bottleneck_tails(eng._h) == 0 and eng._lib.mpx_num_norms(eng._h) == 0 and eng._lib.mpx_num_se(eng._h) == 0


def test_convnext_default_max_batch_and_workspace(mpx_lib, dev):
    eng = MaskedForwardEngine("convnext_tiny", device=0)
    try:
        assert eng.max_batch == 512
        # per slot: three 56x56x384 split-fp16 buffers and the NHWC4 staging: 15.3 MB
        per_slot = 3 * 2 * 56 * 56 * 384 * 2 + 2 * 230 * 230 * 4 * 2
        w = sum(2 * d.cout_pad * d.k_packed * 2 for d in eng.layers)
        assert per_slot * 512 + w < eng.workspace_bytes < per_slot * 512 + w + (16 << 20)
        print("convnext_tiny: %.2f MB per slot, workspace %.2f GB at max_batch 512" % (per_slot / 1e6, eng.workspace_bytes / 1e9))
        assert eng._lib.mpx_weights_complete(eng._h) == 0
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------
# depthwise 7x7 + LayerNorm
# ------------------------------------------------------------------------------------------------
def _dw_case(c, hin, batch, dev):
    x = draws.planes((batch, hin, hin, c), seed=100 * c + hin)
    w, bias = draws.dw_params(c, seed=c + hin)
    gamma, beta = draws.ln_params(c, seed=7 * c + hin)
    return x, w, bias, gamma, beta


def _dw_run(eng, x, w, bias, gamma, beta, dev, max_blocks=0):
    batch, hin, _, c = x.shape
    xh, xl = split(x.to(dev))
    wt = w.reshape(c, 49).t().contiguous().to(dev)
    out = FencedPair(batch * hin * hin, c, dev)
    oh, ol = out.ptrs()
    vec = [t.contiguous().to(dev) for t in (bias, gamma, beta)]
    rc = eng._lib.mpx_dwconv7x7_ln(eng._h, ptr(xh), ptr(xl), ptr(wt), ptr(vec[0]), ptr(vec[1]), ptr(vec[2]), EPS, oh, ol, batch, hin, c, 7, 1, max_blocks, eng._stream())
    _lib.check(eng._h, rc, "mpx_dwconv7x7_ln")
    yh, yl = out.result()
    return yh.view(batch, hin, hin, c), yl.view(batch, hin, hin, c)


@pytest.mark.parametrize("c,hin,batch", draws.DW_CASES)
def test_dwconv7x7_ln_against_fp64(tiny, dev, c, hin, batch):
    x, w, bias, gamma, beta = _dw_case(c, hin, batch, dev)
    yh, yl = _dw_run(tiny, x, w, bias, gamma, beta, dev)
    v64, bv64 = draws.dw_v(x, w, bias, torch.float64)
    want, mag, var = draws.ln_want(v64, bv64, gamma, beta)
    assert var.min().item() >= draws.VAR_FLOOR
    worst = ((merge(yh, yl).cpu().double() - want).abs() / draws.tol(mag, draws.C_F["dw", c, hin])).max().item()
    print("dwconv7x7 + LayerNorm C %d %dx%d batch %d: worst err / bound %.3f (C_f %g)" % (c, hin, hin, batch, worst, draws.C_F["dw", c, hin]))
    assert worst <= 1.0
    if batch == 3:          # image 2 of the batch has the bits of the same image alone
        ah, al = _dw_run(tiny, x[2:3], w, bias, gamma, beta, dev)
        assert torch.equal(ah[0].view(torch.int16), yh[2].view(torch.int16)) and torch.equal(al[0].view(torch.int16), yl[2].view(torch.int16))
    if batch >= 2:          # a grid capped to fewer workgroups than units gives the same bits
        units = batch * hin * ((hin + 3) // 4)
        assert units > 256 // (c // 8)              # one workgroup holds 256 / (C / 8) units at a time: it strides over the rest
        ch, cl = _dw_run(tiny, x, w, bias, gamma, beta, dev, max_blocks=1)
        assert torch.equal(ch.view(torch.int16), yh.view(torch.int16)) and torch.equal(cl.view(torch.int16), yl.view(torch.int16))


def test_dwconv7x7_ln_with_engine_layer_parameters(tiny, dev, sds):
    """The device vectors mpx_load_dwconv_ln made for features.5.0.block.0 (384 channels on 14x14), and the kernel run with them."""
    eng, sd = tiny, sds["convnext_tiny"]
    k = [d.name.decode() for d in eng.dwconvs].index("features.5.0.block.0")
    d = eng.dwconvs[k]
    assert (d.channels, d.hin) == (384, 14)
    pw, ps, pt, pb = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert eng._lib.mpx_dwconv_params(eng._h, k, C.byref(pw), C.byref(ps), C.byref(pt)) == 0
    assert eng._lib.mpx_dwconv_ln(eng._h, k, None, C.byref(pb), None) == 0
    name, lnn = d.name.decode(), d.bn_name.decode()
    w = sd[name + ".weight"].reshape(384, 7, 7)
    assert torch.equal(dev_view(pw, 49 * 384, dev).view(49, 384), w.reshape(384, 49).t())
    assert torch.equal(dev_view(pb, 384, dev), sd[name + ".bias"]) and torch.equal(dev_view(ps, 384, dev), sd[lnn + ".weight"])
    assert torch.equal(dev_view(pt, 384, dev), sd[lnn + ".bias"])
    x = draws.planes((2, 14, 14, 384), seed=5)
    xh, xl = split(x.to(dev))
    out = FencedPair(2 * 14 * 14, 384, dev)
    oh, ol = out.ptrs()
    rc = eng._lib.mpx_dwconv7x7_ln(eng._h, ptr(xh), ptr(xl), pw, pb, ps, pt, EPS, oh, ol, 2, 14, 384, 7, 1, 0, eng._stream())
    _lib.check(eng._h, rc, "mpx_dwconv7x7_ln")
    yh, yl = out.result()
    v64, bv64 = draws.dw_v(x, w, sd[name + ".bias"], torch.float64)
    want, mag, var = draws.ln_want(v64, bv64, sd[lnn + ".weight"], sd[lnn + ".bias"])
    assert var.min().item() >= draws.VAR_FLOOR
    worst = ((merge(yh, yl).cpu().double().view(2, 14, 14, 384) - want).abs() / draws.tol(mag, 2.0)).max().item()
    print("engine layer %s: worst err / bound %.3f" % (name, worst))
    assert worst <= 1.0


def test_dwconv7x7_ln_refuses_bad_arguments(tiny, engines, dev, mpx_lib):
    eng = tiny
    z = torch.zeros(8192, dtype=torch.float16, device=dev)
    f = torch.zeros(4096, dtype=torch.float32, device=dev)
    a, b = ptr(z), ptr(f)
    call = eng._lib.mpx_dwconv7x7_ln
    assert call(eng._h, a, a, b, b, b, b, EPS, a, a, 1, 4, 16, 7, 1, 0, None) == 0
    torch.cuda.synchronize()
    assert call(eng._h, a, a, b, b, b, b, EPS, a, a, 1, 4, 12, 7, 1, 0, None) == -1          # C % 8
    assert call(eng._h, a, a, b, b, b, b, EPS, a, a, 1, 4, 2056, 7, 1, 0, None) == -1        # C above 2048
    assert call(eng._h, a, a, b, b, b, b, EPS, a, a, 1, 4, 16, 7, 2, 0, None) == -1          # stride 2
    for ksize in (3, 5):
        assert call(eng._h, a, a, b, b, b, b, EPS, a, a, 1, 4, 16, ksize, 1, 0, None) == -1  # a 3x3 / 5x5 layer handed to this entry
    assert b"mpx_dwconv_bn_act" in eng._lib.mpx_last_error(eng._h)
    assert eng._lib.mpx_dwconv_bn_act(eng._h, a, a, b, b, b, a, a, 1, 4, 16, 7, 1, 0, 0, None) == -1     # ... and a 7x7 layer to the other
    un = C.c_void_p(z.data_ptr() + 2)
    assert call(eng._h, un, a, b, b, b, b, EPS, a, a, 1, 4, 16, 7, 1, 0, None) == -1         # unaligned planes
    assert call(eng._h, a, a, b, b, b, b, EPS, a, un, 1, 4, 16, 7, 1, 0, None) == -1
    assert call(eng._h, a, a, C.c_void_p(f.data_ptr() + 4), b, b, b, EPS, a, a, 1, 4, 16, 7, 1, 0, None) == -1
    assert call(eng._h, None, a, b, b, b, b, EPS, a, a, 1, 4, 16, 7, 1, 0, None) == -1       # null planes
    assert call(eng._h, a, a, b, b, b, b, EPS, a, a, 0, 4, 16, 7, 1, 0, None) == -1          # empty batch
    assert call(eng._h, a, a, b, b, b, b, -1.0, a, a, 1, 4, 16, 7, 1, 0, None) == -1         # negative eps
    # the loaders: a LayerNorm layer refuses the BatchNorm loader and the other way round
    v = torch.ones(49 * 768)
    vp = C.c_void_p(v.data_ptr())
    assert eng._lib.mpx_load_dwconv(eng._h, 0, vp, vp, vp, vp, vp, 1e-5) == -1 and b"mpx_load_dwconv_ln" in eng._lib.mpx_last_error(eng._h)
    assert eng._lib.mpx_load_dwconv_ln(eng._h, 18, vp, vp, vp, vp, EPS) == -1 and eng._lib.mpx_load_dwconv_ln(eng._h, 0, vp, None, vp, vp, EPS) == -1
    r = MaskedForwardEngine("mobilenet_v2", max_batch=2, device=0)
    try:
        assert r._lib.mpx_load_dwconv_ln(r._h, 0, vp, vp, vp, vp, EPS) == -1
        ln = C.c_int(-1)
        assert r._lib.mpx_dwconv_ln(r._h, 0, C.byref(ln), None, None) == 0 and ln.value == 0
        assert r._lib.mpx_num_lnorms(r._h) == 0 and r.lnorms == [] and set(r.epilogue_acts) == {0}
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# stand-alone and pooled LayerNorm
# ------------------------------------------------------------------------------------------------
def _ln_run(eng, x, gamma, beta, dev, max_blocks=0):
    rows, c = x.shape
    xh, xl = split(x.to(dev))
    out = FencedPair(rows, c, dev)
    oh, ol = out.ptrs()
    g, b = gamma.contiguous().to(dev), beta.contiguous().to(dev)
    rc = eng._lib.mpx_layernorm_c(eng._h, ptr(xh), ptr(xl), ptr(g), ptr(b), EPS, oh, ol, rows, c, max_blocks, eng._stream())
    _lib.check(eng._h, rc, "mpx_layernorm_c")
    yh, yl = out.result()
    return yh.view(rows, c), yl.view(rows, c)


@pytest.mark.parametrize("rows,c", draws.LN_CASES)
def test_layernorm_c_against_fp64(tiny, dev, rows, c):
    x = draws.planes((rows, c), seed=10 * rows + c)
    gamma, beta = draws.ln_params(c, seed=rows + c)
    yh, yl = _ln_run(tiny, x, gamma, beta, dev)
    want, mag, var = draws.ln_want(x.double(), x.double().abs(), gamma, beta)
    assert var.min().item() >= draws.VAR_FLOOR
    worst = ((merge(yh, yl).cpu().double() - want).abs() / draws.tol(mag, draws.C_F["ln", rows, c])).max().item()
    print("LayerNorm %d rows x %d: worst err / bound %.3f (C_f %g)" % (rows, c, worst, draws.C_F["ln", rows, c]))
    assert worst <= 1.0
    if rows >= 50:          # a row has the same bits alone, and on a grid of two workgroups
        at = rows - 7
        ah, al = _ln_run(tiny, x[at:at + 1], gamma, beta, dev)
        assert torch.equal(ah[0].view(torch.int16), yh[at].view(torch.int16)) and torch.equal(al[0].view(torch.int16), yl[at].view(torch.int16))
        ch, cl = _ln_run(tiny, x, gamma, beta, dev, max_blocks=2)
        assert torch.equal(ch.view(torch.int16), yh.view(torch.int16)) and torch.equal(cl.view(torch.int16), yl.view(torch.int16))


@pytest.mark.parametrize("hw,c,batch", draws.POOL_CASES)
def test_global_avgpool_ln_against_fp64(tiny, dev, hw, c, batch):
    eng = tiny
    x = draws.planes((batch, hw, c), seed=hw + c)
    gamma, beta = draws.ln_params(c, seed=3 * hw + c)
    xh, xl = split(x.to(dev))
    out = FencedPair(batch, c, dev)
    oh, ol = out.ptrs()
    g, b = gamma.to(dev), beta.to(dev)
    rc = eng._lib.mpx_global_avgpool_ln(eng._h, ptr(xh), ptr(xl), ptr(g), ptr(b), EPS, oh, ol, batch, hw, c, eng._stream())
    _lib.check(eng._h, rc, "mpx_global_avgpool_ln")
    yh, yl = out.result()
    want, mag, var = draws.ln_want(x.double().mean(1), draws.pool_bv(x.double()), gamma, beta)
    assert var.min().item() >= draws.VAR_FLOOR
    worst = ((merge(yh, yl).cpu().double().view(batch, c) - want).abs() / draws.tol(mag, draws.C_F["pool", hw, c])).max().item()
    print("pooled LayerNorm hw %d x %d batch %d: worst err / bound %.3f (C_f %g)" % (hw, c, batch, worst, draws.C_F["pool", hw, c]))
    assert worst <= 1.0
    if batch == 2:          # the second image alone
        out1 = FencedPair(1, c, dev)
        o1h, o1l = out1.ptrs()
        rc = eng._lib.mpx_global_avgpool_ln(eng._h, ptr(xh[1:].contiguous()), ptr(xl[1:].contiguous()), ptr(g), ptr(b), EPS, o1h, o1l, 1, hw, c, eng._stream())
        _lib.check(eng._h, rc, "mpx_global_avgpool_ln")
        ah, al = out1.result()
        assert torch.equal(ah.view(torch.int16), yh[c:].view(torch.int16)) and torch.equal(al.view(torch.int16), yl[c:].view(torch.int16))
    call = eng._lib.mpx_global_avgpool_ln
    assert call(eng._h, ptr(xh), ptr(xl), ptr(g), ptr(b), EPS, oh, ol, batch, hw, c + 4, None) == -1
    assert call(eng._h, ptr(xh), ptr(xl), None, ptr(b), EPS, oh, ol, batch, hw, c, None) == -1
    assert eng._lib.mpx_layernorm_c(eng._h, ptr(xh), ptr(xl), ptr(g), ptr(b), EPS, oh, ol, 0, c, 0, None) == -1
    assert eng._lib.mpx_layernorm_c(eng._h, ptr(xh), ptr(xl), ptr(g), ptr(b), EPS, oh, ol, 1, 12, 0, None) == -1


# ------------------------------------------------------------------------------------------------
# the conv layers: GELU in the epilogue, block.5 with its residual, the stem, the 2x2 convs
# ------------------------------------------------------------------------------------------------
def _ref_layer(sd, d, act, x64, r64, shift=0.0):
    """fp64 conv + bias (+ GELU) (x layer scale + residual) of the same inputs."""
    name, bn = d.name.decode(), d.bn_name.decode()
    w = sd[name + ".weight"].double().reshape(d.cout, d.cin, d.ksize, d.ksize)
    y = F.conv2d(x64, w, sd[name + ".bias"].double() + shift, d.stride)
    if act:
        y = F.gelu(y)
    if bn:
        y = y * sd[bn].double().reshape(1, d.cout, 1, 1)
    return y + r64 if r64 is not None else y


def _check(eng, sd, i, batch, tile=-1, shift=0.0):
    """-> (kernel mask, want); the fp64 reference is computed on the host."""
    d, act = eng.layers[i], eng.epilogue_acts[i]
    fields = "%d->%d k%d h%d K %d res %d act %d " % (d.cin, d.cout, d.ksize, d.hin, d.k_packed, d.residual, act)

    def ref_layer(d, x64, r64):
        return _ref_layer(sd, d, act, x64.cpu(), None if r64 is None else r64.cpu(), shift)
    return check_conv_layer(eng, i, batch, ref_layer, tile, clamp=False, fenced=True, fields=fields)


def test_gelu_epilogue_on_every_generic_tile_and_the_refusals(tiny, sds):
    """block.3 of each stage (96 -> 384 on 56x56, 192 -> 768 on 28x28, 384 -> 1536 on 14x14, 768 -> 3072 on 7x7) at batches 1 and 3 on
    every tile it accepts; each special tile is refused with the reason."""
    eng, sd = tiny, sds["convnext_tiny"]
    names = [d.name.decode() for d in eng.layers]
    for s in (1, 3, 5, 7):
        i = names.index("features.%d.0.block.3" % s)
        assert eng.epilogue_acts[i] == 1
        accepted = accepted_tiles(eng, i)
        assert set(accepted) == GENERIC, (names[i], accepted)
        for t in (6, 9, 10, 12, 13, 14):
            assert eng._lib.mpx_set_conv_tile(eng._h, i, t) == -1
            msg = eng._lib.mpx_last_error(eng._h).decode()
            assert "GELU" in msg and "generic" in msg and names[i] in msg, msg
        assert eng._lib.mpx_set_conv_tile(eng._h, i, 16) == -1
        eng._lib.mpx_set_conv_tile(eng._h, i, -1)
        assert eng._lib.mpx_get_conv_tile(eng._h, i) == 7
        for t in accepted:
            for batch in (1, 3):
                ran, want = _check(eng, sd, i, batch, tile=t)
                assert ran == 1 << t
                assert (want < -0.1).any() and want.min().item() > -0.1701 and (want > 3.0).any()       # the negative lobe and the linear part


def test_gelu_epilogue_in_the_negative_lobe(tiny, sds, dev):
    """features.1.0.block.3 with its bias moved down by 3 standard deviations: most outputs sit in GELU's negative lobe."""
    eng, sd = tiny, dict(sds["convnext_tiny"])
    name = "features.1.0.block.3"
    i = [d.name.decode() for d in eng.layers].index(name)
    shift = -4.5
    sd[name + ".bias"] = sds["convnext_tiny"][name + ".bias"] + shift
    eng.load_state_dict(sd, only=[name])
    try:
        for t in (2, 7):
            ran, want = _check(eng, sd, i, 3, tile=t)
            frac = (want < 0).double().mean().item()
            print("negative lobe: %.3f of the outputs below zero, min %.4f" % (frac, want.min().item()))
            assert frac > 0.6 and ran == 1 << t
    finally:
        eng.load_state_dict(sds["convnext_tiny"], only=[name])


def test_every_other_distinct_conv_shape_on_every_accepted_tile(tiny, sds):
    """block.5 with its residual and layer scale in every stage, the stem (4x4 stride 4 on the NHWC4 staging, pad 0), the three 2x2 stride-2
    convs and classifier.2, on every tile each accepts, batch 2.  Stage 3's block.5 (3072 -> 768 on 7x7) is the one layer the 256-row tiles
    take: under one round of tiles they hand the work to the small-tile kernel that sums in the same order."""
    eng, sd = tiny, sds["convnext_tiny"]
    seen, count = set(), 0
    for i, d in enumerate(eng.layers):
        key = (d.cin, d.cout, d.ksize, d.hin, d.residual)
        if key in seen or eng.epilogue_acts[i]:
            continue
        seen.add(key)
        accepted = accepted_tiles(eng, i)
        assert eng._lib.mpx_get_conv_tile(eng._h, i) in accepted and GENERIC <= set(accepted), (d.name, accepted)
        if not (d.ksize == 1 and d.cout % 256 == 0 and i != len(eng.layers) - 1):
            assert set(accepted) == GENERIC, (d.name, accepted)
        else:
            assert set(accepted) == GENERIC | {9, 10}, (d.name, accepted)           # a residual operand keeps tile 13 away, K = 3072 tile 14
        for t in accepted:
            ran, want = _check(eng, sd, i, 2, tile=t)
            assert ran & ((1 << t) | (1 << FALLBACK.get(t, t))), (d.name, t, ran)
            if d.residual:
                assert (want < -0.5).any()              # nothing behind the add
        count += 1
    print("distinct conv shapes checked: %d" % count)
    assert count == 1 + 4 + 3 + 1


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ref.ARCHS)
def test_convnext_end_to_end(engines, sds, golden_dir, arch):
    """Engine against the fp64 scorer on both committed segment fixtures: scores within SCORE_BOUND, every argmax equal, all logits through
    the lens (engine <= 4 d_L).  Measured on one MI355X, max |d| of a score, engine vs fp64 against the yardstick (fp32 CPU loop vs fp64),
    felzenszwalb / grid: convnext_tiny 3.1e-07 / 9.5e-07 against 2.0e-07 / 6.1e-07, logits d_L 2.76e-06, engine 6.48e-06 (2.35); convnext_small
    1.4e-06 / 3.0e-07 against 7.9e-07 / 5.2e-07, logits d_L 4.78e-06, engine 6.16e-06 (1.29)."""
    eng, sd = engines[arch], sds[arch]
    lens = LogitsLens(arch)
    for kind, m, seed in ref.E2E_CASES:
        img, seg = ref.e2e_inputs(golden_dir, kind)
        x = scorer.to_tensor_normalize(img)
        S = len(np.unique(seg))
        onoff = synth.random_onoff(m, S, seed=seed)
        with torch.no_grad():
            label = int(ref.forward(ref.cast(sd, torch.float32), x[None]).argmax(1)[0])
        _o, score, pred, logits = eng.score_masks(img, seg, onoff, label, return_logits=True)
        ref_score, ref_pred, ref_logits = ref.score_masks_reference_loop(sd, x, seg, onoff, label, return_logits=True)
        s64, logits64 = ref.score_masks_fp64(sd, x, seg, onoff, label)
        lens.add(kind, logits, ref_logits, logits64)
        top2 = np.sort(logits64, axis=1)[:, -2:]
        gap = top2[:, 1] - top2[:, 0]
        err_engine = float(np.abs(score.astype(np.float64) - s64).max())
        err_cpu = float(np.abs(ref_score.astype(np.float64) - s64).max())
        print("%s %s: %d masks, S %d, label %d, scores %.4f..%.4f; max|d| engine vs fp64 %.3e, fp32 CPU loop vs fp64 %.3e, smallest fp64 logit gap %.4f"
              % (arch, kind, m, S, label, s64.min(), s64.max(), err_engine, err_cpu, gap.min()))
        peaks = F.softmax(torch.from_numpy(logits64), 1).max(1)[0].numpy()
        assert gap.min() >= 1e-3 and peaks.min() >= 0.05 and peaks.max() <= 0.95      # tests/test_convnext_cpu.py holds the weights to it
        assert err_engine <= SCORE_BOUND <= SCORE_TOL
        assert (pred == logits64.argmax(1)).all() and (pred == ref_pred).all()
        p_label, _ = eng.predict(img)
        assert p_label == label
    lens.check()


def test_a_mask_row_scores_the_same_bits_wherever_it_sits(tiny, golden_dir):
    check_position_independence(tiny, *ref.e2e_inputs(golden_dir, "felz"), (3, ((1, 0, (0,)), (8, 41, (0, 5, 7)), (13, 44, (3, 8, 12)))))


def test_api_on_a_convnext_engine(tiny, sds, golden_dir):
    check_api(tiny, Reference(ref, sds["convnext_tiny"]), *ref.e2e_inputs(golden_dir, "grid"),
              rows=4, same_pred=True, heatmaps=0, predict=False, table_step=None, validate=None)


def test_profile_lists_the_layernorm_launches(tiny, dev):
    eng = tiny
    img = torch.from_numpy(synth.make_images(1, kind="noise")[0]).to(dev)
    seg = torch.from_numpy(synth.grid_segments()).to(dev)
    onoff = torch.from_numpy(synth.random_onoff(4, 196)).to(dev)
    labels = torch.zeros(4, dtype=torch.int32, device=dev)
    eng.profile(True)
    eng.stage_masks(img, seg, onoff, 0)
    eng.forward(4, labels)
    eng.profile(False)
    prof = eng.collect_profile()
    assert len(prof["per_dw_ms"]) == 18 and all(ms > 0 for ms in prof["per_dw_ms"])
    assert len(prof["per_lnorm_ms"]) == 5 and all(ms > 0 for ms in prof["per_lnorm_ms"])
    assert prof["per_norm_ms"] == [] and prof["per_se_gate_ms"] == [] and prof["per_shuffle_ms"] == []
    assert prof["launches"]["pool"] == 18 + 5 and prof["launches"]["conv"] == 41 and prof["launches"]["head"] == 1     # 65 launches with K0's


def test_convnext_error_paths(tiny, mpx_lib, dev, sds):
    eng = tiny
    with pytest.raises(ValueError):
        MaskedForwardEngine("convnext_tiny", max_batch=2, device=0, stem="table")
    z = torch.zeros(224, 224, dtype=torch.int32, device=dev)
    im = torch.zeros(224, 224, 3, dtype=torch.uint8, device=dev)
    on = torch.ones(1, 1, dtype=torch.uint8, device=dev)
    mean = (C.c_float * 3)(*scorer.MEAN)
    std = (C.c_float * 3)(*scorer.STD)
    assert eng._lib.mpx_stem_table_build(eng._h, ptr(im), None, ptr(z), 1, mean, std, None) == -2
    assert eng._lib.mpx_stem_table_apply(eng._h, ptr(on), 1, 1, 0, None) == -2
    buf = torch.zeros(64, dtype=torch.float16, device=dev)
    assert eng._lib.mpx_stem_conv_maxpool(eng._h, ptr(buf), ptr(buf), 1, None) == -2
    for bad in (12000, 12003, 12999):
        h = C.c_void_p()
        assert mpx_lib.mpx_create(bad, 2, 0, C.byref(h)) == -1 and not h.value
    ld = _lib.LnormDesc()
    assert eng._lib.mpx_lnorm_info(eng._h, 5, C.byref(ld)) == -1 and eng._lib.mpx_lnorm_info(eng._h, -1, C.byref(ld)) == -1
    a = C.c_int()
    assert eng._lib.mpx_conv_epilogue_act(eng._h, 41, C.byref(a)) == -1 and eng._lib.mpx_dwconv_ln(eng._h, 18, None, None, None) == -1
    v = torch.ones(1024)
    vp = C.c_void_p(v.data_ptr())
    assert eng._lib.mpx_load_lnorm(eng._h, 5, vp, vp, EPS) == -1 and eng._lib.mpx_load_lnorm(eng._h, 0, vp, None, EPS) == -1
    fresh = MaskedForwardEngine("convnext_tiny", max_batch=2, device=0)
    try:
        sd = sds["convnext_tiny"]
        fresh.load_state_dict(sd, only=[d.name.decode() for d in fresh.layers] + [d.name.decode() for d in fresh.dwconvs])   # no LayerNorm
        assert fresh._lib.mpx_weights_complete(fresh._h) == 0
        fresh.stage_masks(im, z, on, 0)
        labels = torch.zeros(1, dtype=torch.int32, device=dev)
        score = torch.zeros(1, device=dev)
        pred = torch.zeros(1, dtype=torch.int32, device=dev)
        assert fresh._lib.mpx_forward(fresh._h, ptr(labels), ptr(score), ptr(pred), None, 1, None) == -2       # missing LayerNorms
        with pytest.raises((KeyError, ValueError)):     # another family's state_dict: features.0.0.weight has another shape
            fresh.load_state_dict(synth.make_state_dict("mobilenet_v2"))
        for k, d in enumerate(fresh.lnorms):
            n = d.name.decode()
            assert fresh._lib.mpx_load_lnorm(fresh._h, k, C.c_void_p(sd[n + ".weight"].data_ptr()), C.c_void_p(sd[n + ".bias"].data_ptr()), EPS) == 0
        assert fresh._lib.mpx_weights_complete(fresh._h) == 1
        assert fresh._lib.mpx_forward(fresh._h, ptr(labels), ptr(score), ptr(pred), None, 1, None) == 0
        torch.cuda.synchronize()
    finally:
        fresh.close()
