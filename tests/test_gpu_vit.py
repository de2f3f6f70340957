"""ViT-B/16 / ViT-B/32 on the MI355X (pytest -m gpu), through the C-ABI as tests/test_gpu_convnext.py does: the topology and the token layers'
descriptors, the attention kernel against fp64 under the per-element bounds of tests/attn_draws.py (behind fenced sentinel rows, at any
position of a batch, on a capped grid, with other heads' and other images' data changed), the token assembly and the LayerNorm of strided
rows likewise, both patchify stems and the four token-layer shapes on every tile each accepts under the per-layer rule, the whole networks
against the batch-1 fp32 CPU loop and the fp64 restatement (tests/vit_ref.py), position independence of a mask row, the reference-named API,
the profile and the refusals.

Bounds.  Attention and token assembly: tol = C_f 2^-22 B + 2^-24 per element (tests/attn_draws.py has B, C_f and r_ref).  LayerNorm of strided
rows: DESIGN.md 22's bound (tests/cnext_draws.py), and the bits of mpx_layernorm_c on the gathered rows.  Per conv layer: 4e-6 sqrt(max(K,
4608) / 4608) of max(|want|, 1), the project's per-layer bound.  End to end: scores within SCORE_BOUND = 2e-5 of fp64 under SCORE_TOL = 1e-4,
printed next to the yardstick (fp32 CPU loop against fp64), every argmax equal, all logits within 4 d_L (tests/logits_lens.py).
Measured on one MI355X: DESIGN.md 23 has the figures; the tests print them on every run."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_draws as draws
import cnext_draws
import vit_ref as ref
from gpu_common import accepted_tiles, bits, dev, dev_view, FALLBACK, FencedPair, GENERIC, LAYER_TOL, merge, ptr, SCORE_BOUND, SCORE_TOL, split  # noqa: F401  (dev is a fixture)
from net_harness import assert_layer_close, check_api, check_position_independence, conv_tile, Reference, stage_stem_input
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
    es = {a: MaskedForwardEngine(a, max_batch=8, device=0).load_state_dict(sds[a]) for a in ref.ARCHS}
    yield es
    for e in es.values():
        e.close()


@pytest.fixture(scope="module")
def b16(engines):
    return engines["vit_b_16"]


# ------------------------------------------------------------------------------------------------
# topology
# ------------------------------------------------------------------------------------------------
def _expected_default_tile(name):
    """The unchanged default_tile rules, spelled out for the ViT shapes; a GELU layer's own default."""
    if name.endswith("in_proj"):
        return 10                       # 768 -> 2304: expanding, cout % 256 == 0, K >= 128
    if name.endswith("out_proj") or name.endswith("mlp.3"):
        return 9                        # reducing / square with cout % 256 == 0 and a residual operand
    if name.endswith("mlp.0") or name == "heads.head":
        return 7                        # GELU in the epilogue: the generic tiles; the logit layer: expanding, cout % 256 != 0
    return 2                            # the stem


@pytest.mark.parametrize("arch", ref.ARCHS)
def test_vit_topology_descriptors_and_rows(engines, arch):
    eng = engines[arch]
    p, t = ref.PATCH[arch], ref.TOKENS[arch]
    convs, lnorms, attns = ref.topology(arch)
    assert (len(eng.layers), len(eng.lnorms), len(eng.attns)) == (50, 25, 12)
    for i, (d, c) in enumerate(zip(eng.layers, convs)):
        name, cin, cout, k, rows, token, residual, act = c
        assert (d.name.decode(), d.bn_name.decode(), d.cin, d.cout, d.ksize, d.stride, d.pad, d.relu, d.residual) == (name, "", cin, cout, k, k, 0, 0, residual)
        assert eng.epilogue_acts[i] == act and eng.groups[i] == 1
        # a token layer is no square map: hin = hout = 0 and mpx_conv_rows has the rows; the stem is a 14 x 14 / 7 x 7 map, the head one row
        assert eng.conv_rows[i] == (t if token else 0)
        assert (d.hin, d.hout) == ((0, 0) if token else ((224, 224 // p) if i == 0 else (1, 1)))
        assert d.cout_pad == -(-d.cout // 128) * 128 and d.k_packed == (p * 4 * p if i == 0 else cin)
        assert eng._lib.mpx_get_conv_tile(eng._h, i) == _expected_default_tile(name), name
    assert [(d.name.decode(), d.channels, d.hw) for d in eng.lnorms] == [(n, 768, 0) for n in lnorms]
    assert [(d.name.decode(), d.tokens, d.heads, d.head_dim) for d in eng.attns] == attns
    assert eng.flops_per_forward == 2.0 * ref.MACS[arch] == 2.0 * ref.macs(arch)
    geo = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert eng._lib.mpx_geometry(eng._h, *[C.byref(v) for v in geo]) == 0 and [v.value for v in geo] == [224, 3, 1000, 1000]
    assert eng.stem == "conv" and not eng.has_stem_table and eng._lib.mpx_weights_complete(eng._h) == 1
    assert eng._lib.mpx_num_dwconvs(eng._h) == 0 and eng._lib.mpx_num_norms(eng._h) == 0 and eng._lib.mpx_num_bottleneck_tails(eng._h) == 0
    r = C.c_int(-1)
    assert eng._lib.mpx_conv_rows(eng._h, 50, C.byref(r)) == -1 and eng._lib.mpx_conv_rows(eng._h, -1, C.byref(r)) == -1


def test_rows_and_attention_lists_are_empty_on_other_engines(mpx_lib, dev):
    r = MaskedForwardEngine("resnet18", max_batch=2, device=0)
    try:
        assert set(r.conv_rows) == {0} and r.attns == [] and r._lib.mpx_num_attn(r._h) == 0
        tk, wd, a, b = C.c_int(-1), C.c_int(-1), C.c_void_p(1), C.c_void_p(1)
        assert r._lib.mpx_token_params(r._h, C.byref(a), C.byref(b), C.byref(tk), C.byref(wd)) == 0 and (tk.value, wd.value, a.value, b.value) == (0, 0, None, None)
    finally:
        r.close()


@pytest.mark.parametrize("arch,per_slot_mb", [("vit_b_16", 6.29), ("vit_b_32", 2.23)])
def test_vit_default_max_batch_and_workspace(mpx_lib, dev, arch, per_slot_mb):
    eng = MaskedForwardEngine(arch, device=0)
    try:
        assert eng.max_batch == 512
        t = ref.TOKENS[arch]
        per_slot = 2 * 2 * t * (768 + 768 + 2304 + 3072) + 2 * 230 * 230 * 4 * 2          # X, T1, QKV, H in both planes, and the NHWC4 staging
        w = sum(2 * d.cout_pad * d.k_packed * 2 for d in eng.layers)
        assert abs(per_slot / 1e6 - per_slot_mb) < 0.01
        assert per_slot * 512 + w < eng.workspace_bytes < per_slot * 512 + w + (16 << 20)
        print("%s: %.2f MB per slot, workspace %.2f GB at max_batch 512" % (arch, per_slot / 1e6, eng.workspace_bytes / 1e9))
        assert eng._lib.mpx_weights_complete(eng._h) == 0
    finally:
        eng.close()


def test_token_parameters_are_uploaded_as_they_are(b16, sds, dev):
    eng, sd = b16, sds["vit_b_16"]
    pc, pp, tk, wd = C.c_void_p(), C.c_void_p(), C.c_int(), C.c_int()
    assert eng._lib.mpx_token_params(eng._h, C.byref(pc), C.byref(pp), C.byref(tk), C.byref(wd)) == 0 and (tk.value, wd.value) == (197, 768)
    assert torch.equal(dev_view(pc, 768, dev), sd["class_token"].flatten())
    assert torch.equal(dev_view(pp, 197 * 768, dev), sd["encoder.pos_embedding"].flatten())


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
def _attn_run(eng, x, heads, dev, max_blocks=0):
    """x: f32 ndarray [B][T][3 D] of valid pairs -> (hi, lo) of the output planes [B][T][D], behind fences."""
    b, t, _ = x.shape
    d = heads * 64
    xh, xl = split(torch.from_numpy(x).to(dev))
    out = FencedPair(b * t, d, dev)
    oh, ol = out.ptrs()
    rc = eng._lib.mpx_attention(eng._h, ptr(xh), ptr(xl), oh, ol, b, t, heads, max_blocks, eng._stream())
    _lib.check(eng._h, rc, "mpx_attention")
    yh, yl = out.result()
    return yh.view(b, t, d).cpu(), yl.view(b, t, d).cpu()


_ATTN = {}


def _attn_case(eng, t, heads, b, dev):
    """The draw, its fp64 yardstick and the kernel's output, computed once per shape and shared by the tests below."""
    key = (t, heads, b)
    if key not in _ATTN:
        x = draws.qkv_planes(b, t, heads, seed=1000 * t + heads)
        want, mag = draws.attn_want(x, heads)
        _ATTN[key] = (x, want, mag) + _attn_run(eng, x, heads, dev)
    return _ATTN[key]


@pytest.mark.parametrize("t,heads,b", draws.ATTN_CASES)
def test_attention_against_fp64(b16, dev, t, heads, b):
    x, want, mag, yh, yl = _attn_case(b16, t, heads, b, dev)
    c_f = draws.C_F["attn", t, heads]
    got = merge(yh, yl).double().numpy()
    worst = (np.abs(got - want) / draws.tol(mag, c_f)).max()
    print("attention T %d heads %d batch %d: worst err / bound %.3f (C_f %g), max |err| %.3e" % (t, heads, b, worst, c_f, np.abs(got - want).max()))
    assert worst <= 1.0
    # every image alone, behind a fence that starts right after its row T - 1: the same bits -- rows >= T of the last query block are not
    # written, and an image's rows depend on neither the batch nor its position in it
    for n in range(b):
        ah, al = _attn_run(b16, x[n:n + 1], heads, dev)
        assert torch.equal(bits(ah[0]), bits(yh[n])) and torch.equal(bits(al[0]), bits(yl[n])), (t, heads, n)


@pytest.mark.parametrize("t,heads,b", [(17, 2, 3), (50, 12, 3), (197, 12, 1)])
def test_attention_bits_do_not_depend_on_the_grid(b16, dev, t, heads, b):
    x, _want, _mag, yh, yl = _attn_case(b16, t, heads, b, dev)
    assert b * heads > 2                    # more units than workgroups: each strides over several (image, head) units
    for cap in (1, 2):
        ch, cl = _attn_run(b16, x, heads, dev, max_blocks=cap)
        assert torch.equal(bits(ch), bits(yh)) and torch.equal(bits(cl), bits(yl)), cap


def test_attention_reads_its_own_head_and_image_alone(b16, dev):
    """Changing the K / V (and Q) data of another head, or of another image, changes nothing: T = 50, 2 heads, 3 images."""
    t, heads, b = 50, 2, 3
    x, _want, _mag, yh, yl = _attn_case(b16, t, heads, b, dev)
    d = heads * 64
    other = draws.qkv_planes(b, t, heads, seed=99)
    y = x.copy()
    for part in range(3):                   # head 1's Q, K and V of every image
        y[:, :, part * d + 64:part * d + 128] = other[:, :, part * d + 64:part * d + 128]
    ah, al = _attn_run(b16, y, heads, dev)
    assert torch.equal(bits(ah[..., :64]), bits(yh[..., :64])) and torch.equal(bits(al[..., :64]), bits(yl[..., :64]))
    assert not torch.equal(bits(ah[..., 64:]), bits(yh[..., 64:]))
    z = x.copy()
    z[0], z[2] = other[0], other[2]         # the images around image 1
    ah, al = _attn_run(b16, z, heads, dev)
    assert torch.equal(bits(ah[1]), bits(yh[1])) and torch.equal(bits(al[1]), bits(yl[1])) and not torch.equal(bits(ah[0]), bits(yh[0]))


@pytest.mark.parametrize("t", [17, 50])
def test_a_row_of_equal_logits_returns_the_mean_of_v(b16, dev, t):
    """A query row of exact zeros: every logit is 0, every weight expf(0) = 1, the sum T, and the output the kernel's fixed-order mean of V."""
    heads = 2
    x = draws.qkv_planes(1, t, heads, seed=7 * t)
    x[0, 3, :heads * 64] = 0.0
    yh, yl = _attn_run(b16, x, heads, dev)
    _q, _k, v = draws.heads_of(x, heads)
    mean = draws.merge(v.astype(np.float64).mean(2, keepdims=True))[0, 0]
    mag = draws.merge(np.abs(v.astype(np.float64)).mean(2, keepdims=True))[0, 0]
    got = merge(yh, yl).double().numpy()[0, 3]
    worst = (np.abs(got - mean) / draws.tol(mag, draws.C_F["attn", t, heads])).max()
    print("equal logits, T %d: worst err / bound %.3f" % (t, worst))
    assert worst <= 1.0


def test_attention_refusals(b16, engines, dev):
    eng = b16
    z = torch.zeros(1 << 16, dtype=torch.float16, device=dev)
    a = ptr(z)
    call = eng._lib.mpx_attention
    assert call(eng._h, a, a, a, a, 1, 4, 1, 0, None) == 0
    torch.cuda.synchronize()
    assert call(eng._h, a, a, a, a, 1, 0, 1, 0, None) == -1 and b"T = 0" in eng._lib.mpx_last_error(eng._h)
    assert call(eng._h, a, a, a, a, 1, 513, 1, 0, None) == -1
    assert call(eng._h, a, a, a, a, 1, 4, 0, 0, None) == -1 and b"heads * 64" in eng._lib.mpx_last_error(eng._h)
    assert call(eng._h, a, a, a, a, 0, 4, 1, 0, None) == -1
    un = C.c_void_p(z.data_ptr() + 2)
    for args in ((un, a, a, a), (a, un, a, a), (a, a, un, a), (a, a, a, un)):
        assert call(eng._h, *args, 1, 4, 1, 0, None) == -1 and b"aligned" in eng._lib.mpx_last_error(eng._h)
    assert call(eng._h, None, a, a, a, 1, 4, 1, 0, None) == -1
    r = MaskedForwardEngine("resnet18", max_batch=2, device=0)
    try:
        f = torch.zeros(4096, dtype=torch.float32, device=dev)
        assert r._lib.mpx_tokens_assemble(r._h, a, a, ptr(f), ptr(f), a, a, 1, 4, 64, 0, None) == -2 and b"ViT" in r._lib.mpx_last_error(r._h)
        assert r._lib.mpx_load_tokens(r._h, ptr(f.cpu()), ptr(f.cpu())) == -2
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# token assembly, LayerNorm of strided rows
# ------------------------------------------------------------------------------------------------
def _tok_run(eng, x, cls, pos, dev, max_blocks=0):
    b, t, d = x.shape[0], pos.shape[0], pos.shape[1]
    xh, xl = split(torch.from_numpy(np.ascontiguousarray(x)).to(dev)) if t > 1 else (torch.zeros(8, dtype=torch.float16, device=dev),) * 2
    out = FencedPair(b * t, d, dev)
    oh, ol = out.ptrs()
    c, p = torch.from_numpy(cls).to(dev), torch.from_numpy(pos).to(dev)
    rc = eng._lib.mpx_tokens_assemble(eng._h, ptr(xh), ptr(xl), ptr(c), ptr(p), oh, ol, b, t, d, max_blocks, eng._stream())
    _lib.check(eng._h, rc, "mpx_tokens_assemble")
    yh, yl = out.result()
    return yh.view(b, t, d).cpu(), yl.view(b, t, d).cpu()


@pytest.mark.parametrize("b,t,d", draws.TOK_CASES)
def test_tokens_assemble_against_fp64(b16, dev, b, t, d):
    x, cls, pos = draws.tok_draw(b, t, d, seed=100 * t + d)
    yh, yl = _tok_run(b16, x, cls, pos, dev)
    want, mag = draws.tok_want(x, cls, pos)
    got = merge(yh, yl).double().numpy()
    worst = (np.abs(got - want) / draws.tol(mag, draws.C_F["tok", b, t, d])).max()
    print("token assembly batch %d T %d D %d: worst err / bound %.3f" % (b, t, d, worst))
    assert worst <= 1.0
    assert np.array_equal(got, draws.emulate_tokens(x, cls, pos).astype(np.float64))        # one add and the split: the emulation's very bits
    if b == 3:              # image 2 alone, and a grid of one workgroup
        ah, al = _tok_run(b16, x[2:3], cls, pos, dev)
        assert torch.equal(bits(ah[0]), bits(yh[2])) and torch.equal(bits(al[0]), bits(yl[2]))
        ch, cl = _tok_run(b16, x, cls, pos, dev, max_blocks=1)
        assert torch.equal(bits(ch), bits(yh)) and torch.equal(bits(cl), bits(yl))


def test_tokens_assemble_refusals(b16, dev):
    eng = b16
    z = torch.zeros(4096, dtype=torch.float16, device=dev)
    f = torch.zeros(4096, dtype=torch.float32, device=dev)
    a, q = ptr(z), ptr(f)
    call = eng._lib.mpx_tokens_assemble
    assert call(eng._h, a, a, q, q, a, a, 1, 4, 64, 0, None) == 0
    torch.cuda.synchronize()
    assert call(eng._h, a, a, q, q, a, a, 1, 0, 64, 0, None) == -1 and b"T = 0" in eng._lib.mpx_last_error(eng._h)
    assert call(eng._h, a, a, q, q, a, a, 1, 4, 60, 0, None) == -1
    assert call(eng._h, a, a, q, q, a, a, 0, 4, 64, 0, None) == -1
    assert call(eng._h, C.c_void_p(z.data_ptr() + 2), a, q, q, a, a, 1, 4, 64, 0, None) == -1 and b"aligned" in eng._lib.mpx_last_error(eng._h)
    assert call(eng._h, a, a, C.c_void_p(f.data_ptr() + 4), q, a, a, 1, 4, 64, 0, None) == -1
    assert call(eng._h, a, a, None, q, a, a, 1, 4, 64, 0, None) == -1


@pytest.mark.parametrize("rows,stride,c", [(3, 50, 768), (5, 197, 768), (7, 3, 96)])
def test_layernorm_rows_against_fp64_and_layernorm_c(b16, dev, rows, stride, c):
    eng = b16
    x = cnext_draws.planes((rows * stride, c), seed=10 * rows + c)
    gamma, beta = cnext_draws.ln_params(c, seed=rows + c)
    xh, xl = split(x.to(dev))
    g, b = gamma.to(dev), beta.to(dev)

    def run(n, max_blocks=0, at=0):
        out = FencedPair(n, c, dev)
        oh, ol = out.ptrs()
        ih, il = C.c_void_p(xh.data_ptr() + at * stride * c * 2), C.c_void_p(xl.data_ptr() + at * stride * c * 2)
        rc = eng._lib.mpx_layernorm_rows(eng._h, ih, il, ptr(g), ptr(b), EPS, oh, ol, n, stride, c, max_blocks, eng._stream())
        _lib.check(eng._h, rc, "mpx_layernorm_rows")
        yh, yl = out.result()
        return yh.view(n, c), yl.view(n, c)

    yh, yl = run(rows)
    picked = x[::stride]
    want, mag, var = cnext_draws.ln_want(picked.double(), picked.double().abs(), gamma, beta)
    assert var.min().item() >= cnext_draws.VAR_FLOOR
    c_f = cnext_draws.C_F["ln", 147, 768] if c == 768 else cnext_draws.C_F["ln", 3136, 96]      # DESIGN.md 22's constants for the same C
    worst = ((merge(yh, yl).cpu().double() - want).abs() / cnext_draws.tol(mag, c_f)).max().item()
    print("LayerNorm of %d rows %d apart x %d: worst err / bound %.3f (C_f %g)" % (rows, stride, c, worst, c_f))
    assert worst <= 1.0
    # mpx_layernorm_c on the gathered rows: the same bits
    ph, pl = split(picked.contiguous().to(dev))
    out = FencedPair(rows, c, dev)
    oh, ol = out.ptrs()
    _lib.check(eng._h, eng._lib.mpx_layernorm_c(eng._h, ptr(ph), ptr(pl), ptr(g), ptr(b), EPS, oh, ol, rows, c, 0, eng._stream()), "mpx_layernorm_c")
    wh, wl = out.result()
    assert torch.equal(bits(wh.view(rows, c)), bits(yh)) and torch.equal(bits(wl.view(rows, c)), bits(yl))
    # the last row alone, and a grid of one workgroup
    ah, al = run(1, at=rows - 1)
    assert torch.equal(bits(ah[0]), bits(yh[rows - 1])) and torch.equal(bits(al[0]), bits(yl[rows - 1]))
    ch, cl = run(rows, max_blocks=1)
    assert torch.equal(bits(ch), bits(yh)) and torch.equal(bits(cl), bits(yl))
    call = eng._lib.mpx_layernorm_rows
    oh, ol = FencedPair(rows, c, dev).ptrs()
    assert call(eng._h, ptr(xh), ptr(xl), ptr(g), ptr(b), EPS, oh, ol, rows, 0, c, 0, None) == -1
    assert call(eng._h, ptr(xh), ptr(xl), ptr(g), ptr(b), EPS, oh, ol, 0, stride, c, 0, None) == -1
    assert call(eng._h, ptr(xh), ptr(xl), ptr(g), ptr(b), EPS, oh, ol, rows, stride, c + 4, 0, None) == -1
    assert call(eng._h, ptr(xh), ptr(xl), None, ptr(b), EPS, oh, ol, rows, stride, c, 0, None) == -1


# ------------------------------------------------------------------------------------------------
# the conv layers: both stems, in_proj, out_proj + residual, mlp.0 + GELU, mlp.3 + residual
# ------------------------------------------------------------------------------------------------
def _sd_tensors(sd, name):
    full = ref.PREFIX + name if name.startswith("encoder_layer_") else name
    if name.endswith(".in_proj"):
        return sd[full + "_weight"], sd[full + "_bias"]
    return sd[full + ".weight"], sd[full + ".bias"]


def _run_layer(eng, i, batch, seed):
    """Layer i on a random input of `batch` images: (engine output fp64 [rows][cout], input fp64, residual fp64 or None)."""
    d = eng.layers[i]
    dev = eng.device
    g = torch.Generator().manual_seed(seed)
    rows = batch * (eng.conv_rows[i] or d.hout * d.hout)
    rh = rl = None
    if d.residual:
        rh, rl = split(torch.randn(rows, d.cout, generator=g).to(dev))
    if i == 0:      # the stem reads the engine's padded NHWC4 staging: write the interior, zero border and 4th channel
        x = torch.randn(batch, 224, 224, 3, generator=g) * 1.5
        xh, xl = split(x.to(dev))
        stage_stem_input(eng, xh, xl, batch)
        in_h = in_l = None
    else:
        x = torch.randn(rows, d.cin, generator=g) * 1.5
        xh, xl = split(x.to(dev))
        in_h, in_l = xh, xl
    fo = FencedPair(rows, d.cout, dev)
    oh, ol = fo.ptrs()
    rc = eng._lib.mpx_conv_bn_act(eng._h, i, ptr(in_h), ptr(in_l), ptr(rh), ptr(rl), oh, ol, None, batch, eng._stream())
    _lib.check(eng._h, rc, "mpx_conv_bn_act")
    yh, yl = fo.result()
    return merge(yh, yl).cpu().double().view(rows, d.cout), merge(xh, xl).cpu().double(), (merge(rh, rl).cpu().double() if d.residual else None)


def _check(eng, sd, i, batch, tile):
    with conv_tile(eng, i, tile):
        got, x64, r64 = _run_layer(eng, i, batch, seed=1000 * i + batch)
        ran = eng._lib.mpx_last_conv_kernels(eng._h)
    d = eng.layers[i]
    name = d.name.decode()
    w, bias = _sd_tensors(sd, name)
    if i == 0:
        want = F.conv2d(x64.permute(0, 3, 1, 2), w.double(), bias.double(), d.stride).permute(0, 2, 3, 1).reshape(-1, d.cout)
    else:
        want = F.linear(x64, w.double(), bias.double())
    if eng.epilogue_acts[i]:
        want = F.gelu(want)
    if r64 is not None:
        want = want + r64
    fields = "%d->%d k%d rows/image %d K %d res %d act %d " % (d.cin, d.cout, d.ksize, eng.conv_rows[i] or d.hout * d.hout, d.k_packed, d.residual, eng.epilogue_acts[i])
    return assert_layer_close(d, got, want, tile, batch, ran, fields), want


@pytest.mark.parametrize("arch", ref.ARCHS)
def test_patchify_stem_on_every_accepted_tile(engines, sds, arch):
    """conv_proj, 16 x 16 stride 16 (k_per_tap 64: two K steps per kernel row) and 32 x 32 stride 32 (k_per_tap 128: four), reading the padded
    NHWC4 staging 3 pixels into its border, batches 1 and 3."""
    eng, sd = engines[arch], sds[arch]
    accepted = accepted_tiles(eng, 0)
    assert set(accepted) == GENERIC and eng._lib.mpx_get_conv_tile(eng._h, 0) == 2
    for t in accepted:
        for batch in (1, 3):
            ran, _want = _check(eng, sd, 0, batch, t)
            assert ran == 1 << t


@pytest.mark.parametrize("arch,layer", [(a, l) for a in ref.ARCHS for l in ("self_attention.in_proj", "self_attention.out_proj", "mlp.0", "mlp.3")])
def test_token_layers_on_every_accepted_tile(engines, sds, arch, layer):
    """in_proj (768 -> 2304), out_proj (768 -> 768 + residual), mlp.0 (768 -> 3072 + GELU) and mlp.3 (3072 -> 768 + residual) of encoder layer
    5 on B x T rows (T = 197: prime, no square map; 50), B = 1 and 3, on every tile each accepts."""
    eng, sd = engines[arch], sds[arch]
    i = [d.name.decode() for d in eng.layers].index("encoder_layer_5." + layer)
    accepted = accepted_tiles(eng, i)
    assert eng._lib.mpx_get_conv_tile(eng._h, i) in accepted
    want_set = GENERIC if layer == "mlp.0" else (GENERIC | {9, 10, 13} if layer.endswith("in_proj") else GENERIC | {9, 10})
    assert set(accepted) == want_set, (layer, accepted)
    for t in accepted:
        for batch in (1, 3):
            ran, want = _check(eng, sd, i, batch, t)
            assert ran & ((1 << t) | (1 << FALLBACK.get(t, t))), (layer, t, ran)
            if layer == "mlp.0":
                assert ran == 1 << t and (want < -0.1).any() and want.min().item() > -0.1701 and (want > 3.0).any()


def test_logit_layer_on_every_accepted_tile(b16, sds, dev):
    eng, sd = b16, sds["vit_b_16"]
    i = len(eng.layers) - 1
    d = eng.layers[i]
    w, bias = _sd_tensors(sd, "heads.head")
    for t in sorted(GENERIC):
        assert eng._lib.mpx_set_conv_tile(eng._h, i, t) == 0
        try:
            x = torch.randn(3, 768, generator=torch.Generator().manual_seed(t)) * 1.5
            xh, xl = split(x.to(dev))
            out = torch.full((3, 1000), float("nan"), dtype=torch.float32, device=dev)
            _lib.check(eng._h, eng._lib.mpx_conv_bn_act(eng._h, i, ptr(xh), ptr(xl), None, None, None, None, ptr(out), 3, eng._stream()), "mpx_conv_bn_act")
            torch.cuda.synchronize()
        finally:
            eng._lib.mpx_set_conv_tile(eng._h, i, -1)
        want = F.linear(merge(xh, xl).cpu().double(), w.double(), bias.double())
        err = (out.cpu().double() - want).abs().max().item()
        assert err <= LAYER_TOL * max(want.abs().max().item(), 1.0), (t, err)
    assert d.cout == 1000


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ref.ARCHS)
def test_vit_end_to_end(engines, sds, golden_dir, arch):
    """Engine against the fp64 scorer on both committed segment fixtures, 3 felzenszwalb + 2 grid rows: scores within SCORE_BOUND, printed
    next to the yardstick (the fp32 CPU loop against fp64), every argmax equal, all logits through the lens (engine <= 4 d_L)."""
    eng, sd = engines[arch], sds[arch]
    lens = LogitsLens(arch)
    for kind, m, _seed in ref.E2E_CASES:
        r = ref.e2e_rows(golden_dir, arch)[kind]
        img, seg, x, onoff, label, s64, logits64 = (r[k] for k in ("img", "seg", "x", "onoff", "label", "s64", "logits64"))
        _o, score, pred, logits = eng.score_masks(img, seg, onoff, label, return_logits=True)
        ref_score, ref_pred, ref_logits = ref.score_masks_reference_loop(sd, x, seg, onoff, label, return_logits=True)
        lens.add(kind, logits, ref_logits, logits64)
        top2 = np.sort(logits64, axis=1)[:, -2:]
        gap = top2[:, 1] - top2[:, 0]
        err_engine = float(np.abs(score.astype(np.float64) - s64).max())
        err_cpu = float(np.abs(ref_score.astype(np.float64) - s64).max())
        print("%s %s: %d masks, label %d, scores %.4f..%.4f; max|d| engine vs fp64 %.3e, fp32 CPU loop vs fp64 %.3e, smallest fp64 logit gap %.4f"
              % (arch, kind, m, label, s64.min(), s64.max(), err_engine, err_cpu, gap.min()))
        peaks = F.softmax(torch.from_numpy(logits64), 1).max(1)[0].numpy()
        assert gap.min() >= 1e-3 and peaks.min() >= 0.05 and peaks.max() <= 0.95      # tests/test_vit_cpu.py holds the weights to it
        assert err_engine <= SCORE_BOUND <= SCORE_TOL
        assert (pred == logits64.argmax(1)).all() and (pred == ref_pred).all()
        p_label, _ = eng.predict(img)
        assert p_label == label
    lens.check()


@pytest.mark.parametrize("arch", ref.ARCHS)
def test_a_mask_row_scores_the_same_bits_wherever_it_sits(engines, golden_dir, arch):
    check_position_independence(engines[arch], *ref.e2e_inputs(golden_dir, "felz"), (3, ((1, 0, (0,)), (8, 41, (0, 5, 7)), (13, 44, (3, 8, 12)))))


def test_api_on_a_vit_engine(engines, sds, golden_dir):
    check_api(engines["vit_b_32"], Reference(ref, sds["vit_b_32"]), *ref.e2e_inputs(golden_dir, "grid"),
              rows=4, same_pred=True, heatmaps=0, predict=False, table_step=None, validate=None)


def test_profile_lists_the_attention_launches(b16, dev):
    eng = b16
    img = torch.from_numpy(synth.make_images(1, kind="noise")[0]).to(dev)
    seg = torch.from_numpy(synth.grid_segments()).to(dev)
    onoff = torch.from_numpy(synth.random_onoff(4, 196)).to(dev)
    labels = torch.zeros(4, dtype=torch.int32, device=dev)
    eng.profile(True)
    eng.stage_masks(img, seg, onoff, 0)
    eng.forward(4, labels)
    eng.profile(False)
    prof = eng.collect_profile()
    assert len(prof["per_attn_ms"]) == 12 and all(ms > 0 for ms in prof["per_attn_ms"]) and prof["tokens_ms"] > 0
    assert len(prof["per_lnorm_ms"]) == 25 and all(ms > 0 for ms in prof["per_lnorm_ms"])
    assert prof["per_dw_ms"] == [] and prof["per_norm_ms"] == [] and prof["per_se_gate_ms"] == []
    assert prof["launches"]["pool"] == 12 + 25 + 1 and prof["launches"]["conv"] == 50 and prof["launches"]["head"] == 1     # 89 launches of the forward and K0's


def test_vit_error_paths(b16, mpx_lib, dev, sds):
    eng = b16
    with pytest.raises(ValueError):
        MaskedForwardEngine("vit_b_16", max_batch=2, device=0, stem="table")
    z = torch.zeros(224, 224, dtype=torch.int32, device=dev)
    im = torch.zeros(224, 224, 3, dtype=torch.uint8, device=dev)
    on = torch.ones(1, 1, dtype=torch.uint8, device=dev)
    mean = (C.c_float * 3)(*scorer.MEAN)
    std = (C.c_float * 3)(*scorer.STD)
    assert eng._lib.mpx_stem_table_build(eng._h, ptr(im), None, ptr(z), 1, mean, std, None) == -2
    assert eng._lib.mpx_stem_table_apply(eng._h, ptr(on), 1, 1, 0, None) == -2
    buf = torch.zeros(64, dtype=torch.float16, device=dev)
    assert eng._lib.mpx_stem_conv_maxpool(eng._h, ptr(buf), ptr(buf), 1, None) == -2
    ad = _lib.AttnDesc()
    assert eng._lib.mpx_attn_info(eng._h, 12, C.byref(ad)) == -1 and eng._lib.mpx_attn_info(eng._h, -1, C.byref(ad)) == -1
    fresh = MaskedForwardEngine("vit_b_32", max_batch=2, device=0)
    try:
        sd = sds["vit_b_32"]
        fresh.load_state_dict(sd, only=[d.name.decode() for d in fresh.layers])     # no LayerNorm, no tokens
        assert fresh._lib.mpx_weights_complete(fresh._h) == 0
        for k, d in enumerate(fresh.lnorms):
            n = ref.PREFIX + d.name.decode() if d.name.startswith(b"encoder_layer_") else d.name.decode()
            assert fresh._lib.mpx_load_lnorm(fresh._h, k, C.c_void_p(sd[n + ".weight"].data_ptr()), C.c_void_p(sd[n + ".bias"].data_ptr()), EPS) == 0
        assert fresh._lib.mpx_weights_complete(fresh._h) == 0                        # the class token and the position embedding count
        fresh.stage_masks(im, z, on, 0)
        labels = torch.zeros(1, dtype=torch.int32, device=dev)
        score = torch.zeros(1, device=dev)
        pred = torch.zeros(1, dtype=torch.int32, device=dev)
        assert fresh._lib.mpx_forward(fresh._h, ptr(labels), ptr(score), ptr(pred), None, 1, None) == -2
        assert fresh._lib.mpx_load_tokens(fresh._h, None, C.c_void_p(sd["encoder.pos_embedding"].data_ptr())) == -1
        assert fresh._lib.mpx_load_tokens(fresh._h, C.c_void_p(sd["class_token"].data_ptr()), C.c_void_p(sd["encoder.pos_embedding"].data_ptr())) == 0
        assert fresh._lib.mpx_weights_complete(fresh._h) == 1
        assert fresh._lib.mpx_forward(fresh._h, ptr(labels), ptr(score), ptr(pred), None, 1, None) == 0
        torch.cuda.synchronize()
        with pytest.raises((KeyError, ValueError)):     # the other ViT's state_dict: conv_proj.weight has another shape
            fresh.load_state_dict(sds["vit_b_16"])
    finally:
        fresh.close()
