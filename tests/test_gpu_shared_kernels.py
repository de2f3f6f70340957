"""The kernels every network ends in -- mpx_maxpool3x3s2, mpx_global_avgpool, mpx_head_softmax_gather, mpx_avgpool2_pad and
mpx_heatmap_accumulate -- at their edges (pytest -m gpu), through the C-ABI as tests/test_gpu_efficientnet.py does.

Every output buffer carries 64 NaN elements (a sentinel for int32) in front of and behind the extent the call owns, and both bands are
asserted untouched.  Inputs come from tests/shared_kernel_draws.py: exact zeros, both signs, values beyond +-10, a channel band scaled by
1e-3 (lo in fp16's subnormals), every value a valid (hi, lo) pair.  The bounds and their rounding counts are in that module's docstring;
tests/test_shared_kernel_bounds_cpu.py holds a numpy emulation of the kernels' arithmetic to the same bounds on the same draws.

Max pool and heat map are exact.  Worst err / bound measured on one MI355X: global pool 0.45, DownsampleB 0.50, head 0.61 (1000 classes)
and 0.35 (10 classes); 5 and 3 of the 57 head rows lie under the 1e-37 floor.  Every test prints its figure on every run."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import shared_kernel_draws as draws
from gpu_common import dev, merge, ptr as _p, split  # noqa: F401  (dev is a fixture)
from network_interpretation_imagenet_amd import _lib
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine
from oracle import scorer

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -1234567


def guarded(n, dtype, dev):
    """(buffer with GUARD elements on either side of n owned ones, the owned view): NaN everywhere, SENTINEL for int32."""
    fill = SENTINEL if dtype == torch.int32 else float("nan")
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def bands_untouched(buf, n):
    front, back = buf[:GUARD], buf[GUARD + n:]
    assert back.numel() == GUARD
    if buf.dtype == torch.int32:
        return bool((front == SENTINEL).all() and (back == SENTINEL).all())
    return bool(torch.isnan(front).all() and torch.isnan(back).all())


def _smallnet_sd(arch, golden_dir):
    g = np.load(os.path.join(golden_dir, "smallnet_%s.npz" % arch))
    return {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}


@pytest.fixture(scope="module")
def engines(mpx_lib, dev, golden_dir):
    """One small resnet18 engine and the reference's two small networks with their shipped weights."""
    es = {"resnet18": MaskedForwardEngine("resnet18", max_batch=8, device=0)}
    for arch in ("cifar_resnet56", "mnist_net"):
        es[arch] = MaskedForwardEngine(arch, max_batch=8, device=0).load_state_dict(_smallnet_sd(arch, golden_dir))
    yield es
    for e in es.values():
        e.close()


def _geometry(eng):
    geo = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert eng._lib.mpx_geometry(eng._h, *[C.byref(v) for v in geo]) == 0
    return [v.value for v in geo]                   # image size, input channels, classes, logit pitch


# ------------------------------------------------------------------------------------------------
# mpx_maxpool3x3s2: bit-exact against F.max_pool2d(merged, 3, 2, 1), whose padding is -inf
# ------------------------------------------------------------------------------------------------
def _maxpool_check(eng, x, what):
    """x: merged fp32 planes [B][hin][hin][c] on the device, every value a valid pair.  -> the wanted output."""
    b, hin, _w, c = x.shape
    ho = hin // 2
    xh, xl = split(x)
    assert torch.equal(merge(xh, xl), x)
    n = b * ho * ho * c
    bh, oh = guarded(n, torch.float16, x.device)
    bl, ol = guarded(n, torch.float16, x.device)
    _lib.check(eng._h, eng._lib.mpx_maxpool3x3s2(eng._h, _p(xh), _p(xl), _p(oh), _p(ol), b, hin, c, eng._stream()), "mpx_maxpool3x3s2")
    torch.cuda.synchronize()
    assert bands_untouched(bh, n) and bands_untouched(bl, n), what
    got = merge(oh, ol).view(b, ho, ho, c)
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    same = torch.equal(got, want)
    print("max pool %s: %d x %d x %d x %d, %d units, bit-exact %s, err / bound %.1f" % (what, b, hin, hin, c, n // 8, same, 0.0 if same else float("inf")))
    assert same, what
    return want


@pytest.mark.parametrize("b,hin,c", draws.MAXPOOL_CASES)
def test_maxpool_small_maps(engines, dev, b, hin, c):
    x = draws.planes((b, hin, hin, c), seed=100 * hin + c).to(dev)
    if hin >= 14:
        assert draws.planes_are_rich(x)
    assert (x < 0).any()
    _maxpool_check(engines["resnet18"], x, "case (%d, %d, %d)" % (b, hin, c))


def test_maxpool_signed_stem_shape(engines, dev):
    """The shape and draw of test_gpu_parity.py::test_maxpool_exact without its clamp: half the taps are negative."""
    x = draws.valid_pairs(torch.randn(3, 112, 112, 64, generator=torch.Generator().manual_seed(0))).to(dev)
    want = _maxpool_check(engines["resnet18"], x, "signed 3 x 112 x 112 x 64")
    assert (want < 0).any() and (want > 0).any()


def test_maxpool_all_negative_map(engines, dev):
    """Strictly negative everywhere: every border output is the maximum of its in-map taps and below 0, so a pool that pads with 0 (or
    clips a window wrongly and lets a 0 in) cannot pass."""
    x = draws.planes((2, 14, 14, 24), seed=5, sign=-1).to(dev)
    want = _maxpool_check(engines["resnet18"], x, "all negative")
    assert (want < 0).all()
    border = torch.cat([want[:, 0].reshape(-1), want[:, :, 0].reshape(-1)])
    assert (border < 0).all() and border.numel() == 2 * 2 * 7 * 24


def test_maxpool_strides_over_the_rest_of_the_capped_grid(engines, dev):
    """43 x 224 x 224 x 64: 43 * 112 * 112 * 8 = 4,315,136 units against the 16384 x 256 = 4,194,304 threads of the capped grid: the first
    threads take a second unit.  Four drawn images, each batch entry one of them rolled by its index, so that no two entries are equal."""
    b, hin, c = 43, 224, 64
    assert b * (hin // 2) * (hin // 2) * (c // 8) > 16384 * 256
    base = draws.planes((4, hin, hin, c), seed=43).to(dev)
    x = torch.stack([base[n % 4].roll(n, dims=1) for n in range(b)])
    assert not torch.equal(x[0], x[4]) and not torch.equal(x[38], x[42])
    _maxpool_check(engines["resnet18"], x, "capped grid")


# ------------------------------------------------------------------------------------------------
# mpx_global_avgpool against the fp64 mean
# ------------------------------------------------------------------------------------------------
def _avgpool_run(eng, x, dev):
    b, hw, c = x.shape
    xh, xl = split(x.to(dev))
    bh, oh = guarded(b * c, torch.float16, dev)
    bl, ol = guarded(b * c, torch.float16, dev)
    _lib.check(eng._h, eng._lib.mpx_global_avgpool(eng._h, _p(xh), _p(xl), _p(oh), _p(ol), b, hw, c, eng._stream()), "mpx_global_avgpool")
    torch.cuda.synchronize()
    assert bands_untouched(bh, b * c) and bands_untouched(bl, b * c)
    return merge(oh, ol).view(b, c).cpu().double()


@pytest.mark.parametrize("b,hw,c", draws.AVGPOOL_CASES)
def test_global_avgpool_against_fp64(engines, dev, b, hw, c):
    x = draws.planes((b, hw, c), seed=100 * hw + c)
    want, bound = draws.avgpool_bound(x.double())
    got = _avgpool_run(engines["resnet18"], x, dev)
    assert not torch.isnan(got).any()
    worst = ((got - want).abs() / bound).max().item()
    print("global pool %d x %d x %d: worst err / bound %.3f" % (b, hw, c, worst))
    assert worst <= 1.0
    if hw >= 49:
        # signed, with cancellation: the non-negative input of test_gpu_parity.py::test_global_avgpool is not the only one that passes
        assert draws.planes_are_rich(x) and (x < 0).any()
        assert (want.abs() < 0.1 * x.double().abs().mean(1)).any()


# ------------------------------------------------------------------------------------------------
# mpx_head_softmax_gather
# ------------------------------------------------------------------------------------------------
def _head_run(eng, rows, label, dev, pad=0.0):
    """rows f32[B][ncls] (numpy) placed in [B][pitch] with `pad` (a value, or a [pitch - ncls] vector) in the columns behind ncls."""
    _img, _ch, ncls, pitch = _geometry(eng)
    b = rows.shape[0]
    assert rows.shape[1] == ncls
    full = torch.zeros(b, pitch, dtype=torch.float32)
    full[:, :ncls] = torch.from_numpy(rows)
    if pitch > ncls:
        full[:, ncls:] = torch.as_tensor(pad, dtype=torch.float32)
    ld = full.contiguous().to(dev)
    lb = torch.from_numpy(np.asarray(label, dtype=np.int32)).to(dev)
    bs, score = guarded(b, torch.float32, dev)
    bp, pred = guarded(b, torch.int32, dev)
    _lib.check(eng._h, eng._lib.mpx_head_softmax_gather(eng._h, _p(ld), _p(lb), _p(score), _p(pred), b, eng._stream()), "mpx_head_softmax_gather")
    torch.cuda.synchronize()
    assert bands_untouched(bs, b) and bands_untouched(bp, b)
    return score.cpu().numpy().copy(), pred.cpu().numpy().copy()


ENGINES = ["resnet18", "cifar_resnet56", "mnist_net"]


@pytest.mark.parametrize("which", ENGINES)
def test_head_scores_and_argmax(engines, dev, which):
    eng = engines[which]
    _img, _ch, ncls, pitch = _geometry(eng)
    assert (ncls, pitch) == ((1000, 1000) if which == "resnet18" else (10, 16))
    worst, low, total = 0.0, 0, 0
    for name, rows, label in draws.head_cases(ncls):
        score, pred = _head_run(eng, rows, label, dev)
        w, n_low = draws.head_check("%s %s" % (which, name), score, pred, rows, label)
        worst, low, total = max(worst, w), low + n_low, total + len(label)
    print("head %s: %d rows, %d under the 1e-37 floor, worst err / bound %.3f" % (which, total, low, worst))
    assert total == 57 and low < 0.10 * total


@pytest.mark.parametrize("which", ENGINES)
def test_head_ties_and_labels_out_of_range(engines, dev, which):
    eng = engines[which]
    ncls = _geometry(eng)[2]
    rows, label, what = draws.head_tie_rows(ncls)
    score, pred = _head_run(eng, rows, label, dev)
    for i, name in enumerate(what):
        assert pred[i] == int(rows[i].argmax()) == int(torch.argmax(torch.from_numpy(rows[i]))), (name, pred[i])
    draws.head_check("%s ties" % which, score, pred, rows, label)
    assert what[-1] == "all equal" and pred[-1] == 0
    assert abs(float(score[-1]) - 1.0 / ncls) <= draws.head_want(rows[-1:], label[-1:])[1][0]
    for bad in (-1, ncls, 2 ** 31 - 1):
        s, p = _head_run(eng, rows, np.full(len(label), bad, dtype=np.int32), dev)
        assert (s.view(np.int32) == 0).all() and np.array_equal(p, pred), bad                 # exactly +0.0, and the argmax is still right
    mixed = label.copy()
    mixed[1::2] = ncls
    s, p = _head_run(eng, rows, mixed, dev)
    assert (s[1::2].view(np.int32) == 0).all() and np.array_equal(s[0::2].view(np.int32), score[0::2].view(np.int32)) and np.array_equal(p, pred)


@pytest.mark.parametrize("which", ["cifar_resnet56", "mnist_net"])
def test_head_never_reads_the_pad_columns(engines, dev, which):
    """ncls = 10 at pitch 16: 54 of the 64 lanes have no element, and columns 10 .. 15 may hold anything."""
    eng = engines[which]
    _img, _ch, ncls, pitch = _geometry(eng)
    assert pitch - ncls == 6
    junk = np.array([np.inf, np.nan, np.inf, np.nan, 3e38, np.inf], dtype=np.float32)
    for name, rows, label in draws.head_cases(ncls)[-3:] + [("ties",) + draws.head_tie_rows(ncls)[:2]]:
        s0, p0 = _head_run(eng, rows, label, dev, pad=0.0)
        s1, p1 = _head_run(eng, rows, label, dev, pad=junk)
        assert np.array_equal(s0.view(np.int32), s1.view(np.int32)) and np.array_equal(p0, p1), name
        assert np.isfinite(s1).all()
    print("head %s: the same bits with 0 and with inf / NaN behind column %d, err / bound 0.0" % (which, ncls))


@pytest.mark.parametrize("which", ENGINES)
def test_head_all_nan_row(engines, dev, which):
    """What the reference computes for an all-masked picture of the small networks: torch.argmax of an all-NaN row is 0, its softmax NaN.
    The rows around it are not disturbed."""
    eng = engines[which]
    ncls = _geometry(eng)[2]
    name, rows, label = draws.head_cases(ncls)[7]                   # B 5, spread 4
    rows = rows.copy()
    rows[1] = np.nan
    rows[4] = np.nan
    assert int(torch.argmax(torch.from_numpy(rows[1]))) == 0
    score, pred = _head_run(eng, rows, label, dev)
    assert np.isnan(score[[1, 4]]).all() and (pred[[1, 4]] == 0).all()
    keep = [0, 2, 3]
    draws.head_check("%s next to NaN rows" % which, score[keep], pred[keep], rows[keep], label[keep])


# ------------------------------------------------------------------------------------------------
# mpx_avgpool2_pad (DownsampleB)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,hin,cin_p,cout_p", draws.AVGPAD_CASES)
def test_avgpool2_pad_against_fp64(engines, dev, b, hin, cin_p, cout_p):
    eng = engines["cifar_resnet56"]
    x = draws.planes((b, hin, hin, cin_p), seed=10 * hin + cin_p)
    xh, xl = split(x.to(dev))
    ho = hin // 2
    n = b * ho * ho * cout_p
    bh, oh = guarded(n, torch.float16, dev)
    bl, ol = guarded(n, torch.float16, dev)
    _lib.check(eng._h, eng._lib.mpx_avgpool2_pad(eng._h, _p(xh), _p(xl), _p(oh), _p(ol), b, hin, cin_p, cout_p, eng._stream()), "mpx_avgpool2_pad")
    torch.cuda.synchronize()
    assert bands_untouched(bh, n) and bands_untouched(bl, n)
    oh, ol = oh.view(b, ho, ho, cout_p), ol.view(b, ho, ho, cout_p)
    got = merge(oh, ol).cpu().double()
    assert not torch.isnan(got).any()
    want, bound = draws.avgpad_bound(x.double(), cin_p)
    worst = ((got[..., :cin_p] - want).abs() / bound).max().item()
    print("avgpool2_pad %d x %d x %d x %d -> %d: worst err / bound %.3f" % (b, hin, hin, cin_p, cout_p, worst))
    assert worst <= 1.0
    if cout_p > cin_p:          # the zero-filled channels: exact zeros in both planes
        assert (oh[..., cin_p:].view(torch.int16) == 0).all() and (ol[..., cin_p:].view(torch.int16) == 0).all()


# ------------------------------------------------------------------------------------------------
# mpx_heatmap_accumulate: exact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,m", [(1, 1), (257, 3), (4096, 5)])
@pytest.mark.parametrize("which", ["resnet18", "cifar_resnet56"])
def test_heatmap_accumulate_edges(engines, dev, which, s, m):
    """Per-row labels, a second block of the count kernel (S > 256), labels outside [0, S) (those pixels keep their old heat) and a
    non-zero starting map.  The reference is the oracle's literal accumulation on the in-range pixels."""
    eng = engines[which]
    side = _geometry(eng)[0]
    assert side == (224 if which == "resnet18" else 32)
    npix = side * side
    rng = np.random.default_rng(1000 * s + m + side)
    seg = rng.integers(0, s, npix).astype(np.int32)
    seg[: min(s, npix)] = np.arange(min(s, npix))                   # the highest rank is present where the map has room for it
    out = rng.choice(npix, 40, replace=False)
    seg[out[:10]], seg[out[10:20]], seg[out[20:30]], seg[out[30:]] = -1, s, 2 ** 31 - 1, -2 ** 31
    inside = (seg >= 0) & (seg < s)
    onoff = rng.integers(0, 2, (m, s)).astype(np.uint8)
    onoff[0, s - 1] = 1
    label = (np.arange(m) * 3 + 1).astype(np.int32)                 # per-row labels that differ from row to row
    pred = label.copy()
    pred[1::3] = label[1::3] + 1                                    # ... some rows predicted wrongly
    pred[2::3] = label[np.arange(2, m, 3) - 1]                      # ... and some predicted as a neighbouring row's label
    start = rng.integers(0, 7, npix).astype(np.float32)
    buf, heat = guarded(npix, torch.float32, dev)
    heat.copy_(torch.from_numpy(start))
    d_seg, d_onoff, d_pred, d_label = (torch.from_numpy(a).to(dev) for a in (seg, onoff, pred, label))
    _lib.check(eng._h, eng._lib.mpx_heatmap_accumulate(eng._h, _p(d_seg), _p(d_onoff), _p(d_pred), _p(d_label), m, s, _p(heat), eng._stream()),
               "mpx_heatmap_accumulate")
    torch.cuda.synchronize()
    assert bands_untouched(buf, npix)
    # every rank appears in the map handed to the oracle (np.unique must be 0 .. S - 1): the in-range pixels, then one pixel per rank
    seg_ref = np.concatenate([np.where(inside, seg, 0), np.arange(s)]).reshape(-1, 1)
    add = scorer.summed_superpixel_labels(seg_ref, onoff, pred == label)[:npix, 0]
    want = start.astype(np.float64) + np.where(inside, add, 0.0)
    got = heat.cpu().numpy().astype(np.float64)
    exact = np.array_equal(got, want)
    print("heat map %s S %d M %d: %d correct rows, %d pixels out of range, exact %s, err / bound %.1f"
          % (which, s, m, int((pred == label).sum()), int((~inside).sum()), exact, 0.0 if exact else float("inf")))
    assert exact and (pred == label).any() and (~inside).sum() == 40
    assert np.array_equal(got[~inside], start[~inside].astype(np.float64)) and (add[inside] > 0).any()
    z = _p(heat)
    assert eng._lib.mpx_heatmap_accumulate(eng._h, z, z, z, z, 1, 4097, z, None) == -1
    assert eng._lib.mpx_heatmap_accumulate(eng._h, z, z, z, z, 1, 0, z, None) == -1


# ------------------------------------------------------------------------------------------------
# refusals: -1 before any launch
# ------------------------------------------------------------------------------------------------
def test_round_one_pool_entries_refuse_misaligned_planes_and_an_int_overflow(engines, dev):
    eng = engines["resnet18"]
    lib = eng._lib
    z = torch.zeros(8192, dtype=torch.float16, device=dev)
    a = _p(z)
    off = C.c_void_p(z.data_ptr() + 2)
    entries = [
        ("maxpool3x3s2", lib.mpx_maxpool3x3s2, (1, 4, 8)),
        ("maxpool2x2s2", lib.mpx_maxpool2x2s2, (1, 4, 8)),
        ("maxpool3x3s2p0", lib.mpx_maxpool3x3s2p0, (1, 5, 8)),
        ("global_avgpool", lib.mpx_global_avgpool, (1, 16, 8)),
        ("avgpool2_pad", lib.mpx_avgpool2_pad, (1, 4, 8, 16)),
        ("avgpool2x2s2", lib.mpx_avgpool2x2s2, (1, 4, 8)),
    ]
    for name, call, shape in entries:
        assert call(eng._h, a, a, _p(z[4096:]), _p(z[6144:]), *shape, None) == 0, name     # the same arguments, aligned: accepted
        torch.cuda.synchronize()
        for k in range(4):
            ptrs = [a, a, _p(z[4096:]), _p(z[6144:])]
            ptrs[k] = off
            assert call(eng._h, *ptrs, *shape, None) == -1, (name, k)
            msg = lib.mpx_last_error(eng._h).decode()
            assert name in msg and "16-byte aligned" in msg, msg
    # B * (c / 8) = 2^31 does not fit the kernel's int: refused, as mpx_global_avgpool_clamp6 refuses it
    assert lib.mpx_global_avgpool(eng._h, a, a, _p(z[4096:]), _p(z[6144:]), 2 ** 28, 1, 64, None) == -1
    assert lib.mpx_global_avgpool(eng._h, a, a, _p(z[4096:]), _p(z[6144:]), 0, 1, 64, None) == -1
    assert lib.mpx_global_avgpool(eng._h, a, a, _p(z[4096:]), _p(z[6144:]), 1, 1, 12, None) == -1
    assert lib.mpx_head_softmax_gather(eng._h, None, a, a, a, 1, None) == -1
    assert lib.mpx_head_softmax_gather(eng._h, a, a, a, a, 0, None) == -1
    assert not z.any()                                              # nothing but the accepted calls wrote, and those wrote zeros
