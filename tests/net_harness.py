"""The drivers the tests/test_gpu_<net>.py files share (test infrastructure only): one conv layer through mpx_conv_bn_act against the
family's fp64 arithmetic, the whole network against the fp64 restatement and the batch-1 fp32 CPU loop, position independence of a mask
row, and the reference-named API on an engine.  A family's file supplies its engine fixtures, its `_ref_layer`, a `Reference` bound to its
tests/<net>_ref.py, and the tables of what it checks; the derivations of the bounds stay in the family files' docstrings."""
import contextlib
import random

import numpy as np
import torch
import torch.nn.functional as F

import netref
from gpu_common import FencedPair, SCORE_BOUND, SCORE_TOL, layer_bound, merge, pitch_of, ptr, round_up_one_digit, split
from logits_lens import LogitsLens
from network_interpretation_imagenet_amd import _lib, api, shard, synth
from network_interpretation_imagenet_amd.engine import rank_segments
from oracle import scorer


class Reference:
    """A family's tests/<net>_ref.py bound to one state_dict (and, where the module serves several, one arch): what the drivers below call.
    The forward(sd, x) is the module's own, or its bound(arch)."""

    def __init__(self, mod, sd, arch=None):
        a = () if arch is None else (arch,)
        self.sd, self.forward = sd, mod.forward if arch is None else mod.bound(arch)
        self.loop = lambda *args, **kw: mod.score_masks_reference_loop(sd, *a, *args, **kw)
        self.fp64 = lambda *args, **kw: mod.score_masks_fp64(sd, *a, *args, **kw)

    def predict(self, x_chw):
        return netref.predict(self.forward, self.sd, x_chw)

    def scorer32(self):
        """masked CHW image, label -> the fp32 softmax score of one batch-1 forward (the state_dict is cast once)."""
        sd32 = netref.cast(self.sd, torch.float32)

        def score_one(masked_chw, label):
            with torch.no_grad():
                logits = self.forward(sd32, torch.from_numpy(masked_chw[None]))
            return F.softmax(logits, 1).numpy()[0][label]
        return score_one


# ------------------------------------------------------------------------------------------------
# a. one conv layer
# ------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def conv_tile(eng, i, tile):
    """Layer i on `tile` (-1: its default) for the block, back on its default tile behind it."""
    rc = eng._lib.mpx_set_conv_tile(eng._h, i, tile)
    assert rc == 0, eng._lib.mpx_last_error(eng._h)
    try:
        yield
    finally:
        eng._lib.mpx_set_conv_tile(eng._h, i, -1)


def stage_stem_input(eng, xh, xl, batch):
    """The stem reads the engine's padded NHWC4 staging: write the interior, zero border and 4th channel."""
    ih, il = eng.input_planes(batch)
    ih.zero_()
    il.zero_()
    ih[:, 3:227, 3:227, :3] = xh
    il[:, 3:227, 3:227, :3] = xl
    eng.mark_input_staged(0, batch)


def assert_layer_close(d, got, want, tile, batch, ran, fields=""):
    """max |got - want| of conv layer d within layer_bound; prints the measurement with the family's `fields` behind the name (None: no
    line).  -> ran, for the caller's kernel-mask assertions."""
    name = d.name.decode()
    err = (got - want).abs().max().item()
    scale = want.abs().max().item()
    bound = layer_bound(d, scale)
    if fields is not None:
        print("%s %stile %d batch %d: max err %.3e (scale %.2f, bound %.3e), kernels 0x%x" % (name, fields, tile, batch, err, scale, bound, ran))
    assert err <= bound, "%s tile %d batch %d: max err %.3e (scale %.2f)" % (name, tile, batch, err, scale)
    return ran


def check_conv_layer(eng, i, batch, ref_layer, tile=-1, clamp=True, pitched=False, fenced=False, fields=""):
    """mpx_conv_bn_act of layer i on `tile` with seeded split-fp16 inputs (seed 1000 i + batch; a residual where the layer takes one)
    against ref_layer(d, x64 [B][cin][h][h], r64 or None) -> fp64 [B][cout][ho][ho].

    clamp:   the draw is clamped at -0.5 (post-ReLU-like) before it is scaled.
    pitched: activations sit at pitch_of(channels) with exact zeros in the pad channels, on the way in (drawn so) and on the way out
             (asserted); otherwise the planes are dense.
    fenced:  the output planes are FencedPair (sentinel rows around them) instead of NaN-prefilled tensors.
    fields:  what the printed line says between the layer's name and the tile (assert_layer_close).
    The last layer writes fp32 logits.  -> (mpx_last_conv_kernels, want [B][ho][ho][cout])."""
    d = eng.layers[i]
    dev = eng.device
    last = i == len(eng.layers) - 1
    cin_p = pitch_of(d.cin) if pitched and d.cin != 3 else d.cin
    cout_p = pitch_of(d.cout) if pitched and not last else d.cout
    g = torch.Generator().manual_seed(1000 * i + batch)
    x = torch.randn(batch, d.hin, d.hin, cin_p, generator=g)
    x = (x.clamp_min(-0.5) if clamp else x) * 1.5
    x[..., d.cin:] = 0.0                                    # padded channels hold exact zeros wherever they are read
    xh, xl = split(x.to(dev))
    rh = rl = None
    if d.residual:
        res = torch.randn(batch, d.hout, d.hout, cout_p, generator=g)
        res[..., d.cout:] = 0.0
        rh, rl = split(res.to(dev))
    with conv_tile(eng, i, tile):
        if i == 0:
            stage_stem_input(eng, xh, xl, batch)
            in_h = in_l = None
        else:
            in_h, in_l = xh, xl
        if last:
            out = torch.full((batch, d.cout), float("nan"), dtype=torch.float32, device=dev)
            rc = eng._lib.mpx_conv_bn_act(eng._h, i, ptr(in_h), ptr(in_l), None, None, None, None, ptr(out), batch, eng._stream())
            _lib.check(eng._h, rc, "mpx_conv_bn_act")
            torch.cuda.synchronize()
            got = out.double().view(batch, 1, 1, d.cout)
        else:
            if fenced:
                planes = FencedPair(batch * d.hout * d.hout, cout_p, dev)
                oh, ol = planes.ptrs()
            else:
                yh = torch.full((batch, d.hout, d.hout, cout_p), float("nan"), dtype=torch.float16, device=dev)
                yl = torch.full_like(yh, float("nan"))
                oh, ol = ptr(yh), ptr(yl)
            rc = eng._lib.mpx_conv_bn_act(eng._h, i, ptr(in_h), ptr(in_l), ptr(rh), ptr(rl), oh, ol, None, batch, eng._stream())
            _lib.check(eng._h, rc, "mpx_conv_bn_act")
            torch.cuda.synchronize()
            if fenced:
                yh, yl = (t.view(batch, d.hout, d.hout, cout_p) for t in planes.result())
            assert (yh[..., d.cout:].view(torch.int16) == 0).all() and (yl[..., d.cout:].view(torch.int16) == 0).all(), d.name     # exact zeros
            got = merge(yh, yl).double()[..., :d.cout]
        ran = eng._lib.mpx_last_conv_kernels(eng._h)
    assert not torch.isnan(got).any(), d.name
    x64 = merge(xh, xl).double()[..., :d.cin].permute(0, 3, 1, 2)
    r64 = merge(rh, rl).double()[..., :d.cout].permute(0, 3, 1, 2) if d.residual else None
    want = ref_layer(d, x64, r64).permute(0, 2, 3, 1)
    assert_layer_close(d, got.to(want.device), want, tile, batch, ran, fields)
    return ran, want


# ------------------------------------------------------------------------------------------------
# b. end to end
# ------------------------------------------------------------------------------------------------
def e2e_rows(ref, cases, golden_dir):
    """(kind, img, seg, onoff, label, s64, logits64) per (kind, m, seed) of a family's E2E_CASES: the label is the fp32 prediction of the
    unmasked image, which must be neither flat nor saturated."""
    for kind, m, seed in cases:
        img, seg = netref.e2e_inputs(golden_dir, kind)
        label, prob = ref.predict(scorer.to_tensor_normalize(img))
        assert 0.05 <= prob.max() <= 0.95
        onoff = synth.random_onoff(m, len(np.unique(seg)), seed=seed)
        s64, logits64 = ref.fp64(scorer.to_tensor_normalize(img), seg, onoff, label)
        yield kind, img, seg, onoff, label, s64, logits64


def check_end_to_end(eng, arch, ref, rows, summary, segments=True, peaks=False):
    """The engine on every row of `rows` (e2e_rows, or a family's cached (kind, img, seg, onoff, label, s64, logits64)) against the fp64
    restatement and against the batch-1 fp32 CPU loop, which is the yardstick: with d = max |fp32 loop - fp64| over all rows, the bound on
    |engine - fp64| and |engine - fp32 loop| is SCORE_BOUND when 4 d < SCORE_BOUND, else 4 d rounded up to one digit and never above
    SCORE_TOL.  Every row: a top-two fp64 logit gap >= 1e-3 and the same argmax from all three; all logits through the logits lens;
    predict() agrees on the label.

    summary:  the yardstick line, a % format over arch, d, n (rows) and bound.
    segments: the first line of a row names the number of segments.
    peaks:    every row's fp64 softmax peak lies in [0.05, 0.95]."""
    lens = LogitsLens(arch)
    done = []
    for kind, img, seg, onoff, label, s64, logits64 in rows:
        x = scorer.to_tensor_normalize(img)
        _o, score, pred, logits = eng.score_masks(img, seg, onoff, label, return_logits=True)
        ref_score, ref_pred, ref_logits = ref.loop(x, seg, onoff, label, return_logits=True)
        lens.add(kind, logits, ref_logits, logits64)
        top2 = np.sort(logits64, axis=1)[:, -2:]
        gap = top2[:, 1] - top2[:, 0]
        err_engine = float(np.abs(score.astype(np.float64) - s64).max())
        err_cpu = float(np.abs(ref_score.astype(np.float64) - s64).max())
        err_both = float(np.abs(score.astype(np.float64) - ref_score.astype(np.float64)).max())
        print("%s %s: %d masks, %slabel %d, scores %.4f..%.4f"
              % (arch, kind, len(onoff), "S %d, " % len(np.unique(seg)) if segments else "", label, ref_score.min(), ref_score.max()))
        print("%s %s: max|d| engine vs fp64 %.3e, fp32 CPU loop vs fp64 (the yardstick) %.3e, engine vs fp32 CPU loop %.3e, smallest fp64 logit gap %.4f"
              % (arch, kind, err_engine, err_cpu, err_both, gap.min()))
        assert gap.min() >= 1e-3
        if peaks:
            top = F.softmax(torch.from_numpy(logits64), 1).max(1)[0].numpy()
            assert top.min() >= 0.05 and top.max() <= 0.95
        done.append((kind, err_engine, err_cpu, err_both, pred, ref_pred, logits64.argmax(1)))
        p_label, _ = eng.predict(img)
        assert p_label == label
    d = max(r[2] for r in done)
    bound = SCORE_BOUND if 4 * d < SCORE_BOUND else min(round_up_one_digit(4 * d), SCORE_TOL)
    print(summary % dict(arch=arch, d=d, n=sum(len(r[4]) for r in done), bound=bound))
    for kind, err_engine, _err_cpu, err_both, pred, ref_pred, arg64 in done:
        assert err_engine <= bound and err_both <= bound, (kind, err_engine, err_both, bound)
        assert (pred == arg64).all() and (pred == ref_pred).all()          # every row
    lens.check()


# ------------------------------------------------------------------------------------------------
# c. position independence, the reference-named API
# ------------------------------------------------------------------------------------------------
def check_position_independence(eng, img, seg, table):
    """table = (rows, ((m, seed, positions), ...)): `rows` seeded mask rows score the same bits -- score, prediction and all logits --
    alone and at `positions` inside batches of m other rows."""
    n_rows, batches = table
    S = len(np.unique(seg))
    rows = synth.random_onoff(n_rows, S, seed=31)
    label = 3
    _o, base_s, base_p, base_l = eng.score_masks(img, seg, rows, label, return_logits=True)
    for m, seed, at in batches:
        onoff = synth.random_onoff(m, S, seed=seed)
        for j, pos in enumerate(at):
            onoff[pos] = rows[j]
        _o, s, p, l = eng.score_masks(img, seg, onoff, label, return_logits=True)
        for j, pos in enumerate(at):
            assert np.array_equal(s[pos], base_s[j]) and p[pos] == base_p[j] and np.array_equal(l[pos], base_l[j]), (m, pos)


def check_api(eng, ref, img, seg, rows=12, tol=SCORE_BOUND, windows=(0, 9), same_pred=False, heatmaps=2, predict=True, table_step=11, validate=20):
    """The reference-named entry points on engine `eng` against the family's batch-1 fp32 forward: api.score_masks (the engine's own and the
    sharded scorer give the same bits), api.sample_loss on `windows`, and what the family's table asks for beyond that --
    same_pred: every prediction equals the CPU loop's;  heatmaps: 1 the sharded heatmap, 2 the engine's own as well, 0 neither;
    predict: predict() agrees and its probabilities sum to 1;  table_step: every table_step-th entry of SaliencySession.table();
    validate: validate_many == validate on that many mask samples.  None or 0 leaves a part out."""
    score_one = ref.scorer32()
    x = scorer.to_tensor_normalize(img)
    label, _ = ref.predict(x)
    S = len(np.unique(seg))
    assert eng.stem == "conv" and eng.stem_for_rows(4096) == "conv" and shard.job_stem(eng, 4096) == "conv"
    onoff = synth.random_onoff(rows, S, seed=5)
    _o, score, pred = api.score_masks(eng, img, seg, onoff, label)
    _o, score2, pred2 = eng.score_masks(img, seg, onoff, label)
    assert np.array_equal(score, score2) and np.array_equal(pred, pred2)
    ref_score, ref_pred = ref.loop(x, seg, onoff, label)
    assert np.abs(score.astype(np.float64) - ref_score).max() <= tol
    assert not same_pred or (pred == ref_pred).all()
    s_sh, p_sh = shard.score_masks_sharded(eng, img, seg, onoff, label)
    assert np.array_equal(s_sh, score) and np.array_equal(p_sh, pred)
    if heatmaps:
        rank_map = rank_segments(seg)[0]
        heat, n_ok = shard.heatmap_sharded(eng, img, rank_map, onoff, label)
        want_heat = sum((onoff[i][rank_map] for i in range(rows) if pred[i] == label), np.zeros((224, 224)))
        assert n_ok == int((pred == label).sum()) and np.array_equal(heat.cpu().numpy().astype(np.float64), want_heat.astype(np.float64))
        if heatmaps > 1:
            assert np.array_equal(eng.heatmap(rank_map, onoff, pred, label), want_heat.astype(np.float64))
    if predict:
        p_label, p_prob = eng.predict(img)
        assert p_label == label and abs(float(p_prob.sum()) - 1.0) < 1e-5
    api.configure(eval_img_index=1, segmenter=lambda _img_show: seg, mask_dir=None, seed=None)
    loader = [(x[None], torch.tensor([label]))]
    for f in windows:
        got = api.sample_loss([f], loader, eng, None)
        assert abs(float(got) - float(score_one(scorer.apply_mask(x, scorer.window_mask_u8(seg, f)), label))) <= tol
    if table_step:
        table_s, _table_p = api.SaliencySession(eng, x, label, segments=seg).table()
        assert len(table_s) == S + 1
        for f in range(0, S + 1, table_step):
            assert abs(float(table_s[f]) - float(score_one(scorer.apply_mask(x, scorer.window_mask_u8(seg, f)), label))) <= tol
    if validate:
        many = api.validate_many(list(loader), eng, None, [1], num_mask_samples=validate, rng=random.Random(3))
        one = api.validate(list(loader), eng, None, 1, num_mask_samples=validate, rng=random.Random(3))
        assert many == {1: one}
