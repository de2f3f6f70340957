#!/usr/bin/env python3
"""Time the linear-surrogate path (csrc/mpx_surrogate.h) on a ResNet-101 engine, in one process:
  1. mpx_surrogate_accumulate per chunk of `batch` rows at (S, K) = (64, 1), (330, 5), (330, 1000), next to that chunk's forward
     (mpx_forward with the logits kept) and its class_scores -- device events, warm-up first, two alternating rounds;
  2. lime(n_samples) and kernel_shap(n_samples) in rows/s (wall clock around a synchronise: draws, uploads, forwards, sums, the one
     download, the host solve and the paint) next to score_masks on the same on/off rows.
`--baseline` runs only score_masks, on rows drawn here with numpy exactly as masks.lime_onoff draws them, and uses nothing this path added:
copied into a checkout of the parent commit it gives the parent's rows/s for the same rows.
usage: python tools/surrogate_bench.py [--baseline] [batch=2340] [reps=10] [n_samples=2000] [out=profiles/surrogate_bench.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

g.build()
from network_interpretation_imagenet_amd import synth  # noqa: E402
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine  # noqa: E402

args = [a for a in sys.argv[1:] if a != "--baseline"]
baseline = "--baseline" in sys.argv[1:]
batch = int(args[0]) if len(args) > 0 else 2340
reps = int(args[1]) if len(args) > 1 else 10
n_samples = int(args[2]) if len(args) > 2 else 2000
out_path = args[3] if len(args) > 3 else os.path.join(ROOT, "profiles", "surrogate_bench.txt")
arch = "resnet101"
SHAPES = ((64, 1), (330, 5), (330, 1000))
BLOCKS = {64: (8, 8), 330: (15, 22)}
dev = torch.device("cuda", 0)
lines = []


def say(text):
    lines.append(text)
    sys.stdout.write(text + "\n")
    sys.stdout.flush()


def block_segments(rows, cols):
    r, c = np.arange(224) * rows // 224, np.arange(224) * cols // 224
    return (r[:, None] * cols + c[None, :]).astype(np.int32)


def lime_rows(m, s, seed):
    """masks.lime_onoff's draws, restated so that the baseline mode runs on a checkout that has no such function."""
    out = np.random.default_rng(seed).integers(0, 2, size=(m, s), dtype=np.uint8)
    out[0] = 1
    return out


def timed(fn, n=reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def wall(fn, n=3):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


eng = MaskedForwardEngine(arch, max_batch=batch, device=0).load_state_dict(synth.make_state_dict(arch))
img_np = synth.make_images(1, seed=3, kind="noise")[0]
label = eng.predict(img_np)[0]
seg330 = block_segments(*BLOCKS[330])
onoff330 = lime_rows(n_samples, 330, 0)


def score_masks_rows_per_s():
    t = [wall(lambda: eng.score_masks(img_np, seg330, onoff330, label)) for _ in range(2)]
    return [n_samples / v for v in t]


if baseline:
    r = score_masks_rows_per_s()
    say("%s engine, max_batch %d: score_masks on %d rows of S = 330 (%s staging), wall clock, 3 calls per figure, two rounds:"
        % (arch, batch, n_samples, eng.stem_for_rows(n_samples)))
    say("score_masks %.0f %.0f rows/s" % (r[0], r[1]))
else:
    from network_interpretation_imagenet_amd import masks  # noqa: E402

    assert (masks.lime_onoff(n_samples, 330, 0) == onoff330).all()
    say("%s engine, %d rows per chunk, %d timed calls per figure; ms per call, two alternating rounds each (device events)" % (arch, batch, reps))
    say("%-30s %5s %5s %10s %10s %12s %12s %10s" % ("entry", "S", "K", "sums #1", "sums #2", "forward #1", "forward #2", "sums / fwd"))
    labels = torch.zeros(batch, dtype=torch.int32, device=dev)
    img_d = eng._image_to_device(img_np)
    for s, k in SHAPES:
        seg_d = torch.from_numpy(block_segments(*BLOCKS[s])).to(dev)
        onoff = lime_rows(batch, s, s)
        onoff_d = torch.from_numpy(onoff).to(dev)
        w_d = torch.from_numpy(masks.lime_weights(onoff)).to(dev)
        cls_d = None if k == 1000 else torch.arange(k, dtype=torch.int32, device=dev)
        scores = torch.empty(batch, k, dtype=torch.float32, device=dev)
        A = torch.zeros(s + 1, s + 1, dtype=torch.float64, device=dev)
        B = torch.zeros(s + 1, k, dtype=torch.float64, device=dev)
        eng.build_stem_table(img_d, seg_d, s)

        def forward():
            eng.apply_stem_table(onoff_d, 0)
            eng.class_scores(eng.forward(batch, labels, want_logits=True)[2], cls_d, out=scores)

        def sums():
            eng.surrogate_accumulate(onoff_d, w_d, scores, A, B)

        t = [timed(sums), timed(forward), timed(sums), timed(forward)]
        say("%-30s %5d %5d %10.3f %10.3f %12.3f %12.3f %9.2f%%" % ("mpx_surrogate_accumulate", s, k, t[0], t[2], t[1], t[3],
                                                                 100.0 * (t[0] + t[2]) / (t[1] + t[3])))
    say("(forward = mpx_stem_table_apply + mpx_forward with the logits + mpx_softmax_gather_classes of the same chunk)")
    say("")
    out = torch.zeros(5, 224, 224, dtype=torch.float32, device=dev)
    cls = masks.top_classes(eng.score_masks(img_np, seg330, onoff330[:1], 0, return_logits=True)[3][0], 5)
    r_lime = [n_samples / wall(lambda: eng.lime(img_np, seg330, classes=cls, n_samples=n_samples, out=out)) for _ in range(2)]
    r_score = score_masks_rows_per_s()
    r_shap = [(n_samples + 2) / wall(lambda: eng.kernel_shap(img_np, seg330, classes=cls, n_samples=n_samples, out=out)) for _ in range(2)]
    say("end to end on %d rows of S = 330, K = 5 (%s staging), wall clock, 3 calls per figure, two rounds each, rows/s:"
        % (n_samples, eng.stem_for_rows(n_samples)))
    say("lime %.0f %.0f   kernel_shap %.0f %.0f   score_masks (one class, this tree) %.0f %.0f   lime / score_masks %.3f"
        % (r_lime[0], r_lime[1], r_shap[0], r_shap[1], r_score[0], r_score[1], sum(r_lime) / sum(r_score)))
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write(text)
eng.close()
