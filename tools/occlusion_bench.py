#!/usr/bin/env python3
"""Time the occlusion-sensitivity path on a ResNet-50 engine, in one process:
  1. mpx_box_apply without and with a fill image next to mpx_softmask_apply on the SAME rows' explicit weights (masks.box_weights) and
     next to mpx_mask_apply_normalize (K0, S = 196: the same bytes written, the yardstick) -- `batch` rows per call, device events,
     `runs` alternating runs of `reps` calls each; the median and the run-to-run spread (slowest - fastest run) of every entry;
  2. mpx_box_saliency_classes and mpx_box_saliency_mean at R = 169, K = 5 (window 32, stride 16, the five largest logits) and at
     R = 729, K = 1000 (window 16, stride 8, every class), on random scores;
  3. occlusion(top=5) end to end at window 32 / stride 16 (170 rows) and window 16 / stride 8 (730 rows) in rows/s (wall clock around a
     synchronise: the boxes' upload, the forwards, the class scores, the overlap mean, out= on the device) next to the plain forward rate
     of the same process.
The one condition the code implies is checked and printed: the box source reads 200 KB per row less than the explicit source and writes
the same bytes, so its median must not exceed the explicit entry's median by more than the run-to-run spread.
usage: python tools/occlusion_bench.py [batch=1024] [reps=50] [runs=5] [out=profiles/occlusion_bench.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

g.build()
from network_interpretation_imagenet_amd import masks, synth  # noqa: E402
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine  # noqa: E402

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "occlusion_bench.txt")
arch = "resnet50"
dev = torch.device("cuda", 0)
eng = MaskedForwardEngine(arch, max_batch=batch, device=0).load_state_dict(synth.make_state_dict(arch))
img_np = synth.make_images(1, seed=3, kind="noise")[0]
img = torch.from_numpy(img_np).to(dev)
seg_np = synth.grid_segments()
S = int(seg_np.max()) + 1
seg = torch.from_numpy(seg_np).to(dev)
onoff = torch.from_numpy(synth.random_onoff(batch, S)).to(dev)
job = np.concatenate([np.zeros((1, 4), dtype=np.int32), masks.occlusion_boxes(32, 16)])        # occlusion()'s rows, repeated to `batch`
boxes_np = np.ascontiguousarray(job[np.arange(batch) % len(job)])
boxes = torch.from_numpy(boxes_np).to(dev)
weights = torch.from_numpy(masks.box_weights(boxes_np)).to(dev)             # batch x 200 KB: what the source saves
fill = eng.blur_fill(img)
labels = torch.zeros(batch, dtype=torch.int32, device=dev)
score = torch.empty(batch, dtype=torch.float32, device=dev)
pred = torch.zeros(batch, dtype=torch.int32, device=dev)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(entries):
    """Every run times every entry once, in order: -> {name: [ms per call of run 1, run 2, ..]}."""
    times = {name: [] for name, _fn in entries}
    for _ in range(runs):
        for name, fn in entries:
            times[name].append(timed(fn))
    return times


def table(entries, times, ref=None):
    rows = ["%-46s %s %9s %9s %7s" % ("entry", " ".join("%9s" % ("run %d" % (i + 1)) for i in range(runs)), "median", "spread",
                                      "x K0" if ref else "")]
    for name, _fn in entries:
        t = times[name]
        rows.append("%-46s %s %9.5f %9.5f %7s" % (name, " ".join("%9.5f" % v for v in t), np.median(t), max(t) - min(t),
                                                  "%.3f" % (np.median(t) / np.median(times[ref])) if ref else ""))
    return rows


apply_entries = [("mpx_mask_apply_normalize (K0, S=%d)" % S, lambda: eng.stage_masks(img, seg, onoff, 0)),
                 ("mpx_softmask_apply (box_weights)", lambda: eng.stage_soft_masks(img, weights, 0)),
                 ("mpx_box_apply", lambda: eng.stage_boxes(img, boxes, 0)),
                 ("mpx_box_apply, fill", lambda: eng.stage_boxes(img, boxes, 0, fill=fill))]
apply_times = alternate(apply_entries)
t_fwd = timed(lambda: eng.forward(batch, labels, score_out=score, pred_out=pred))       # over the slots staged last
lines = ["%s, %d rows per call, %d runs of %d timed calls each, alternating; ms per call (device events); one forward batch of %d: %.3f ms"
         % (arch, batch, runs, reps, batch, t_fwd)]
lines += table(apply_entries, apply_times, ref=apply_entries[0][0])
box, soft = apply_times["mpx_box_apply"], apply_times["mpx_softmask_apply (box_weights)"]
spread = max(max(box) - min(box), max(soft) - min(soft))
lines.append("condition: median of mpx_box_apply (%.5f ms) <= median of mpx_softmask_apply (%.5f ms) + run-to-run spread (%.5f ms): %s"
             % (np.median(box), np.median(soft), spread, "holds" if np.median(box) <= np.median(soft) + spread else "FAILS"))
lines.append("cost of the fill: %+.5f ms per call" % (np.median(apply_times["mpx_box_apply, fill"]) - np.median(box)))

lines.append("")
lines.append("the overlap mean on random scores; ms per call")
sal_entries = []
for window, stride, k in ((32, 16, 5), (16, 8, 1000)):
    b_np = masks.occlusion_boxes(window, stride)
    r = len(b_np)
    b_d = torch.from_numpy(b_np).to(dev)
    sc = torch.rand(r + 1, k, dtype=torch.float32, device=dev)
    s_d = torch.zeros(k, 224, 224, dtype=torch.float32, device=dev)
    c_d = torch.zeros(224, 224, dtype=torch.int32, device=dev)
    o_d = torch.empty_like(s_d)
    sal_entries.append(("mpx_box_saliency_classes R=%d K=%d" % (r, k),
                        lambda b_d=b_d, sc=sc, s_d=s_d, c_d=c_d: eng.occlusion_accumulate(b_d, sc[1:], sc[0], s_d, c_d)))
    sal_entries.append(("mpx_box_saliency_mean K=%d" % k, lambda s_d=s_d, c_d=c_d, o_d=o_d: eng.occlusion_mean(s_d, c_d, out=o_d)))
lines += table(sal_entries, alternate(sal_entries))


def wall(fn, n=3):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


lines.append("")
out = torch.zeros(5, 224, 224, dtype=torch.float32, device=dev)
for window, stride in ((32, 16), (16, 8)):
    rows = len(masks.occlusion_boxes(window, stride)) + 1
    rate = [rows / wall(lambda: eng.occlusion(img_np, top=5, window=window, stride=stride, out=out)) for _ in range(2)]
    lines.append("occlusion(top=5, window=%d, stride=%d): %d rows, wall clock, 3 calls per figure, two rounds: %.0f %.0f rows/s"
                 % (window, stride, rows, rate[0], rate[1]))
lines.append("the plain forward of %d staged rows: %.0f rows/s" % (batch, batch / t_fwd * 1e3))
text = "\n".join(lines) + "\n"
sys.stdout.write(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write(text)
eng.close()
