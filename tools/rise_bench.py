#!/usr/bin/env python3
"""Time the real-valued mask entries against their binary counterparts on a ResNet-101 engine, in one process:
mpx_rise_apply (s = 7 and s = 32) and mpx_softmask_apply against mpx_mask_apply_normalize (K0 writes the same bytes: the yardstick),
mpx_rise_saliency and mpx_softmask_saliency against mpx_heatmap_accumulate, and each as a share of one forward batch.
usage: python tools/rise_bench.py [batch=2340] [reps=10] [out=profiles/rise_bench.txt]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

g.build()
from network_interpretation_imagenet_amd import masks, synth  # noqa: E402
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine  # noqa: E402

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 2340
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "rise_bench.txt")
arch = "resnet101"
dev = torch.device("cuda", 0)
eng = MaskedForwardEngine(arch, max_batch=batch, device=0).load_state_dict(synth.make_state_dict(arch))
img = torch.from_numpy(synth.make_images(1, seed=3, kind="noise")[0]).to(dev)
seg_np = synth.grid_segments()
S = int(seg_np.max()) + 1
seg = torch.from_numpy(seg_np).to(dev)
onoff = torch.from_numpy(synth.random_onoff(batch, S)).to(dev)
grids = {}
for s in (7, 32):
    cells, shifts = masks.rise_masks(batch, s, 0.5, seed=s)
    grids[s] = torch.from_numpy(cells).to(dev), torch.from_numpy(shifts).to(dev)
weights = torch.from_numpy(masks.rise_weights(*masks.rise_masks(batch, 7, 0.5, seed=7), 7)).to(dev)       # batch x 200 KB, what RISE saves
labels = torch.zeros(batch, dtype=torch.int32, device=dev)
score = torch.rand(batch, dtype=torch.float32, device=dev)
pred = torch.zeros(batch, dtype=torch.int32, device=dev)
sal = torch.zeros(224, 224, dtype=torch.float32, device=dev)


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


plane_bytes = batch * 230 * 230 * 4 * 2 * 2          # what every apply launch writes: both padded NHWC4 fp16 planes of every slot
rows = []
t_k0 = timed(lambda: eng.stage_masks(img, seg, onoff, 0))
t_fwd = timed(lambda: eng.forward(batch, labels, score_out=score, pred_out=pred))       # over the slots K0 just staged
rows.append(("mpx_mask_apply_normalize (K0, S=%d)" % S, t_k0, t_k0, plane_bytes))
for s in (7, 32):
    c, sh = grids[s]
    rows.append(("mpx_rise_apply s=%d" % s, timed(lambda: eng.stage_rise(img, c, sh, s, 0)), t_k0, plane_bytes))
rows.append(("mpx_softmask_apply", timed(lambda: eng.stage_soft_masks(img, weights, 0)), t_k0, plane_bytes + weights.numel() * 4))
score.uniform_()
t_heat = timed(lambda: eng.heatmap_accumulate(seg, onoff, pred, labels, sal))
rows.append(("mpx_heatmap_accumulate (K5, S=%d)" % S, t_heat, t_heat, 0))
for s in (7, 32):
    c, sh = grids[s]
    rows.append(("mpx_rise_saliency s=%d" % s, timed(lambda: eng.rise_saliency_accumulate(c, sh, s, score, sal)), t_heat, 0))
rows.append(("mpx_softmask_saliency", timed(lambda: eng.soft_saliency_accumulate(weights, score, sal)), t_heat, weights.numel() * 4))

lines = ["%s, %d masks per call, %d timed calls each; one forward batch of %d: %.3f ms" % (arch, batch, reps, batch, t_fwd),
         "%-40s %9s %12s %10s %10s" % ("entry", "ms", "x yardstick", "GB/s", "% forward")]
for name, ms, ref, nbytes in rows:
    lines.append("%-40s %9.3f %12.2f %10s %10.2f" % (name, ms, ms / ref, ("%.0f" % (nbytes / ms * 1e-6)) if nbytes else "-", 100.0 * ms / t_fwd))
text = "\n".join(lines) + "\n"
sys.stdout.write(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write(text)
eng.close()
