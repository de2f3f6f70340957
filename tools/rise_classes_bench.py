#!/usr/bin/env python3
"""Time the many-class RISE entries against the single-class entries they restate, on a ResNet-101 engine, in one process:
mpx_rise_saliency_classes (s = 7 and s = 32) against K consecutive mpx_rise_saliency calls, mpx_softmask_saliency_classes against K
consecutive mpx_softmask_saliency calls, mpx_softmax_gather_classes against mpx_head_softmax_gather, for K = 1, 5, 16, 100, 1000, and
rise_saliency_classes(top=5) end to end against 5 x rise_saliency.  The yardstick is always the existing entry; new and old alternate
(new, old, new, old) and both rounds are printed.
usage: python tools/rise_classes_bench.py [batch=2340] [reps=10] [out=profiles/rise_classes_bench.txt]"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

g.build()
from network_interpretation_imagenet_amd import _lib, masks, synth  # noqa: E402
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine  # noqa: E402

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 2340
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "rise_classes_bench.txt")
arch = "resnet101"
KS = (1, 5, 16, 100, 1000)
dev = torch.device("cuda", 0)
eng = MaskedForwardEngine(arch, max_batch=batch, device=0).load_state_dict(synth.make_state_dict(arch))
img_np = synth.make_images(1, seed=3, kind="noise")[0]
grids = {}
for s in (7, 32):
    cells, shifts = masks.rise_masks(batch, s, 0.5, seed=s)
    grids[s] = torch.from_numpy(cells).to(dev), torch.from_numpy(shifts).to(dev)
weights = torch.from_numpy(masks.rise_weights(*masks.rise_masks(batch, 7, 0.5, seed=7), 7)).to(dev)
scores = torch.rand(batch, 1000, dtype=torch.float32, device=dev)           # [M, K]: the new entries' rows
scores_t = scores.t().contiguous()                                          # [K, M]: one weight vector per class for the old entries
sal = torch.zeros(1000, 224, 224, dtype=torch.float32, device=dev)
logits = (torch.rand(batch, 1000, dtype=torch.float32, device=dev) - 0.5) * 40.0
labels = torch.zeros(batch, dtype=torch.int32, device=dev)
score1 = torch.empty(batch, dtype=torch.float32, device=dev)
pred1 = torch.empty(batch, dtype=torch.int32, device=dev)
gathered = torch.empty(batch, 1000, dtype=torch.float32, device=dev)
lines = []


def say(text):
    lines.append(text)
    sys.stdout.write(text + "\n")
    sys.stdout.flush()


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


def alternate(new, old):
    """(new, old, new, old) -> the two rounds of each, in ms per call."""
    t = [timed(new), timed(old), timed(new), timed(old)]
    return (t[0], t[2]), (t[1], t[3])


def row(name, k, new, old):
    n, o = sum(new) / 2, sum(old) / 2
    say("%-34s %5d %10.3f %10.3f %11.3f %11.3f %9.2f" % (name, k, new[0], new[1], old[0], old[1], o / n))
    return n, o


say("%s engine, %d masks per call, %d timed calls per figure, class tile %d; ms per call, two alternating rounds each"
    % (arch, batch, reps, _lib.SALIENCY_CLASS_TILE))
say("%-34s %5s %10s %10s %11s %11s %9s" % ("entry (new vs K x old)", "K", "new #1", "new #2", "K x old #1", "K x old #2", "old / new"))
floor_note = {}
for s in (7, 32):
    c, sh = grids[s]
    for k in KS:
        def new():
            eng.rise_saliency_accumulate_classes(c, sh, s, scores[:, :k], sal[:k])

        def old():
            for j in range(k):
                eng.rise_saliency_accumulate(c, sh, s, scores_t[j], sal[j])

        floor_note[(s, k)] = row("mpx_rise_saliency_classes s=%d" % s, k, *alternate(new, old))
        sal.zero_()
for k in KS:
    def new():
        eng.soft_saliency_accumulate_classes(weights, scores[:, :k], sal[:k])

    def old():
        for j in range(k):
            eng.soft_saliency_accumulate(weights, scores_t[j], sal[j])

    row("mpx_softmask_saliency_classes", k, *alternate(new, old))
    sal.zero_()

say("")
say("%-34s %5s %10s %10s %11s %11s %9s" % ("head, B=%d (new vs K x old)" % batch, "K", "new #1", "new #2", "K x old #1", "K x old #2", "old / new"))
for k in KS:
    cls = None if k == 1000 else torch.arange(k, dtype=torch.int32, device=dev)

    def new():
        eng.class_scores(logits, cls, out=gathered[:, :k])

    def old():
        for _ in range(k):
            _lib.check(eng._h, eng._lib.mpx_head_softmax_gather(eng._h, logits.data_ptr(), labels.data_ptr(), score1.data_ptr(),
                                                                pred1.data_ptr(), batch, eng._stream()), "mpx_head_softmax_gather")

    row("mpx_softmax_gather_classes", k, *alternate(new, old))


def wall(fn, n=reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


say("")
top5, _ = eng.rise_saliency_classes(img_np, top=5, n_masks=batch, s=7, out=sal[:5])
one = torch.zeros(224, 224, dtype=torch.float32, device=dev)


def e2e_new():
    eng.rise_saliency_classes(img_np, top=5, n_masks=batch, s=7, out=sal[:5])


def e2e_old():
    for c in top5:
        eng.rise_saliency(img_np, int(c), n_masks=batch, s=7, out=one)


t = [wall(e2e_new), wall(e2e_old), wall(e2e_new), wall(e2e_old)]
say("end to end, n_masks=%d, s=7, wall clock with the mask draws and uploads, ms per call (new, old, new, old):" % batch)
say("rise_saliency_classes(top=5) %.1f %.1f   5 x rise_saliency %.1f %.1f   old / new %.2f"
    % (t[0], t[2], t[1], t[3], (t[1] + t[3]) / (t[0] + t[2])))
n1000 = {s: floor_note[(s, 1000)][0] for s in (7, 32)}
say("")
say("K=1000: %.2f ms (s=7), %.2f ms (s=32) against a DERIVED floor of about 6 ms (one multiply and one add per class, mask and pixel at the"
    % (n1000[7], n1000[32]))
say("fp32 vector peak) or about 3 ms with packed fp32 operations; the floor is arithmetic, not a measurement.")
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write(text)
eng.close()
