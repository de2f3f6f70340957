#!/usr/bin/env python3
"""Sobol total-order indices over a grid of cells on one synthetic image, scored by the deletion / insertion curves next to RISE.

    python examples/sobol_demo.py [arch] [grid] [n_design]

Every cell of the grid x grid grid gets a weight in [0, 1] from a scrambled Sobol design; the n_design * (grid^2 + 1) perturbed images are
never built: the apply kernel gathers each row's weights from the two design matrices.  A cell's index is the share of the class score's
variance that involves it, interactions with other cells included.  The map is computed twice -- cells pulled towards zero, and towards the
blurred image (the paper's second perturbation) -- and out= keeps it on the device, where deletion_insertion takes it as it takes a RISE map.
"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

g.build()
from network_interpretation_imagenet_amd import api, masks, synth  # noqa: E402
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine  # noqa: E402

arch = sys.argv[1] if len(sys.argv) > 1 else "resnet18"
grid = int(sys.argv[2]) if len(sys.argv) > 2 else 8
n_design = int(sys.argv[3]) if len(sys.argv) > 3 else 32
img = synth.make_images(1, seed=1234)[0]
model = MaskedForwardEngine(arch, max_batch=256).load_state_dict(synth.make_state_dict(arch))
label = model.predict(img)[0]
rows = masks.sobol_rows(n_design, grid)
sal = torch.empty(1, 224, 224, dtype=torch.float32, device=model.device)
print("%s, class %d, %d x %d cells, %d designs, %d rows" % (arch, label, grid, grid, n_design, rows))


def curves(name, seconds):
    res = api.deletion_insertion(model, img, sal[0], label)
    print("%-14s %.3f s: deletion AUC %.4f, insertion AUC %.4f" % (name, seconds, res["del_auc"], res["ins_auc"]))


for name, fill in (("Sobol (zero)", None), ("Sobol (blur)", "blur")):
    t0 = time.perf_counter()
    _cls, st, _sal = api.sobol_saliency(model, img, label=label, grid=grid, n_design=n_design, fill=fill, out=sal)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    y, x = divmod(int(st[0].argmax()), grid)
    print("%s: largest total-order index %.4f at cell (%d, %d), sum of the indices %.3f" % (name, st[0].max(), y, x, st[0].sum()))
    curves(name, seconds)

t0 = time.perf_counter()
api.rise_saliency(model, img, label, n_masks=rows, s=7, out=sal[0])
torch.cuda.synchronize()
curves("RISE", time.perf_counter() - t0)
model.close()
