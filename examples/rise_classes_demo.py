#!/usr/bin/env python3
"""RISE for the top-k classes of one image in ONE pass over the masks, then the deletion / insertion curves of every map.

    python examples/rise_classes_demo.py [arch] [top] [n_masks]

rise_saliency_classes runs the masked forwards once and weights every mask with the scores of all k classes; map i is what
api.rise_saliency(model, image, classes[i]) returns, bit for bit.  The curves need no entry of their own: deletion_insertion_many takes
the same image k times, each time with the map and the label of one class.
"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

g.build()
from network_interpretation_imagenet_amd import api, synth  # noqa: E402
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine  # noqa: E402

arch = sys.argv[1] if len(sys.argv) > 1 else "resnet18"
top = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n_masks = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
img = synth.make_images(1, seed=1234)[0]
model = MaskedForwardEngine(arch, max_batch=256).load_state_dict(synth.make_state_dict(arch))

t0 = time.perf_counter()
classes, sal = api.rise_saliency_classes(model, img, top=top, n_masks=n_masks, s=7)
torch.cuda.synchronize()
print("%s: %d maps from %d masks in %.3f s; classes %s" % (arch, len(classes), n_masks, time.perf_counter() - t0, classes.tolist()))
curves = api.deletion_insertion_many(model, [img] * len(classes), list(sal), [int(c) for c in classes])
for c, res in zip(classes, curves):
    print("class %4d: deletion AUC %.4f, insertion AUC %.4f" % (c, res["del_auc"], res["ins_auc"]))
model.close()
