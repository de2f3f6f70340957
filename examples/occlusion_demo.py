#!/usr/bin/env python3
"""Occlusion sensitivity on one synthetic image, scored by the deletion / insertion curves next to RISE.

    python examples/occlusion_demo.py [arch] [window] [stride]

A window x window box slides over the image by `stride`; every pixel gets the mean drop of the class score over the boxes that cover it
(Zeiler & Fergus, ECCV 2014).  The occluded images are never built: the apply kernel compares every pixel against its row's box, and the
overlap mean runs on the device.  The map is computed twice -- the box covered with the mean colour, and with the blurred image -- and
out= keeps it on the device, where deletion_insertion takes it as it takes a RISE map.
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
window = int(sys.argv[2]) if len(sys.argv) > 2 else 32
stride = int(sys.argv[3]) if len(sys.argv) > 3 else 16
img = synth.make_images(1, seed=1234)[0]
model = MaskedForwardEngine(arch, max_batch=256).load_state_dict(synth.make_state_dict(arch))
label = model.predict(img)[0]
rows = len(masks.occlusion_boxes(window, stride)) + 1
sal = torch.empty(1, 224, 224, dtype=torch.float32, device=model.device)
print("%s, class %d, window %d, stride %d, %d rows" % (arch, label, window, stride, rows))


def curves(name, seconds):
    res = api.deletion_insertion(model, img, sal[0], label)
    print("%-18s %.3f s: deletion AUC %.4f, insertion AUC %.4f" % (name, seconds, res["del_auc"], res["ins_auc"]))


for name, fill in (("occlusion (mean)", None), ("occlusion (blur)", "blur")):
    t0 = time.perf_counter()
    _cls, base, scores, _sal = api.occlusion_saliency(model, img, label=label, window=window, stride=stride, fill=fill, out=sal)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    drop = (base[0] - scores[:, 0]).cpu().numpy()
    y0, x0, y1, x1 = masks.occlusion_boxes(window, stride)[int(drop.argmax())]
    print("%s: score %.4f, largest drop %.4f under the box [%d:%d, %d:%d]" % (name, float(base[0]), drop.max(), y0, y1, x0, x1))
    curves(name, seconds)

t0 = time.perf_counter()
api.rise_saliency(model, img, label, n_masks=rows, s=7, out=sal[0])
torch.cuda.synchronize()
curves("RISE", time.perf_counter() - t0)
model.close()
