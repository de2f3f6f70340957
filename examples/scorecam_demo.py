#!/usr/bin/env python3
"""Score-CAM on one synthetic image, scored by the deletion / insertion curves next to RISE and occlusion sensitivity.

    python examples/scorecam_demo.py [arch]

Every channel of the map the network's global pool reads (ResNet-18's layer4: 512 maps of 7 x 7) becomes a mask -- upsampled to the image
inside the apply kernel, normalised to [0, 1] --, the masked images are scored at full batch, and the class activation map is the channels'
sum weighted by those scores (Wang et al., CVPR-W 2020).  One unmasked forward gives the maps; nothing comes down before the end, and
out= keeps the map on the device, where deletion_insertion takes it as it takes a RISE map.
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
img = synth.make_images(1, seed=1234)[0]
model = MaskedForwardEngine(arch, max_batch=256).load_state_dict(synth.make_state_dict(arch))
label = model.predict(img)[0]
sal = torch.empty(1, 224, 224, dtype=torch.float32, device=model.device)


def curves(name, seconds):
    res = api.deletion_insertion(model, img, sal[0], label)
    print("%-18s %.3f s: deletion AUC %.4f, insertion AUC %.4f" % (name, seconds, res["del_auc"], res["ins_auc"]))


t0 = time.perf_counter()
_cls, channels, scores, low, _sal = api.score_cam_saliency(model, img, label=label, out=sal)
torch.cuda.synchronize()
seconds = time.perf_counter() - t0
rows = len(channels)
best = int(scores[:, 0].argmax())
print("%s, class %d: %d channels scored (a flat one is skipped), map %d x %d; best channel %d scores %.4f"
      % (arch, label, rows, low.shape[1], low.shape[2], int(channels[best]), float(scores[best, 0])))
curves("Score-CAM", seconds)

t0 = time.perf_counter()
api.occlusion_saliency(model, img, label=label, window=32, stride=16, out=sal)
torch.cuda.synchronize()
curves("occlusion (mean)", time.perf_counter() - t0)

t0 = time.perf_counter()
api.rise_saliency(model, img, label, n_masks=max(rows, 1), s=7, out=sal[0])
torch.cuda.synchronize()
curves("RISE", time.perf_counter() - t0)
model.close()
