#!/usr/bin/env python3
"""LIME and KernelSHAP on the superpixels of one synthetic image, scored by the deletion / insertion curves next to RISE.

    python examples/lime_shap_demo.py [arch] [n_samples]

Both explainers fit a linear surrogate of the predicted class's score to random on/off rows over the felzenszwalb superpixels: the rows
run at full batch, their moment sums are accumulated on the device in fp64 and one small system is solved on the host.  sal[0] paints the
coefficients (LIME) or the Shapley values (KernelSHAP) onto the pixels; out= keeps it on the device, where deletion_insertion takes it as
it takes a RISE map.
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
n_samples = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
img = synth.make_images(1, seed=1234)[0]
model = MaskedForwardEngine(arch, max_batch=256).load_state_dict(synth.make_state_dict(arch))
label = model.predict(img)[0]
segments = api.default_segmenter(img)
sal = torch.empty(1, 224, 224, dtype=torch.float32, device=model.device)


def curves(name, seconds):
    res = api.deletion_insertion(model, img, sal[0], label)
    print("%-11s %.3f s: deletion AUC %.4f, insertion AUC %.4f" % (name, seconds, res["del_auc"], res["ins_auc"]))


t0 = time.perf_counter()
_cls, intercept, coef, _sal = api.lime_saliency(model, img, label=label, segments=segments, n_samples=n_samples, out=sal)
torch.cuda.synchronize()
t_lime = time.perf_counter() - t0
print("%s, class %d, %d superpixels, %d rows" % (arch, label, coef.shape[1], n_samples))
print("LIME: intercept %.5f, largest coefficient %.5f on superpixel %d" % (intercept[0], coef[0].max(), int(coef[0].argmax())))
curves("LIME", t_lime)

t0 = time.perf_counter()
n_shap = max(n_samples, coef.shape[1] + coef.shape[1] % 2)
_cls, base, phi, _sal = api.kernel_shap_saliency(model, img, label=label, segments=segments, n_samples=n_shap + n_shap % 2, out=sal)
torch.cuda.synchronize()
t_shap = time.perf_counter() - t0
print("KernelSHAP: base %.5f + sum(phi) %.5f = the unmasked score %.5f" % (base[0], phi[0].sum(), base[0] + phi[0].sum()))
curves("KernelSHAP", t_shap)

t0 = time.perf_counter()
api.rise_saliency(model, img, label, n_masks=n_samples, s=7, out=sal[0])
torch.cuda.synchronize()
curves("RISE", time.perf_counter() - t0)
model.close()
