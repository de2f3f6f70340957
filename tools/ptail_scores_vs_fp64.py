#!/usr/bin/env python3
"""Are the scores with layer2's pointwise tails (fusion mask 7) further from the truth than without them (mask 3)?  The same masks scored
both ways on the GPU and by the oracle's fp64 forward on the CPU (oracle/scorer.py, score_masks_batched(dtype=float64)).
usage: python tools/ptail_scores_vs_fp64.py [arch] [masks]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

g.build()
from network_interpretation_imagenet_amd import synth  # noqa: E402
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine  # noqa: E402
from oracle import scorer  # noqa: E402

arch = sys.argv[1] if len(sys.argv) > 1 else "resnet101"
m = int(sys.argv[2]) if len(sys.argv) > 2 else 128
sd = synth.make_state_dict(arch)
img = synth.make_images(1, seed=9, kind="noise")[0]
seg = synth.grid_segments()
onoff = synth.random_onoff(m, 196, seed=6)
eng = MaskedForwardEngine(arch, max_batch=m, device=0).load_state_dict(sd)
label, _ = eng.predict(img)
got = {}
for mask in (7, 3):
    eng.set_fusion(mask)
    _o, s, p = eng.score_masks(img, seg, onoff, label)
    got[mask] = (s.astype(np.float64), p)
torch.cuda.synchronize()
eng.close()
ref, ref_p = scorer.score_masks_batched(sd, arch, scorer.to_tensor_normalize(img), seg, onoff, label, dtype=torch.float64)
print("%s, %d masks, label %d, fp64 scores %.4f .. %.4f" % (arch, m, label, ref.min(), ref.max()))
for mask in (7, 3):
    d = np.abs(got[mask][0] - ref)
    print("fusion mask %d against fp64: max %.3e  mean %.3e  rms %.3e  argmax equal %s" % (mask, d.max(), d.mean(), np.sqrt((d * d).mean()), bool((got[mask][1] == ref_p).all())))
d = np.abs(got[7][0] - got[3][0])
print("mask 7 against mask 3:       max %.3e  mean %.3e" % (d.max(), d.mean()))
