#!/usr/bin/env python3
"""The bits of the templated element-wise kernels as a fixture: tests/golden/elementwise_digests.json.  Needs an MI355X.

For every case of tests/elementwise_pin.py -- the public entries mpx_dwconv3x3_bn, mpx_dwconv_bn_act, mpx_global_avgpool / _clamp6 / _silu,
mpx_maxpool2x2s2 / mpx_maxpool3x3s2p0, mpx_layernorm_c / mpx_layernorm_rows on fixed inputs -- this script records the sha256 of the output
hi plane and of the output lo plane, one sha256 over all inputs, and the version of the hipcc that compiled the library.

Recorded ONCE, with the per-network copies of these kernels as they stood before they were folded into templates, and not
regenerated while they were folded: the file is the proof that the fold changed no bit.  tests/test_gpu_elementwise_pin.py replays the cases.
    python tests/golden/make_elementwise_digests.py [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, ".."))
import __graft_entry__ as g  # noqa: E402

g.build()
import elementwise_pin as pin  # noqa: E402
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine  # noqa: E402

PATH = os.path.join(HERE, "elementwise_digests.json")


def hipcc_version():
    try:
        text = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True, text=True).stdout
        return next(line.strip() for line in text.splitlines() if "HIP version" in line)
    except (OSError, StopIteration):
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=PATH)
    args = ap.parse_args()
    eng = MaskedForwardEngine("resnet18", max_batch=4, device=0)
    out = {"hipcc": hipcc_version(), "inputs": pin.inputs_digest(), "cases": {}}
    for family, case_id, a in pin.cases():
        out["cases"][case_id] = pin.run(eng, family, case_id, a)
    eng.close()
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("wrote", args.out, len(out["cases"]), "cases,", os.path.getsize(args.out), "bytes;", out["hipcc"])


if __name__ == "__main__":
    sys.exit(main())
