#!/usr/bin/env python3
"""The layer plan of every served architecture as a fixture: tests/golden/plan_digests.json.

mpx_describe_plan (include/mpx.h) prints the plan build_topology makes for an arch id -- host data, no GPU.  This script records, for
each name of engine.ARCH_IDS, the number of records and a sha256 per section of that text (tests/plan_text.py), so that a change of the
builders that moves any field of any layer fails tests/test_plan_cpu.py with the architecture and the section in the message.

Recorded ONCE, with the per-family builders as they stood before they were folded into one PlanBuilder, and not
regenerated while they were folded: the file is the proof that the fold changed no plan.  A new architecture appends its row:
    python tests/golden/make_plan_digests.py --only NAME [NAME ...]
With --dump DIR the full texts are written to DIR/<name>.txt as well (to diff by hand; not committed).
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, ".."))
import __graft_entry__ as g  # noqa: E402

g.compile_only()
import plan_text  # noqa: E402
from network_interpretation_imagenet_amd import _lib  # noqa: E402
from network_interpretation_imagenet_amd.engine import ARCH_IDS  # noqa: E402

PATH = os.path.join(HERE, "plan_digests.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", help="record these architectures only and keep every other row of the file")
    ap.add_argument("--dump", help="directory for the full texts")
    args = ap.parse_args()
    lib = _lib.load()
    out = {}
    if args.only:
        with open(PATH) as fh:
            out = json.load(fh)
    for name in args.only or sorted(ARCH_IDS):
        rc, text = plan_text.describe(lib, ARCH_IDS[name])
        assert rc == 0, (name, rc)
        out[name] = plan_text.digests(text)
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            with open(os.path.join(args.dump, name + ".txt"), "w") as fh:
                fh.write(text)
        print("%-20s %6d bytes  %s" % (name, len(text), " ".join("%s=%d" % (s, d["n"]) for s, d in out[name].items() if d["n"])))
    with open(PATH, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    sys.exit(main())
