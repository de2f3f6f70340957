"""The arena of every architecture has the size it had before mpx_create's layout was written down once (pytest -m gpu).

workspace_bytes is a function of (arch, max_batch) alone -- no weights, no device property enters it -- so
tests/golden/workspace_bytes.json, recorded with this loop on the commit before the single layout pass, pins every buffer's size and
256-byte rounding: max_batch 2 and 3 separate the per-slot part of the arena from the fixed part (weights, scratch), so a buffer that
changes size in either shows.  An architecture added later needs its two numbers in the file."""
import json
import os

import pytest

from network_interpretation_imagenet_amd.engine import ARCH_IDS, MaskedForwardEngine

pytestmark = pytest.mark.gpu


def test_workspace_bytes_match_the_recorded_layout(mpx_lib, golden_dir):
    with open(os.path.join(golden_dir, "workspace_bytes.json")) as fh:
        want = json.load(fh)
    assert sorted(want) == sorted(ARCH_IDS), "tests/golden/workspace_bytes.json does not list exactly the architectures of ARCH_IDS"
    got = {}
    for arch in sorted(ARCH_IDS):
        got[arch] = {}
        for max_batch in (2, 3):
            eng = MaskedForwardEngine(arch, max_batch=max_batch, device=0)
            got[arch][str(max_batch)] = eng.workspace_bytes
            eng.close()
    diff = {a: (got[a], want[a]) for a in got if got[a] != want[a]}
    print("workspace_bytes: %d architectures x 2 sizes, %d differ from the recorded layout" % (len(got), len(diff)))
    assert not diff, "workspace_bytes (got, recorded): %r" % diff
