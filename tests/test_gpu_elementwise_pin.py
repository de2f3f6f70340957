"""The templated element-wise kernels keep their bits (pytest -m gpu): every case of tests/elementwise_pin.py, replayed through the public
entries, gives the sha256 of its output hi and lo plane that tests/golden/elementwise_digests.json recorded with the per-network copies of
these kernels, before they were folded into templates.  Exact: a digest has no tolerance."""
import json
import os

import pytest
import torch

import elementwise_pin as pin
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine

pytestmark = pytest.mark.gpu

FAMILIES = ("dw", "dwact", "gap", "maxpool", "ln")


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "elementwise_digests.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def engine(mpx_lib):
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = MaskedForwardEngine("resnet18", max_batch=4, device=0)
    yield e
    e.close()


def test_pin_inputs_and_cases_are_the_recorded_ones(golden):
    assert pin.inputs_digest() == golden["inputs"], "the input generator drifted: the digests below would speak of other inputs"
    assert sorted(golden["cases"]) == sorted(cid for _, cid, _ in pin.cases())


@pytest.mark.parametrize("family", FAMILIES)
def test_elementwise_bits_are_the_recorded_ones(engine, golden, family):
    mine = [(cid, a) for f, cid, a in pin.cases() if f == family]
    assert mine
    bad = [cid for cid, a in mine if pin.run(engine, family, cid, a) != golden["cases"][cid]]
    print("%s: %d cases, %d differ (library compiled here; digests recorded with %s)" % (family, len(mine), len(bad), golden["hipcc"]))
    assert not bad, "%d of %d cases changed bits: %s" % (len(bad), len(mine), ", ".join(bad))
