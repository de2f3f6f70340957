"""The layer plan of every architecture, on the CPU: mpx_describe_plan (include/mpx.h) runs the build_topology that mpx_create runs and
prints what it made, and tests/golden/plan_digests.json pins that text section by section -- recorded with the per-family builders before
they were folded into one PlanBuilder (tests/golden/make_plan_digests.py).  No GPU anywhere in this file."""
import ctypes as C
import json
import os

import pytest

import plan_text
from network_interpretation_imagenet_amd.engine import ARCH_IDS

MPX_E_ARG = -1


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "plan_digests.json")) as fh:
        return json.load(fh)


def test_every_architecture_has_the_recorded_plan(mpx_lib, golden):
    assert sorted(golden) == sorted(ARCH_IDS), "tests/golden/plan_digests.json does not list exactly the architectures of ARCH_IDS"
    wrong = []
    for arch in sorted(ARCH_IDS):
        rc, text = plan_text.describe(mpx_lib, ARCH_IDS[arch])
        assert rc == 0, "mpx_describe_plan(%s) returned %d" % (arch, rc)
        got = plan_text.digests(text)
        assert sorted(got) == sorted(golden[arch]) == sorted(plan_text.SECTIONS), arch
        for section in plan_text.SECTIONS:
            if got[section] != golden[arch][section]:
                wrong.append("%s: section %s: %d records, recorded %d%s" % (
                    arch, section, got[section]["n"], golden[arch][section]["n"],
                    "" if got[section]["n"] != golden[arch][section]["n"] else " (the same number, another sha256)"))
    assert not wrong, "the plan differs from tests/golden/plan_digests.json:\n" + "\n".join(wrong)


def test_the_text_is_records_of_known_sections(mpx_lib):
    rc, text = plan_text.describe(mpx_lib, ARCH_IDS["resnet101"])
    assert rc == 0 and text.endswith("\n") and "0x" not in text
    sec = plan_text.by_section(text)
    # (105 convs, four op lists, 3 block tails and 2 pointwise tails)
    assert [len(sec[s]) for s in ("engine", "conv", "ops", "ops_bt", "ops_pt", "ops_pt0", "tail", "ptail")] == [1, 105, 108, 100, 98, 106, 3, 2]
    order = [line.split(" ", 1)[0] for line in text.splitlines()]
    assert sorted(order, key=plan_text.SECTIONS.index) == order, "the sections come in the order of include/mpx.h"
    conv = plan_text.records(sec["conv"])
    assert conv[0]["name"] == "conv1" and conv[0]["is_stem"] == "1" and conv[-1]["name"] == "fc" and conv[-1]["is_fc"] == "1"
    assert plan_text.describe(mpx_lib, ARCH_IDS["resnet101"])[1] == text, "deterministic"


def test_length_idiom_and_small_buffer(mpx_lib):
    arch = ARCH_IDS["mnist_net"]
    n = C.c_size_t(12345)
    assert mpx_lib.mpx_describe_plan(arch, None, 0, C.byref(n)) == 0 and 0 < n.value < 12345
    need = n.value
    assert mpx_lib.mpx_describe_plan(arch, None, 0, None) == MPX_E_ARG
    for cap in (0, 1, need - 1, need):          # the NUL does not fit: nothing is written, the length still is
        buf = C.create_string_buffer(b"\x55" * (need + 8), need + 8)
        n = C.c_size_t(0)
        assert mpx_lib.mpx_describe_plan(arch, buf, cap, C.byref(n)) == MPX_E_ARG, cap
        assert n.value == need and buf.raw == b"\x55" * (need + 8), cap
    buf = C.create_string_buffer(b"\x55" * (need + 8), need + 8)
    n = C.c_size_t(0)
    assert mpx_lib.mpx_describe_plan(arch, buf, need + 1, C.byref(n)) == 0 and n.value == need
    assert len(buf.value) == need and buf.raw[need] == 0 and buf.raw[need + 1:] == b"\x55" * 7, "writes the text and its NUL, nothing behind"
    assert buf.value.decode() == plan_text.describe(mpx_lib, arch)[1]


@pytest.mark.parametrize("arch_id", [5161, 7010, 13014, 0, 2021, 3012, 14005, 16000])
def test_an_id_mpx_create_rejects_is_rejected(mpx_lib, arch_id):
    n = C.c_size_t(777)
    buf = C.create_string_buffer(b"\x55" * 64, 64)
    assert mpx_lib.mpx_describe_plan(arch_id, buf, 64, C.byref(n)) == MPX_E_ARG
    assert n.value == 0 and buf.raw == b"\x55" * 64
