"""What mpx_describe_plan prints is what an engine holds (pytest -m gpu): for every architecture, an engine without weights at max_batch 1
reports the conv descriptors, the tiles and the list lengths of the text that tests/test_plan_cpu.py pins on the CPU."""
import pytest

import plan_text
from network_interpretation_imagenet_amd import _lib
from network_interpretation_imagenet_amd.engine import ARCH_IDS, MaskedForwardEngine

pytestmark = pytest.mark.gpu

DESC_INTS = ("cin", "cout", "ksize", "stride", "pad", "hin", "hout", "relu", "residual", "k_packed", "cout_pad")
COUNTS = (("mpx_num_norms", "norm"), ("mpx_num_dwconvs", "dw"), ("mpx_num_se", "se"), ("mpx_num_lnorms", "lnorm"), ("mpx_num_attn", "attn"),
          ("mpx_num_shuffles", "shuffle"), ("mpx_num_clip_pools", "pool3c"), ("mpx_num_bottleneck_tails", "tail"),
          ("mpx_num_pointwise_tails", "ptail"))


def test_an_engine_holds_the_described_plan(mpx_lib):
    wrong, layers = [], 0
    for arch in sorted(ARCH_IDS):
        rc, text = plan_text.describe(mpx_lib, ARCH_IDS[arch])
        assert rc == 0, arch
        sec = plan_text.by_section(text)
        conv = plan_text.records(sec["conv"])
        eng = MaskedForwardEngine(arch, max_batch=1, device=0)
        try:
            h = eng._h
            if mpx_lib.mpx_num_convs(h) != len(conv):
                wrong.append("%s: mpx_num_convs %d, %d conv records" % (arch, mpx_lib.mpx_num_convs(h), len(conv)))
                continue
            for i, rec in enumerate(conv):
                d = _lib.ConvDesc()
                assert mpx_lib.mpx_conv_info(h, i, d) == 0
                got = dict(name=d.name.decode(), bn_name=d.bn_name.decode(), tile=str(mpx_lib.mpx_get_conv_tile(h, i)),
                           **{k: str(getattr(d, k)) for k in DESC_INTS})
                bad = {k: (v, rec[k]) for k, v in got.items() if rec[k] != v}
                if bad:
                    wrong.append("%s: conv %d (engine, text): %r" % (arch, i, bad))
            layers += len(conv)
            for fn, section in COUNTS:
                if getattr(mpx_lib, fn)(h) != len(sec[section]):
                    wrong.append("%s: %s %d, %d %s records" % (arch, fn, getattr(mpx_lib, fn)(h), len(sec[section]), section))
        finally:
            eng.close()
    print("plan: %d architectures, %d conv layers compared, %d differences" % (len(ARCH_IDS), layers, len(wrong)))
    assert not wrong, "\n".join(wrong)
