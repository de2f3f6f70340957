"""CPU-side checks of the many-class RISE path (csrc/mpx_saliency_classes.h): the numpy restatement of the class-tiled sum against the
single-class emulation column by column, the argument checks and the tie rule of rise_saliency_classes, and the three new entries in the
built library and the ctypes table.  No GPU anywhere in this file."""
import numpy as np
import pytest

from network_interpretation_imagenet_amd import _lib, masks
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine
import rise_ref

NEW_ENTRIES = ("mpx_softmax_gather_classes", "mpx_softmask_saliency_classes", "mpx_rise_saliency_classes")


def test_saliency_sum_classes_is_the_single_class_emulation_per_column():
    """K = 3, M = 5, a nonzero sal0, scores with negatives and both zeros: column k, as int32 bit patterns, is
    rise_ref.saliency_emulation(sal0[k], scores[:, k], w)."""
    k_all, m_all = 3, 5
    cells, shifts = rise_ref.draws(7, m_all, seed=2)
    w = masks.rise_weights(cells, shifts, 7)
    rng = np.random.default_rng(6)
    sal0 = rng.standard_normal((k_all, 224, 224)).astype(np.float32)
    scores = rng.standard_normal((m_all, k_all)).astype(np.float32)
    scores[0, 0], scores[1, 1], scores[2, 2], scores[3, 0] = 0.0, -0.0, -0.37, 3.0e4
    assert np.signbit(scores[1, 1]) and (scores < 0).any() and (sal0 != 0).all()
    got = masks.saliency_sum_classes(sal0, scores, w)
    assert got.dtype == np.float32 and got.shape == sal0.shape
    for k in range(k_all):
        want = rise_ref.saliency_emulation(sal0[k], scores[:, k], w)
        assert (got[k].view(np.int32) == want.view(np.int32)).all(), k
    assert (sal0 != got).any()                      # the input is not accumulated in place


def test_saliency_sum_classes_refuses_mismatched_shapes():
    w = np.zeros((2, 224, 224), np.float32)
    with pytest.raises(ValueError):
        masks.saliency_sum_classes(np.zeros((3, 224, 224), np.float32), np.zeros((2, 4), np.float32), w)
    with pytest.raises(ValueError):
        masks.saliency_sum_classes(np.zeros((3, 224, 224), np.float32), np.zeros((3, 3), np.float32), w)


def _bare_engine():
    """An engine object with no device behind it: rise_saliency_classes checks its arguments before it touches one."""
    e = object.__new__(MaskedForwardEngine)
    e._h = None
    e.small = False
    return e


@pytest.mark.parametrize("kw", [
    dict(classes=[1, 2], top=3),            # both
    dict(top=0), dict(top=-2), dict(top=1001),
    dict(classes=[3, 1000]), dict(classes=[-1]),
    dict(classes=[]),
])
def test_rise_saliency_classes_argument_checks(kw):
    img = np.zeros((224, 224, 3), np.uint8)
    with pytest.raises(ValueError):
        _bare_engine().rise_saliency_classes(img, n_masks=4, **kw)
    with pytest.raises(ValueError):
        masks.class_selection(kw.get("classes"), kw.get("top"))


def test_class_selection_accepts():
    assert masks.class_selection(None, None) == (None, None)
    assert masks.class_selection(None, 1000) == (None, 1000)
    cls, top = masks.class_selection([7, 0, 999, 7], None)           # unsorted, a repeat: kept as given
    assert top is None and cls.dtype == np.int32 and cls.tolist() == [7, 0, 999, 7]


def test_top_ties_go_to_the_lower_index():
    logits = np.array([0.5, 2.0, -1.0, 2.0, 0.5, 2.0, 3.0], dtype=np.float32)
    assert masks.top_classes(logits, 1).tolist() == [6]
    assert masks.top_classes(logits, 3).tolist() == [6, 1, 3]
    assert masks.top_classes(logits, 5).tolist() == [6, 1, 3, 5, 0]
    got = masks.top_classes(logits, 7)
    assert got.dtype == np.int32 and got.tolist() == np.argsort(-logits, kind="stable").tolist()
    with pytest.raises(ValueError):
        masks.top_classes(logits, 8)


def test_new_entries_are_exported_and_bound(mpx_lib):
    for name in NEW_ENTRIES:
        assert name in _lib.SIGNATURES
        assert getattr(mpx_lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.SALIENCY_CLASS_TILE >= 2
    src = open(_lib.__file__.replace("_lib.py", "csrc/mpx_saliency_classes.h")).read()
    assert "constexpr int SC_KT = %d;" % _lib.SALIENCY_CLASS_TILE in src          # the one Python copy of the kernel's class tile
