"""CPU-side checks of the real-valued mask convention (RISE, explicit weights): the four C-ABI entries exist and are bound, the public numpy
restatement of the kernel's weight formula (masks.rise_weights) sits within the bound derived from its operation count of torch's own
bilinear upsampling in fp64, the weights have the properties the device tests lean on, and the Python layer refuses what the device entries
leave to the caller.  No GPU anywhere in this file."""
import numpy as np
import pytest

from network_interpretation_imagenet_amd import _lib, masks
import rise_ref

ENTRIES = ("mpx_softmask_apply", "mpx_rise_apply", "mpx_softmask_saliency", "mpx_rise_saliency")


def test_entries_exported_and_bound(mpx_lib):
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and getattr(mpx_lib, name) is not None and name.encode() in blob, name
    # the apply entries take K0's arguments with the mask description swapped in; the RISE ones add (shift, s) to the explicit ones
    assert len(_lib.SIGNATURES["mpx_rise_apply"][1]) == len(_lib.SIGNATURES["mpx_softmask_apply"][1]) + 2
    assert len(_lib.SIGNATURES["mpx_rise_saliency"][1]) == len(_lib.SIGNATURES["mpx_softmask_saliency"][1]) + 2
    assert _lib.SOFTMASK_TILE == 32 and (masks.RISE_S_MIN, masks.RISE_S_MAX) == (2, 32)


@pytest.mark.parametrize("s", rise_ref.S_CASES)
def test_geometry(s):
    assert masks.rise_geometry(s) == rise_ref.GEOMETRY[s]


@pytest.mark.parametrize("s", rise_ref.S_CASES)
def test_emulation_within_derived_bound_of_fp64(s):
    """Corner shifts (0, 0), (cell-1, cell-1), (0, cell-1) and random ones; every element within rise_ref.W_BOUND = 9 * 2^-24 (+ 1e-12) of
    torch.nn.functional.interpolate in fp64.  The emulation sits at ~1.1e-7."""
    cells, shifts = rise_ref.draws(s, 12, seed=s)
    cell = rise_ref.GEOMETRY[s][0]
    assert (shifts[:3] == [[0, 0], [cell - 1, cell - 1], [0, cell - 1]]).all()
    w = masks.rise_weights(cells, shifts, s)
    assert w.dtype == np.float32 and w.shape == (12, 224, 224)
    err = np.abs(w.astype(np.float64) - rise_ref.ref_weights64(cells, shifts, s)).max()
    print("s=%d max |emulation - fp64| = %.3e (bound %.3e)" % (s, err, rise_ref.W_BOUND))
    assert err <= rise_ref.W_BOUND


@pytest.mark.parametrize("s", rise_ref.S_CASES)
def test_constant_grids_are_exact(s):
    shifts = np.concatenate([rise_ref.corner_shifts(s), masks.rise_shifts(5, s, rng=1)])
    m = len(shifts)
    ones = masks.rise_weights(np.ones((m, s, s), dtype=np.uint8), shifts, s)
    zeros = masks.rise_weights(np.zeros((m, s, s), dtype=np.uint8), shifts, s)
    assert (ones == np.float32(1.0)).all() and (zeros.view(np.int32) == 0).all()
    assert (masks.rise_weights(np.full((m, s, s), 255, dtype=np.uint8), shifts, s) == np.float32(1.0)).all()      # non-zero = keep


@pytest.mark.parametrize("s", (7, 13, 32))
def test_weights_are_really_real_valued(s):
    """On the seeded p1 = 0.5 draws at least half of the weights lie strictly inside (0, 1) and both exact ends occur: a test on such masks
    is not a test of binary masks in disguise."""
    rng = np.random.default_rng(0)
    cells, shifts = masks.rise_cells(16, s, 0.5, rng), masks.rise_shifts(16, s, rng)
    w = masks.rise_weights(cells, shifts, s)
    assert w.min() >= 0.0 and w.max() <= 1.0
    inside = float(((w > 0) & (w < 1)).mean())
    print("s=%d share strictly inside (0, 1): %.3f" % (s, inside))
    assert inside >= 0.5
    assert (w == 0).any() and (w == 1).any()


def test_generators_shapes_dtypes_and_seeds():
    for s in rise_ref.S_CASES:
        cell = rise_ref.GEOMETRY[s][0]
        cells, shifts = masks.rise_cells(9, s, 0.5, rng=5), masks.rise_shifts(9, s, rng=5)
        assert cells.dtype == np.uint8 and cells.shape == (9, s, s) and set(np.unique(cells)) <= {0, 1}
        assert shifts.dtype == np.int32 and shifts.shape == (9, 2) and shifts.min() >= 0 and shifts.max() < cell
        assert (cells == masks.rise_cells(9, s, 0.5, rng=5)).all() and (shifts == masks.rise_shifts(9, s, rng=5)).all()
        assert (cells != masks.rise_cells(9, s, 0.5, rng=6)).any()
    assert masks.rise_cells(2000, 7, 0.25, rng=0).mean() == pytest.approx(0.25, abs=0.01)
    assert masks.rise_cells(3, 7, 1.0, rng=0).all() and not masks.rise_cells(3, 7, 0.0, rng=0).any()
    assert masks.rise_cells(0, 7).shape == (0, 7, 7) and masks.rise_shifts(0, 7).shape == (0, 2)
    # one job's draws: the cells, then the shifts, from one generator
    cells, shifts = masks.rise_masks(6, 7, 0.5, seed=11)
    rng = np.random.default_rng(11)
    assert (cells == masks.rise_cells(6, 7, 0.5, rng)).all() and (shifts == masks.rise_shifts(6, 7, rng)).all()


def test_python_side_refusals():
    cells, shifts = rise_ref.draws(7, 4)
    for s in (1, 33, 0, -7):
        with pytest.raises(ValueError):
            masks.rise_geometry(s)
        with pytest.raises(ValueError):
            masks.rise_cells(4, s)
        with pytest.raises(ValueError):
            masks.rise_shifts(4, s)
    for bad in ([[0, 32]], [[32, 0]], [[-1, 0]], [[0, -1]]):          # cell = 32 at s = 7
        sh = shifts.copy()
        sh[2] = bad[0]
        with pytest.raises(ValueError):
            masks.check_rise(cells, sh, 7)
        with pytest.raises(ValueError):
            masks.rise_weights(cells, sh, 7)
    with pytest.raises(ValueError):
        masks.check_rise(cells, shifts, 13)                           # cells are 7 x 7
    with pytest.raises(ValueError):
        masks.check_rise(cells.astype(np.int32), shifts, 7)
    with pytest.raises(ValueError):
        masks.check_rise(cells, shifts.astype(np.int64), 7)
    with pytest.raises(ValueError):
        masks.check_rise(cells, shifts[:3], 7)
    with pytest.raises(ValueError):
        masks.check_rise(cells[:, :6], shifts, 7)
    with pytest.raises(ValueError):
        masks.rise_cells(4, 7, p1=1.5)
    c2, s2 = masks.check_rise(cells, shifts, 7)
    assert c2.flags.c_contiguous and s2.flags.c_contiguous and (c2 == cells).all() and (s2 == shifts).all()
