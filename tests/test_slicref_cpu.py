"""tests/_slicref.py without a GPU: the fp64 reference of tests/test_slic_rounds_gpu.py against the float32 evaluation with
oracle/slic_oracle.py's arithmetic (where TAU comes from), against the oracle itself, and the facts about the cases that the
GPU tests rely on (which kernel and branch each one reaches)."""
import functools

import numpy as np
import pytest

import _slicref as sr
from oracle import slic_oracle as so

SINGLES = list(dict.fromkeys(list(sr.CASES) + [(k, H, W, n, m) for ks, H, W, n, m in sr.BATCHES for k in ks]))
# the cases of test_slic_gpu.test_slic_matches_restatement (synth_image(5), compactness 40)
RESTATEMENT = [(96, 128, 60), (120, 120, 72), (64, 200, 40)]


@functools.lru_cache(maxsize=None)
def _fp32_rounds(case):
    """Per round: compare() of the float32 evaluation with the fp64 reference forced onto its trajectory (tau = TAU)."""
    kind, H, W, n, m = case
    img = sr.image(kind, H, W)
    return [r for _, r, _, _ in sr.forced_rounds(img, n, m, sr.fp32_teacher(img, n, m), tau=sr.TAU)]


def test_tau_is_four_times_the_measured_fp32_excess():
    worst, where = 0.0, None
    for case in SINGLES:
        w = max(r['worst'] for r in _fp32_rounds(case))
        if w > worst:
            worst, where = w, sr.case_id(case)
    print(f'fp32 against fp64, one forced round at a time: largest excess {worst:.4e} at {where}; TAU = 4 x = {4 * worst:.4e}')
    assert worst == pytest.approx(sr.FP32_EXCESS, rel=1e-3), (worst, where)
    assert sr.TAU == 4 * sr.FP32_EXCESS > 0


@pytest.mark.parametrize('case', SINGLES, ids=sr.case_id)
def test_fp32_alone_stays_under_the_cap(case):
    _, H, W, _, _ = case
    for i, r in enumerate(_fp32_rounds(case), 1):
        assert len(r['bad']) == 0, (i, r)
        assert r['n_diff'] <= sr.CAP * H * W, (i, r['n_diff'], sr.CAP * H * W)


def test_cases_reach_the_branches_they_are_listed_for():
    steps = {(H, W, n): sr.Grid(H, W, n) for H, W, n, _, _ in sr._ROWS}
    tiled = lambda g: (15 // g.step + 2 + 6) ** 2 <= 176                 # wesup_slic's choice of the tile kernel
    assert [(g.step, g.start, tiled(g)) for g in steps.values()] == [                  # one entry per (H, W, n_segments)
        (14, 7, True), (3, 1, True), (2, 0, False), (2, 0, False), (1, 0, False), (1, 0, False),
        (6, 2, True), (3, 0, True), (3, 0, True), (6, 2, True)]
    g = steps[(5, 7, 1)]
    assert (g.gy, g.gx) == (1, 1)
    assert steps[(5, 7, 100)].K == 35 and steps[(33, 47, 1551)].K == 33 * 47          # every pixel a centre
    assert sr.Grid(1, 40, 4).start == 0 < int(np.floor(np.sqrt(40 / 4) / 2))            # start was clipped to H - 1
    assert 50 * 21 > 1024 > 33 * 21
    # step 3 is the smallest step of the tile kernel and the one where its LDS centre table is fullest.  16 consecutive pixels
    # touch at most 6 cells of 3 pixels, so a tile stages at most (6 + 2 * 3)^2 = 144 centres; the 13 x 13 = 169 of the host's
    # bound (15 / step + 2 + 6)^2 is never reached.  One more cell of radius (14 x 14 = 196) no longer fits the table of 176.
    g = steps[(96, 128, 1400)]
    assert g.tile_table_sizes(3).max() == 144
    assert max(sr.Grid(96, 128, n).tile_table_sizes(3).max() for n in (1400, 800, 500, 60)) == 144
    assert g.tile_table_sizes(4).max() == 196 > 176


@pytest.mark.parametrize('H,W', sorted({(H, W) for H, W, _, _, _ in sr._ROWS}))
def test_dark_image_covers_both_branches_of_the_lab_conversion(H, W):
    rgb, xyz = sr.lab_branches(sr.image('dark', H, W))
    assert (rgb > 0.04045).any() and (rgb <= 0.04045).any() and (rgb[rgb <= 0.04045] > 0).any()
    assert (xyz > 0.008856).any() and (xyz <= 0.008856).any()


def test_lab64_is_the_oracles_conversion_in_fp64():
    for kind in sr.IMAGES:
        img = sr.image(kind, 33, 47)
        a, b = sr.lab64(img), so.rgb2lab(img).astype(np.float64)
        assert np.abs(a - b).max() < 2e-4 * (1 + np.abs(a).max() / 100), kind       # float32 of values up to 100, through cbrt
    # textbook values: white, black, the red primary
    px = np.array([[1, 1, 1], [0, 0, 0], [1, 0, 0]], dtype=np.float32).T.reshape(3, 1, 3)
    np.testing.assert_allclose(sr.lab64(px)[0], [[100.0, 0.0, 0.0], [0.0, 0.0, 0.0], [53.24, 80.09, 67.20]], atol=0.02)


def test_pixel_inside_no_window_takes_its_home_cell_and_counts_in_its_sums():
    H = W = 24
    grid = sr.Grid(H, W, 36)
    assert (grid.step, grid.start, grid.gy, grid.gx) == (4, 2, 6, 6)
    rs = np.random.RandomState(0)
    lab = rs.rand(H, W, 3)
    cen = sr.init_centres(lab, grid)
    cen[:, 0:2] = rs.rand(36, 2) * 4.0                                   # every centre in the top-left corner: windows end at 12
    none = sr.in_no_window(cen, grid).reshape(H, W)
    assert none[13:, :].all() and none[:, 13:].all() and not none[:12, :12].any()
    labels = sr.assign(lab, cen, grid)
    home = grid.home()
    assert home.reshape(H, W)[20, 20] == 35 and home.reshape(H, W)[0, 0] == 0 and home.reshape(H, W)[23, 5] == 5 * 6 + 1
    assert np.array_equal(labels[none.ravel()], home[none.ravel()])
    # the exhaustive search over all centres agrees where a window holds the pixel
    y, x = np.divmod(np.arange(H * W), W)
    d = np.stack([sr.dist(lab, cen, grid, np.arange(H * W), np.full(H * W, k)) for k in range(36)])
    held = (np.abs(y[None] - cen[:, 0:1]) <= 8) & (np.abs(x[None] - cen[:, 1:2]) <= 8)
    brute = np.where(held, d, np.inf).argmin(axis=0)                      # argmin: the first, i.e. lowest, index among equals
    assert np.array_equal(labels[~none.ravel()], brute[~none.ravel()])
    # the 4 x 4 no-window pixels of the last home cell are members of centre 35 and move it
    new = sr.update(cen, labels, lab)
    mem = np.nonzero(labels == 35)[0]
    fallback = np.nonzero(none.ravel() & (home == 35))[0]
    assert len(fallback) == 16 and np.isin(fallback, mem).all() and not np.isin(mem, fallback).all()
    assert new[35, 0] == (mem // W).mean() and new[35, 1] == (mem % W).mean()
    np.testing.assert_allclose(new[35, 2:], lab.reshape(-1, 3)[mem].mean(axis=0), rtol=1e-14)


def test_strict_less_in_ascending_order_keeps_the_lower_index():
    grid = sr.Grid(8, 8, 4)                                               # step 4, centres at 2 and 6
    lab = np.zeros((8, 8, 3))
    cen = sr.init_centres(lab, grid)
    labels = sr.assign(lab, cen, grid).reshape(8, 8)
    assert labels[4, 4] == 0 and labels[4, 5] == 1 and labels[5, 4] == 2 and labels[0, 4] == 0     # row / column 4 is equidistant


@pytest.mark.parametrize('case', [('synth', 96, 128, 60, 40.0), ('noise', 33, 47, 388, 10.0), ('dark', 50, 21, 30, 20.0),
                                  ('region', 5, 7, 1, 40.0), ('noise', 1, 40, 4, 40.0)], ids=sr.case_id)
def test_reference_unforced_is_the_oracle(case):
    """Where float32 and fp64 agree in every forced round (no near tie), ten unforced rounds of the reference are the oracle's
    labels; in float32 the reference is the oracle to the bit, near ties or not."""
    kind, H, W, n, m = case
    img = sr.image(kind, H, W)
    assert all(r['n_diff'] == 0 for r in _fp32_rounds(case))
    want = so.kmeans_labels(img, n, m, 10)
    assert (want >= 0).all()
    assert np.array_equal(sr.unforced(img, n, m, 10), want)
    assert np.array_equal(sr.unforced(img, n, m, 10, np.float32), want)


def test_float32_reference_is_the_oracle_where_a_tie_is_near():
    img = sr.image('synth', 96, 128)
    assert max(r['n_diff'] for r in _fp32_rounds(('synth', 96, 128, 60, 1.0))) > 0
    assert np.array_equal(sr.unforced(img, 60, 1.0, 10, np.float32), so.kmeans_labels(img, 60, 1.0, 10))


@pytest.mark.parametrize('H,W,n', RESTATEMENT)
def test_restatement_cases_have_no_near_tie(H, W, n):
    """test_slic_gpu.test_slic_matches_restatement may compare ten unforced rounds exactly: float32 and fp64 agree everywhere."""
    from wesup_amd import synth
    img = synth.synth_image(5, H, W)
    rounds = [r for _, r, _, _ in sr.forced_rounds(img, n, 40.0, sr.fp32_teacher(img, n, 40.0), tau=sr.TAU)]
    assert all(r['n_diff'] == 0 for r in rounds)
    assert np.array_equal(sr.unforced(img, n, 40.0, 10), so.kmeans_labels(img, n, 40.0, 10))
