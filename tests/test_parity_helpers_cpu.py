"""The yardsticks of tests/_parity.py bite: each is shown, on small random tensors, to catch what it exists to catch."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _parity          # noqa: E402
import _tol             # noqa: E402
from oracle import wesup_oracle as orc          # noqa: E402


@pytest.fixture(autouse=True)
def _keep_the_tolerance_record_clean():
    """The self-tests feed deliberately wrong values through _tol.within: none of them may land in tolerances.json."""
    n = len(_tol.RECORDS)
    yield
    del _tol.RECORDS[n:]


def test_windowed_fp64_conv_equals_the_full_conv_on_every_window():
    g = torch.Generator().manual_seed(0)
    for (ci, co, h, w) in [(3, 8, 37, 29), (16, 12, 9, 14), (8, 4, 5, 3), (4, 6, 50, 50)]:
        x = torch.randn(ci, h, w, generator=g)
        wt = torch.randn(co, ci, 3, 3, generator=g)
        bs = torch.randn(co, generator=g)
        full = F.conv2d(x[None].double(), wt.double(), bs.double(), padding=1)[0]
        wins = _parity.windows(h, w, 16) + [(0, h, 0, w), (1, h - 1, 2, w), (h - 1, h, w - 1, w)]
        for r0, r1, c0, c1 in wins:
            got = _parity.conv3x3_fp64(x, wt, bs, r0, r1, c0, c1)
            assert got.dtype == torch.float64 and got.shape == (co, r1 - r0, c1 - c0)
            assert float((got - full[:, r0:r1, c0:c1]).abs().max()) <= 1e-12 * float(full.abs().max()), (h, w, r0, r1, c0, c1)
    # the windows: four corners and the centre, clipped to the map; the bottom-right one ends at the ragged edge
    assert _parity.windows(50, 50) == [(0, 16, 0, 16), (0, 16, 34, 50), (34, 50, 0, 16), (34, 50, 34, 50), (17, 33, 17, 33)]
    assert _parity.windows(9, 14) == [(0, 9, 0, 14)]


def test_layer_input_applies_relu_and_the_pooling_of_the_layer_below():
    y = torch.randn(4, 7, 9)
    assert torch.equal(_parity.layer_input(1, None, y), torch.relu(y))                     # conv1_1 is not pooled
    assert torch.equal(_parity.layer_input(2, None, y), F.max_pool2d(torch.relu(y)[None], 2, 2)[0])   # conv1_2 is
    assert _parity.layer_input(2, None, y).shape == (4, 3, 4)
    img = torch.rand(3, 5, 5)
    assert _parity.layer_input(0, img, None) is img


def test_windowed_check_catches_a_wrong_output_in_a_ragged_corner():
    """check_conv_layers over a tiny 13-layer network: exact layers pass, one output off by 1e-4 of the layer's max in
    the bottom-right corner of a deep layer fails the 1e-5 bar."""
    g = torch.Generator().manual_seed(1)
    H, W = 70, 54
    weights = {}
    for idx, (ci, co) in zip(orc.CONV_IDX, orc.CONV_CH):
        ci, co = min(ci, 6), min(co, 6)
        weights[f'backbone.{idx}.weight'] = torch.randn(co, ci, 3, 3, generator=g) * 0.3
        weights[f'backbone.{idx}.bias'] = torch.randn(co, generator=g) * 0.05
    img = torch.rand(3, H, W, generator=g)
    ys, x = [], img
    for l, idx in enumerate(orc.CONV_IDX):
        y = F.conv2d(x[None].double(), weights[f'backbone.{idx}.weight'].double(), weights[f'backbone.{idx}.bias'].double(),
                     padding=1)[0].float()
        ys.append(y)
        if l < 12:
            x = _parity.layer_input(l + 1, None, y)
    assert max(_parity.check_conv_layers('cpu-helper', img, ys, weights, 1e-5)) <= 1e-6
    assert max(_parity.check_conv_layers('cpu-helper', img, ys, weights, 1e-5, full=True)) <= 1e-6
    bad = [y.clone() for y in ys]
    l = 10                                                                # conv5_1: 4 x 3 map (70 -> 35 -> 17 -> 8 -> 4)
    bad[l][2, -1, -1] += 1e-4 * float(bad[l].abs().max())
    try:
        _parity.check_conv_layers('cpu-helper', img, bad, weights, 1e-5)
    except AssertionError as e:
        assert e.args[0][1] == l
    else:
        raise AssertionError('a corner output off by 1e-4 of the layer max passed')


def test_per_slice_comparison_catches_what_the_global_max_misses():
    g = torch.Generator().manual_seed(2)
    ref = torch.randn(40, orc.FM_CHANNELS, generator=g)
    a, b = _parity.SLICES[5]
    assert (a, b) == (320, 448) and _parity.SLICES[-1] == (1856, 2112) and _parity.SLICES[0] == (0, 32)
    ref[:, a:b] *= 1e-3                                                   # a slice of small values
    got = ref.clone()
    got[7, a + 3] += 1e-3 * float(ref[:, a:b].abs().max())                # wrong by 1e-3 of its own scale
    glob = float((got - ref).abs().max() / ref.abs().max())
    assert glob < 1e-4                                                    # the global comparison passes it ...
    ok, errs = _parity.check_sp_slices('cpu-helper', 'per-slice helper self-test', got, ref, 1e-4)
    assert not ok and max(range(13), key=errs.__getitem__) == 5           # ... the per-slice one names the slice
    assert abs(errs[5] - 1e-3) < 1e-6 and max(errs[:5] + errs[6:]) == 0.0
    ok, _ = _parity.check_sp_slices('cpu-helper', 'per-slice helper self-test', ref.clone(), ref, 1e-4)
    assert ok


def _net(seed, H=12, W=10):
    """13 pre-activations of one image (C,h,w) at the real pooling pattern, and three fc outputs after their ReLU."""
    g = torch.Generator().manual_seed(seed)
    ys, h, w = [], H, W
    for l in range(13):
        ys.append(torch.randn(3, h, w, generator=g))
        if orc.POOL_AFTER[l]:
            h, w = max(h // 2, 1), max(w // 2, 1)
    fc = [torch.relu(torch.randn(9, 5, generator=g)) for _ in range(3)]
    return ys, fc


def test_decision_counter_finds_sign_flips_and_pooling_swaps():
    ys, fc = _net(3)
    n, bad = _parity.decision_diffs(ys, ys, fc, fc)
    assert n == 0 and bad == []
    # near-ties: a conv unit at +1e-7 of the layer max moved to -1e-7, an fc unit at +1e-7 zeroed by its ReLU
    ref = [y.clone() for y in ys]
    ref[4][1, 2, 1] = 1e-7 * float(ref[4].abs().max())
    run = [y.clone() for y in ref]
    run[4][1, 2, 1] = -run[4][1, 2, 1]
    fr = [h.clone() for h in fc]
    fr[1][3, 2] = 1e-7 * float(fr[1].abs().max())
    fh = [h.clone() for h in fr]
    fh[1][3, 2] = 0.0
    n, bad = _parity.decision_diffs(run, ref, fh, fr)
    assert n == 2 and bad == []
    # a sign flip that is not a near-tie is named
    run[0][0, 5, 5] = -run[0][0, 5, 5] if float(run[0][0, 5, 5]) != 0 else 1.0
    n, bad = _parity.decision_diffs(run, ref, fh, fr)
    assert n == 3 and bad == [('relu', 0, (0, 5, 5))]
    # pooling: a window whose two best candidates are swapped (conv1_2 is pooled); the gap is not a near-tie
    ref2 = [y.clone() for y in ys]
    win = ref2[1][0, 0:2, 0:2]
    win.copy_(torch.tensor([[0.2, 1.0], [0.3, 0.1]]))
    run2 = [y.clone() for y in ref2]
    run2[1][0, 0:2, 0:2] = torch.tensor([[1.0, 0.2], [0.3, 0.1]])        # arg-max 1 -> 0, both stay positive
    n, bad = _parity.decision_diffs(run2, ref2, fc, fc)
    assert n == 1 and bad == [('pool', 1, (0, 0, 0, 0, 0))]
    # ... and the same swap between two candidates within rounding of each other is a near-tie
    run2[1][0, 0:2, 0:2] = torch.tensor([[1.0, 1.0], [0.3, 0.1]])
    ref2[1][0, 0:2, 0:2] = torch.tensor([[1.0 - 1e-7, 1.0], [0.3, 0.1]])
    n, bad = _parity.decision_diffs(run2, ref2, fc, fc)
    assert n == 1 and bad == []
    # a swap inside a window that passes nothing (max <= 0) is no decision of consequence
    run3 = [y.clone() for y in ys]
    ref3 = [y.clone() for y in ys]
    ref3[3][1, 0:2, 2:4] = torch.tensor([[-0.5, -0.1], [-0.9, -0.7]])
    run3[3][1, 0:2, 2:4] = torch.tensor([[-0.05, -0.1], [-0.9, -0.7]])
    n, bad = _parity.decision_diffs(run3, ref3, fc, fc)
    assert n == 1 and bad == []


def test_near_tie_rows_follow_the_propagation_definition():
    """Row 0 sits on the threshold, row 1 has two equally close sources, row 2 is decided with room to spare."""
    lab = torch.tensor([[0.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 2.0, 0.0]])
    un = torch.tensor([[0.0, 0.0, 0.0, 0.5], [0.5, 0.3, 0.0, 0.0], [0.0, 0.0, 1.9, 0.1]])
    feats = torch.cat([lab, un])
    sp_labels = torch.eye(2)[[0, 1, 0]]
    thr = float(np.exp(np.float32(-0.25)))
    assert _parity.near_tie_rows(feats, sp_labels, threshold=thr).tolist() == [True, True, False]
    assert _parity.near_tie_rows(feats, sp_labels, threshold=0.5).tolist() == [False, True, False]
