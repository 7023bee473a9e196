"""Painted object comparisons on the GPU (csrc/paint.hip, ops.object_match / ops.label_paint, the device paths of paint.py and
evaluate.evaluate_flat) against the host functions.  Integer image processing, the float formulas the same host code fed the
same integers: every comparison is EXACT (array_equal, ==)."""
import logging
import os

import numpy as np
import pytest
import torch

from _paintcases import eval_case, paint_case, write_eval_dirs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'paint.npz'))


def _dev(a, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype).contiguous()


def _match_on_device(tables, nS_own, nG_own):
    from wesup_amd import ops
    out = ops.object_match(_dev(np.stack(tables)), _dev(nS_own), _dev(nG_own))
    assert out.dtype == torch.int32
    return out.cpu().numpy()


def _random_table(rs, nS, nG):
    """A table whose columns hold, planted among random counts: exact halves, halves plus one, and several candidates of one
    area for one row (ties) -- the decisions the rule turns on."""
    C = rs.randint(0, 4, (nS + 1, nG + 1)).astype(np.int64)
    for g in range(1, nG + 1):
        if nS == 0:
            break
        p = rs.randint(1, nS + 1)
        kind = rs.randint(4)
        rest = int(C[:, g].sum() - C[p, g])
        if kind == 0:
            C[p, g] = rest                                   # exactly half of the column
        elif kind == 1:
            C[p, g] = rest + 1                               # half plus one: a match
        elif kind == 2 and g > 1:                            # a tie: the column before once more (its area, its candidates)
            C[:, g] = C[:, g - 1]
    return C


def test_object_match_edges_by_hand():
    from wesup_amd.paint import match_objects_from_table
    C = np.array([[900, 0, 0, 50, 40, 9], [10, 100, 100, 0, 0, 0], [5, 0, 0, 50, 0, 0], [7, 0, 0, 0, 0, 0], [0, 0, 0, 0, 41, 10]])
    D = C.copy()
    D[4, 4], D[0, 4] = 40, 41
    got = _match_on_device([C, D], [4, 4], [5, 5])
    assert got.tolist() == [[0, 1, 7, 8, 4], [0, 1, 7, 8, 5]]
    assert got[0].tolist() == match_objects_from_table(C).tolist()


@pytest.mark.parametrize('cols', [1, 2, 63, 64, 65, 257, 1025])
def test_object_match_equals_the_host_rule_on_random_tables(cols):
    from wesup_amd import ops
    from wesup_amd.paint import match_objects_from_table
    rs = np.random.RandomState(cols)
    nG = cols - 1
    matched = 0
    for nS in (0, 1, 300):
        C = _random_table(rs, nS, nG)
        want = match_objects_from_table(C)
        got = ops.object_match(_dev(C), _dev([nS]), _dev([nG])).cpu().numpy()             # the unbatched form
        assert got.shape == (nS + 1,) and np.array_equal(got, want), (nS, nG)
        matched += int((want[1:] <= nG).sum())
    assert matched > 0 or nG == 0                                                         # the planted candidates are found


def test_object_match_batch_with_each_images_own_counts():
    """Tables of the batch maxima; what lies outside an image's own counts is not read (garbage there), the rows past its
    own count are 0 and its fresh ids start above ITS counts."""
    from wesup_amd.paint import match_objects_from_table
    rs = np.random.RandomState(5)
    own = [(300, 70), (7, 129), (0, 0)]
    nS, nG = 300, 129
    tables, want = [], []
    for s, g in own:
        T = rs.randint(1, 1000, (nS + 1, nG + 1)).astype(np.int64)
        C = _random_table(rs, s, g)
        T[:s + 1, :g + 1] = C
        tables.append(T)
        want.append(np.r_[match_objects_from_table(C), np.zeros(nS - s, np.int64)])
    got = _match_on_device(tables, [s for s, _ in own], [g for _, g in own])
    assert np.array_equal(got, np.stack(want))


def _numpy_paint(labels, lut):
    """lut (n, 3) uint8; labels outside the table black."""
    ok = (labels >= 0) & (labels < len(lut))
    out = np.zeros(labels.shape + (3,), np.uint8)
    out[ok] = lut[labels[ok]]
    return out


@pytest.mark.parametrize('shape', [(7, 9), (96, 120), (522, 775)])
@pytest.mark.parametrize('n_lut', [1, 105, 20000])
def test_label_paint_equals_a_numpy_gather(shape, n_lut):
    """A batch of three: with H * W odd the second image starts off a word, so the groups at both of its ends straddle."""
    from wesup_amd import ops
    from wesup_amd.paint import pack_colours
    rs = np.random.RandomState(n_lut + shape[0])
    labels = rs.randint(0, n_lut, (3,) + shape).astype(np.int32)
    luts = rs.randint(0, 256, (3, n_lut, 3)).astype(np.uint8)
    packed = np.stack([pack_colours(l) for l in luts]) | np.int32(0x55 << 24)                # the top byte is not a colour
    out, status = ops.label_paint(_dev(labels), _dev(packed))
    assert out.dtype == torch.uint8 and tuple(out.shape) == (3,) + shape + (3,) and status.cpu().tolist() == [0, 0, 0]
    got = out.cpu().numpy()
    for b in range(3):
        assert np.array_equal(got[b], _numpy_paint(labels[b], luts[b])), b
    one, status = ops.label_paint(_dev(labels[1]), _dev(packed[1]))                       # the unbatched form
    assert tuple(one.shape) == shape + (3,) and np.array_equal(one.cpu().numpy(), got[1]) and status.cpu().tolist() == [0]


def test_label_paint_from_an_unaligned_view():
    """Labels that do not start on 16 bytes take the byte-wise kernel: the same picture."""
    from wesup_amd import ops
    from wesup_amd.paint import pack_colours
    rs = np.random.RandomState(1)
    lut = rs.randint(0, 256, (40, 3)).astype(np.uint8)
    flat = rs.randint(0, 40, 1 + 33 * 21).astype(np.int32)
    view = _dev(flat)[1:].view(33, 21)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    out, status = ops.label_paint(view, _dev(pack_colours(lut)))
    assert np.array_equal(out.cpu().numpy(), _numpy_paint(flat[1:].reshape(33, 21), lut)) and status.cpu().tolist() == [0]


@pytest.mark.parametrize('n_lut', [105, 20000])
def test_label_paint_flags_a_label_outside_the_table(n_lut):
    from wesup_amd import ops
    from wesup_amd.paint import pack_colours
    rs = np.random.RandomState(2)
    labels = rs.randint(0, n_lut, (3, 95, 121)).astype(np.int32)       # H * W = 4 k + 3
    labels[0, 50, 60] = n_lut                              # one past the table, in a whole group
    labels[2, 94, 120] = -1                                # negative, the last pixel of the batch (the tail)
    labels[2, 0, 0] = 1 << 30                              # far outside, in the group that straddles images 1 and 2
    lut = rs.randint(1, 256, (n_lut, 3)).astype(np.uint8)  # no black in the table: a black pixel is a refused label
    out, status = ops.label_paint(_dev(labels), _dev(np.stack([pack_colours(lut)] * 3)))
    assert status.cpu().tolist() == [1, 0, 1]
    got = out.cpu().numpy()
    assert np.array_equal(got, np.stack([_numpy_paint(l, lut) for l in labels]))
    black = ~got.any(-1)
    assert black.sum() == 3 and black[0, 50, 60] and black[2, 94, 120] and black[2, 0, 0]


def test_paint_pred_and_gt_on_the_device_equals_the_host_on_every_case(gold):
    from wesup_amd import paint
    for name in (str(c) for c in gold['cases']):
        S, G = paint_case(gold, name)
        rs_h, rs_d = paint.reference_rng(), paint.reference_rng()
        want = paint.paint_pred_and_gt(S, G, rs_h)
        got = paint.paint_pred_and_gt(S, G, rs_d, device=DEV)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
        assert np.array_equal(got[0], gold[f'pred_{name}']) and np.array_equal(got[1], gold[f'gt_{name}']), name
        assert rs_h.randint(1 << 30) == rs_d.randint(1 << 30), name                        # and leaves the generator where the host does


def test_paint_pred_and_gt_on_the_device_at_glas_size():
    from wesup_amd import paint, synth
    S, G = synth.gland_pair(0)
    assert S.shape == (522, 775)
    want = paint.paint_pred_and_gt(S, G)
    got = paint.paint_pred_and_gt(S, G, device=DEV)
    assert got[0].dtype == np.uint8 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert len(np.unique(want[0].reshape(-1, 3), axis=0)) > 3


def test_paint_falls_back_to_the_host_for_an_oversize_table(gold, monkeypatch, caplog):
    from wesup_amd import ops, paint
    S, G = paint_case(gold, 'many')
    monkeypatch.setattr(ops, 'CONTINGENCY_MAX_CELLS', 1000)
    monkeypatch.setattr(paint, '_said', set())
    with caplog.at_level(logging.WARNING, logger='wesup_amd.paint'):
        got = paint.paint_pred_and_gt(S, G, device=DEV)
        paint.paint_pred_and_gt(S, G, device=DEV)
    assert np.array_equal(got[0], gold['pred_many']) and np.array_equal(got[1], gold['gt_many'])
    assert sum('painted on the host' in r.getMessage() for r in caplog.records) == 1       # said once


def test_evaluate_flat_on_the_device_equals_the_host(gold, tmp_path):
    from PIL import Image
    from wesup_amd.evaluate import evaluate_flat
    pred_root, gt_dir = write_eval_dirs(gold, tmp_path)
    rows_h, means_h, maps_h = evaluate_flat(pred_root, gt_dir, log=lambda s: None)
    saved_h = [np.asarray(Image.open(p)).copy() for p in sorted((tmp_path / 'results-new').glob('*.png'))]
    rows_d, means_d, maps_d = evaluate_flat(pred_root, gt_dir, log=lambda s: None, device=DEV)
    saved_d = [np.asarray(Image.open(p)) for p in sorted((tmp_path / 'results-new').glob('*.png'))]
    assert len(maps_d) == len(maps_h) == int(gold['eval_n'])
    for i in range(len(maps_h)):
        assert maps_d[i].dtype == np.float64 and np.array_equal(maps_d[i], maps_h[i]), i
        assert np.array_equal(maps_d[i], eval_case(gold, i)[2]) and np.array_equal(saved_d[i], saved_h[i]), i
    assert rows_d == rows_h and means_d == means_h
