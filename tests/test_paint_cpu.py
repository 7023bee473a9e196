"""Painted object comparisons, mask visualisation and the CRAG / LUSC evaluation on the host (wesup_amd/paint.py,
evaluate.evaluate_flat) against outputs of the reference's own scripts (tests/golden/paint.npz, tools/make_paint_golden.py).

Integer image processing: every comparison is EXACT, except the five means against the values the reference printed, which are
held to the 1e-9 relative bar of tests/test_oracle_golden.py (reference-produced floats; the object metrics are restated around
one contingency table here, which reorders float sums)."""
import os

import numpy as np
import pytest

from _paintcases import eval_case, paint_case, write_eval_dirs

REL = 1e-9


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'paint.npz'))


def test_palette_is_the_references(gold):
    from wesup_amd import paint
    p = paint.palette()
    assert p.dtype == np.uint8 and p.shape == (104, 3) and np.array_equal(p, gold['palette'])
    assert tuple(p[0]) == (64, 255, 64) and tuple(p[-1]) == (255, 255, 128)


def test_reference_rng_continues_after_the_shuffle():
    from wesup_amd import paint
    rs = paint.reference_rng()
    assert rs.randint(0, 256, size=(3,), dtype='uint8').tolist() == [242, 85, 231]
    assert rs.randint(0, 256, size=(3,), dtype='uint8').tolist() == [80, 154, 244]
    assert paint.reference_rng().randint(0, 256, size=(3,), dtype='uint8').tolist() == [242, 85, 231]      # a fresh one per call


def test_match_rule_edges_by_hand():
    from wesup_amd.paint import match_objects_from_table
    #        bg  g1   g2   g3  g4  g5
    C = [[900, 0, 0, 50, 40, 9],
         [10, 100, 100, 0, 0, 0],       # p1 covers g1 and g2 (100 each) entirely: equal areas, the lower id
         [5, 0, 0, 50, 0, 0],           # p2 covers exactly half of g3 (100): no match -> max(4, 5) + 2
         [7, 0, 0, 0, 0, 0],            # p3 covers nothing -> 5 + 3
         [0, 0, 0, 0, 41, 10]]          # p4: 41 of 81 (g4) and 10 of 19 (g5) both match: the larger one
    assert match_objects_from_table(C).tolist() == [0, 1, 7, 8, 4]
    C[4][4], C[0][4] = 40, 41                                       # 40 of 81: only g5 is left
    assert match_objects_from_table(C).tolist() == [0, 1, 7, 8, 5]
    assert match_objects_from_table([[5]]).tolist() == [0]
    assert match_objects_from_table([[5], [3], [2]]).tolist() == [0, 3, 4]                 # no ground truth: nP + p
    assert match_objects_from_table([[5, 3, 2]]).tolist() == [0]


def test_match_reproduces_the_relabelled_maps_of_the_reference(gold):
    """The reference paints its relabelled prediction; inside the palette the colour of a pixel names its id, so on the cases
    with fewer than 104 ids the painted array determines the relabelled map."""
    from wesup_amd import paint
    from wesup_amd.utils import metrics as M
    pal = paint.palette()
    for name in ('ellipses', 'edges', 'no_gt', 'no_pred'):
        S, G = paint_case(gold, name)
        P, T = M.label(S), M.label(G)
        match = paint.match_objects_from_table(M._contingency(P, T)[0])
        assert match.max() < len(pal), name
        lut = np.zeros((len(pal), 3), np.uint8)
        lut[1:] = pal[1:]
        assert np.array_equal(lut[match[P]], gold[f'pred_{name}']), name
    S, G = paint_case(gold, 'edges')
    P, T = M.label(S), M.label(G)
    match = paint.match_objects_from_table(M._contingency(P, T)[0])
    assert match[P[5, 5]] == T[5, 5] and T[5, 5] < T[5, 20]                   # equal areas: the lower id
    assert match[P[5, 50]] == T[5, 62] and T[5, 62] > T[5, 50]                # the larger one, although later
    nP, nG = int(P.max()), int(T.max())
    assert match[P[40, 0]] == max(nP, nG) + P[40, 0]                          # exactly half: no match
    assert match[P[40, 26]] == T[40, 30]                                     # six tenths
    assert match[P[70, 60]] == max(nP, nG) + P[70, 60]                        # over nothing
    assert match[P[61, 6]] == T[60, 5]                                       # 9 of 16


def test_paint_pred_and_gt_equals_the_reference_on_every_case(gold):
    from wesup_amd import paint
    drew = 0
    for name in (str(c) for c in gold['cases']):
        S, G = paint_case(gold, name)
        pred, gt = paint.paint_pred_and_gt(S, G)
        assert pred.dtype == gt.dtype == np.uint8 and pred.shape == gt.shape == S.shape + (3,)
        assert np.array_equal(pred, gold[f'pred_{name}']), name
        assert np.array_equal(gt, gold[f'gt_{name}']), name
        rs = paint.reference_rng()
        paint.paint_pred_and_gt(S, G, rs)
        drew += rs.randint(1 << 30) != paint.reference_rng().randint(1 << 30)
    assert drew == 1                                       # 'many' alone goes beyond the palette: it did draw
    S, G = paint_case(gold, 'no_pred')
    assert not paint.paint_pred_and_gt(S, G)[0].any()      # an empty prediction is black


def test_paint_labels_beyond_the_palette_draw_in_ascending_order():
    from wesup_amd import paint
    m = np.array([[0, 300, 3], [104, 103, 300]])
    rs = paint.reference_rng()
    out = paint.paint(m, rs)
    pal = paint.palette()
    assert out[0, 0].tolist() == [0, 0, 0] and np.array_equal(out[0, 2], pal[3]) and np.array_equal(out[1, 1], pal[103])
    assert out[1, 0].tolist() == [242, 85, 231] and out[0, 1].tolist() == out[1, 2].tolist() == [80, 154, 244]


def _write_paint_dirs(gold, root):
    from PIL import Image
    os.makedirs(root / 'run' / 'pred')
    os.makedirs(root / 'run' / 'gt')
    for fname in (str(n) for n in gold['seq_inputs']):
        stem = fname.rsplit('.', 1)[0]
        S, G = paint_case(gold, 'many')[::-1] if stem == 'zz_many_swapped' else paint_case(gold, stem)
        Image.fromarray(S * np.uint8(255)).save(root / 'run' / 'pred' / fname)
        Image.fromarray(G).save(root / 'run' / 'gt' / fname)
    return root / 'run' / 'pred', root / 'run' / 'gt'


def test_cli_writes_the_files_of_one_run_of_the_reference(gold, tmp_path):
    """Names, default output directory and contents of a single-process run of the script over one directory: one generator in
    file order (the second case beyond the palette continues where the first stopped)."""
    from PIL import Image
    from wesup_amd import paint
    pred_dir, gt_dir = _write_paint_dirs(gold, tmp_path)
    paint.main([str(pred_dir), str(gt_dir), '-m', 'wesup'])
    out = tmp_path / 'run' / 'paintings'
    names = [str(n) for n in gold['seq_names']]
    assert sorted(os.listdir(out)) == names
    for n in names:
        assert np.array_equal(np.asarray(Image.open(out / n)), gold[f'seq_{n}']), n
    fresh = paint.paint_pred_and_gt(*paint_case(gold, 'many')[::-1])[0]
    assert not np.array_equal(gold['seq_zz_many_swapped.wesup.png'], fresh)                  # it is not a fresh generator's
    paint.main([str(pred_dir), str(gt_dir), '-o', str(tmp_path / 'elsewhere')])
    assert sorted(os.listdir(tmp_path / 'elsewhere')) == [n.replace('.wesup.', '.pred.') for n in names]


def test_masks_option_writes_every_mask_times_255(tmp_path):
    from PIL import Image
    from wesup_amd import paint
    rs = np.random.RandomState(0)
    os.makedirs(tmp_path / 'data' / 'masks')
    masks = {'a.png': (rs.rand(9, 7) < 0.5).astype(np.uint8), 'b.bmp': (rs.rand(5, 11) < 0.5).astype(np.uint8)}
    for name, m in masks.items():
        Image.fromarray(m).save(tmp_path / 'data' / 'masks' / name)
    paint.main(['--masks', str(tmp_path / 'data' / 'masks')])
    assert sorted(os.listdir(tmp_path / 'data' / 'viz')) == sorted(masks)
    for name, m in masks.items():
        assert np.array_equal(np.asarray(Image.open(tmp_path / 'data' / 'viz' / name)), m * 255), name
    paint.main(['--masks', str(tmp_path / 'data' / 'masks'), '-o', str(tmp_path / 'out')])
    assert sorted(os.listdir(tmp_path / 'out')) == sorted(masks)


def test_evaluate_flat_reproduces_the_reference(gold, tmp_path):
    from PIL import Image
    from wesup_amd.evaluate import evaluate_flat, remove_small_regions
    pred_root, gt_dir = write_eval_dirs(gold, tmp_path)
    lines = []
    rows, means, maps = evaluate_flat(pred_root, gt_dir, log=lines.append, csv_path=tmp_path / 'flat.csv')
    n = int(gold['eval_n'])
    assert len(rows) == len(maps) == n
    differs = 0
    for i in range(n):
        pred, _, post = eval_case(gold, i)
        assert maps[i].dtype == np.float64 and np.array_equal(maps[i], post), i
        assert np.array_equal(np.asarray(Image.open(tmp_path / 'results-new' / f'im{i}.png')), post * np.uint8(255)), i
        differs += not np.array_equal(remove_small_regions(pred / 255), post)
    assert differs == n                                    # the 2000-pixel rule of GlaS gives other maps on every pair
    keys = ('accuracy', 'dice', 'detection_f1', 'object_dice', 'object_hausdorff')
    for want in (gold['eval_means_crag'], gold['eval_means_lusc']):
        for k, w in zip(keys, want):
            assert abs(means[k] - w) <= REL * abs(w), (k, means[k], w)
    assert [l.split(':')[0] for l in lines] == [str(s) for s in gold['eval_names']]
    assert [float(l.split(': ')[1]) for l in lines] == [means[k] for k in keys]
    assert open(tmp_path / 'flat.csv').read().splitlines()[1].startswith('im0.png,')
    os.remove(gt_dir / 'im2.png')
    with pytest.raises(ValueError):
        evaluate_flat(pred_root, gt_dir, log=lambda s: None)


def test_dataset_option_routes_the_command_line(monkeypatch):
    from wesup_amd import evaluate
    calls = []
    monkeypatch.setattr(evaluate, 'evaluate_flat', lambda *a, **k: calls.append(('flat', a, k)))
    monkeypatch.setattr(evaluate, 'evaluate_glas', lambda *a, **k: calls.append(('glas', a, k)))
    evaluate.main(['P', '--dataset', 'crag'])
    evaluate.main(['P', '--dataset', 'lusc'])
    evaluate.main(['P', '--dataset', 'crag', '--gt-dir', 'D', '--gpu-scoring', '-d', 'cuda:1'])
    assert calls == [('flat', ('P', '~/data/CRAG/test/masks', 5000), {'device': None}),
                     ('flat', ('P', 'LUSC/test/masks', 5000), {'device': None}),
                     ('flat', ('P', 'D', 5000), {'device': 'cuda:1'})]
    del calls[:]
    evaluate.main(['P', '--dataset', 'glas'])
    evaluate.main(['P'])
    evaluate.main(['P', '--gt-root', 'R', '--min-size', '30', '--gpu-scoring'])
    assert calls == [('glas', ('P', '~/data/GLAS_all', 2000), {'device': None})] * 2 + \
                    [('glas', ('P', 'R', 30), {'device': 'cuda'})]
