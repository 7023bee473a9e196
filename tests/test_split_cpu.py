"""Splitting touching objects: the numpy definitions in wesup_amd/split.py against scipy and against the
properties they promise, the scoring of a merged pair before and after the split, the command lines, and the host-side argument
checks of the new C entries.  No GPU."""
import os

import numpy as np
import pytest
from scipy import ndimage

from wesup_amd import evaluate, split
from wesup_amd.utils import metrics as M

from _splitcases import (EDT_CASES, RADII, check_properties, disc_scene, random_mask, random_seeds, serpentine,
                         serpentine_ends, write_scene)


@pytest.mark.parametrize('h,w,dens', EDT_CASES)
def test_edt_sq_host_equals_scipy(h, w, dens):
    F = random_mask(h, w, dens, seed=h * 1000 + w)
    e = ndimage.distance_transform_edt(F)
    for r in RADII:
        cap = r * r
        got = split.edt_sq_host(F, cap)
        assert got.dtype == np.int32
        assert np.array_equal(got, np.minimum(np.rint(e ** 2), cap))


def test_edt_sq_host_edges():
    assert (split.edt_sq_host(np.ones((9, 13), np.uint8), 400) == 400).all()       # no background in reach: the cap
    assert (split.edt_sq_host(np.ones((9, 13), np.uint8), 65025) == 65025).all()
    assert (split.edt_sq_host(np.zeros((9, 13), np.uint8), 400) == 0).all()
    row = np.array([[1, 1, 0, 1, 1, 1, 1]], np.uint8)
    assert split.edt_sq_host(row, 9).tolist() == [[4, 1, 0, 1, 4, 9, 9]]           # H = 1
    assert split.edt_sq_host(row.T, 9).tolist() == [[4], [1], [0], [1], [4], [9], [9]]   # W = 1
    assert split.edt_sq_host(np.ones((1, 1), np.uint8), 1).tolist() == [[1]]
    both = split.edt_sq_host(np.stack([row, 1 - row]), 9)                          # images of a batch do not see each other
    assert both.tolist() == [[[4, 1, 0, 1, 4, 9, 9]], [[0, 0, 1, 0, 0, 0, 0]]]
    for cap in (0, 65026):
        with pytest.raises(ValueError):
            split.edt_sq_host(row, cap)


def test_label_grow_host_serpentine_one_seed():
    F = serpentine()
    assert F.shape == (41, 67) and M.label(F).max() == 1
    (y0, x0), _ = serpentine_ends(F)
    S = np.zeros(F.shape, np.int32)
    S[y0, x0] = 1
    L, rounds = split.label_grow_host(F, S, return_rounds=True)
    assert L.dtype == np.int32 and np.array_equal(L, F.astype(np.int32))
    assert rounds > 1000                                                           # the front walks the whole corridor


def test_label_grow_host_serpentine_two_seeds():
    F = serpentine()
    a, b = serpentine_ends(F)
    assert F[a] and F[b]
    S = np.zeros(F.shape, np.int32)
    S[a], S[b] = 1, 2
    L = split.label_grow_host(F, S)
    assert set(np.unique(L[F != 0])) == {1, 2} and (L[F == 0] == 0).all()
    pairs = 0                                                                      # unordered 8-adjacent pairs of different labels
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
        n = split._shifted(L, dy, dx)
        pairs += int(((L > 0) & (n > 0) & (L != n)).sum())
    assert pairs == 1
    out = split.label_cut_host(F, L)
    cleared = (F != 0) & (out == 0)
    assert cleared.sum() >= 1 and (L[cleared] == 2).all()
    assert M.label(out).max() == 2


@pytest.mark.parametrize('density', (0.55, 0.6))
def test_cut_properties_on_random_masks(density):
    rng = np.random.default_rng(int(density * 100))
    for trial in range(3):
        F = (rng.random((97, 131)) < density).astype(np.uint8)
        S = random_seeds(F, 40, seed=trial + 7)
        L = split.label_grow_host(F, S)
        out = split.label_cut_host(F, L)
        check_properties(F, S, L, out)


def test_close_seeds_cut_the_larger_one():
    """Two seeds are never 8-adjacent, but that alone does not protect a seed pixel: with one free pixel between two seeds the
    pixel takes the smaller label in round 1 and the larger seed, now next to it, is cut."""
    F = np.ones((1, 5), np.uint8)
    S = np.array([[0, 5, 0, 9, 0]], np.int32)
    L = split.label_grow_host(F, S)
    assert L.tolist() == [[5, 5, 5, 9, 9]]
    assert split.label_cut_host(F, L).tolist() == [[1, 1, 1, 0, 1]]


def test_largest_label_spreads():
    """Seed labels may be any positive int32: 2^31 - 1 grows like every other label and loses against every other label."""
    top = 2 ** 31 - 1
    F = np.ones((3, 9), np.uint8)
    F[1, 4] = 0
    S = np.zeros((3, 9), np.int32)
    S[1, 0] = top
    L = split.label_grow_host(F, S)
    assert L.dtype == np.int32 and (L[F != 0] == top).all() and L[1, 4] == 0
    S[1, 8] = top - 1
    L = split.label_grow_host(F, S)
    assert set(np.unique(L[F != 0])) == {top - 1, top}
    out = split.label_cut_host(F, L)
    assert (L[(F != 0) & (out == 0)] == top).all() and M.label(out).max() == 2


def test_split_properties_with_distance_seeds():
    pred, _ = disc_scene()
    out, L = split.split_objects(pred, 16, return_labels=True)
    r2 = 16 * 16
    seeds = M.label(split.edt_sq_host(pred, r2) >= r2)
    assert seeds.max() == 2
    check_properties(pred, seeds, L, out)


def test_radius_one_is_the_identity():
    F = random_mask(37, 53, 0.4, seed=3)
    assert np.array_equal(split.split_objects(F, 1), F)
    B = np.stack([F, 1 - F])
    assert np.array_equal(split.split_objects(B, 1), B)
    for r in (0, 256):
        with pytest.raises(ValueError):
            split.split_objects(F, r)


def test_disc_scene_scores():
    pred, gt = disc_scene()
    assert M.label(pred).max() == 1
    f1_before, hd_before = M.detection_f1(pred, gt), M.object_hausdorff(pred, gt)
    assert f1_before < 0.67 and hd_before == 59.0
    for r in (12, 16, 20):
        out = split.split_objects(pred, r)
        assert M.label(out).max() == 2
        assert M.detection_f1(out, gt) > 0.9999
        assert M.object_hausdorff(out, gt) == 4.0
        assert M.object_dice(out, gt) > 0.86 > 0.56 > M.object_dice(pred, gt)
    assert np.array_equal(split.split_objects(pred, 31), pred)                     # no seed: the mask comes back unchanged


def test_evaluate_split_with_split_radius(tmp_path):
    pred_dir, gt_dir = write_scene(tmp_path)
    quiet = lambda *a: None
    rows0, means0 = evaluate.evaluate_split(pred_dir, gt_dir, None, None, 100, quiet)
    pred, gt = disc_scene()
    assert rows0[0]['detection_f1'] == float(M.detection_f1(pred.astype(np.float64), gt))       # today's numbers
    assert rows0[0]['object_dice'] == float(M.object_dice(pred.astype(np.float64), gt))
    assert rows0[0]['object_hausdorff'] == 59.0
    rows_none, _ = evaluate.evaluate_split(pred_dir, gt_dir, None, None, 100, quiet, None, split_radius=None)
    assert rows_none == rows0
    rows1, means1 = evaluate.evaluate_split(pred_dir, gt_dir, tmp_path / 'new', tmp_path / 'scene.csv', 100, quiet,
                                            split_radius=16)
    assert means0['detection_f1'] < 0.67 and means1['detection_f1'] > 0.9999
    assert rows1[0]['object_hausdorff'] == 4.0
    from PIL import Image
    saved = np.asarray(Image.open(tmp_path / 'new' / 'scene.png'))
    assert np.array_equal(saved, split.split_objects(pred, 16) * 255)              # the saved map is the split map
    assert str(rows1[0]['detection_f1']) in open(tmp_path / 'scene.csv').read()
    # the flat driver takes the same keyword
    _, means2, maps = evaluate.evaluate_flat(pred_dir, gt_dir, 100, quiet, split_radius=16)
    assert means2 == means1 and M.label(maps[0]).max() == 2


def test_command_lines_parse(tmp_path):
    a = split.build_parser().parse_args(['preds', 'out', '--radius', '16', '--gpu', '--labels'])
    assert (a.pred_dir, a.out_dir, a.radius, a.gpu, a.labels) == ('preds', 'out', 16, True, True)
    a = split.build_parser().parse_args(['preds', 'out', '--radius', '20'])
    assert not a.gpu and not a.labels
    with pytest.raises(SystemExit):
        split.build_parser().parse_args(['preds', 'out'])                          # --radius is required
    e = evaluate.build_parser().parse_args(['preds', '--dataset', 'crag', '--split-objects', '16'])
    assert e.split_objects == 16 and e.dataset == 'crag'
    assert evaluate.build_parser().parse_args(['preds']).split_objects is None
    # the tool end to end on the host
    pred_dir, _ = write_scene(tmp_path)
    split.main([str(pred_dir), str(tmp_path / 'out'), '--radius', '16', '--labels'])
    from PIL import Image
    pred, _ = disc_scene()
    out = np.asarray(Image.open(tmp_path / 'out' / 'scene.png'))
    inst = np.asarray(Image.open(tmp_path / 'out' / 'scene_labels.png'))
    assert np.array_equal(out, split.split_objects(pred, 16) * 255)
    assert inst.dtype == np.uint16 and inst.max() == 2 and np.array_equal(inst, M.label(out))


@pytest.fixture(scope='module')
def lib():
    from wesup_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_entries_refuse_bad_arguments_on_the_host(lib):
    """Every refusal differs from a valid call in one argument: the maps are five separate stretches of one buffer."""
    import ctypes
    h = lib.load()
    buf = ctypes.create_string_buffer(8192)          # non-null addresses; no entry gets as far as using them
    base = ctypes.cast(buf, ctypes.c_void_p).value
    m, s, l, c, w = (base + 1024 * k for k in range(5))          # mask, seeds / d2, labels / out, changed, workspace
    big = 1 << 20

    def grow(mask=m, seeds=s, labels=l, changed=c, shape=(1, 5, 7), first=1, launches=2, rounds=8, ws=w, nb=big):
        return h.wesup_label_grow(mask, seeds, labels, changed, *shape, first, launches, rounds, ws, nb, None)

    assert h.wesup_edt_sq_workspace_bytes(2, 5, 7) >= 2 * 5 * 7
    assert h.wesup_label_grow_workspace_bytes(2, 5, 7) >= 2 * 5 * 7 * 4
    for B, H, W in ((0, 5, 7), (1, 0, 7), (1, 5, -1), (65536, 5, 7), (1, 65536, 7), (1, 5, 65536), (1, 40000, 40000)):
        assert h.wesup_edt_sq_workspace_bytes(B, H, W) == 0 and h.wesup_label_grow_workspace_bytes(B, H, W) == 0
        assert h.wesup_edt_sq(m, s, B, H, W, 400, w, big, None) == -1
        assert grow(shape=(B, H, W)) == -1
        assert h.wesup_label_cut(m, s, l, B, H, W, None) == -1
    # null pointers
    assert h.wesup_edt_sq(None, s, 1, 5, 7, 400, w, big, None) == -1
    assert h.wesup_edt_sq(m, None, 1, 5, 7, 400, w, big, None) == -1
    assert h.wesup_edt_sq(m, s, 1, 5, 7, 400, None, big, None) == -1
    for name in ('mask', 'seeds', 'labels', 'changed', 'ws'):
        assert grow(**{name: None}) == -1
    assert h.wesup_label_cut(None, s, l, 1, 5, 7, None) == -1
    assert h.wesup_label_cut(m, None, l, 1, 5, 7, None) == -1
    assert h.wesup_label_cut(m, s, None, 1, 5, 7, None) == -1
    # cap outside 1 .. 65025
    for cap in (0, -1, 65026):
        assert h.wesup_edt_sq(m, s, 1, 5, 7, cap, w, big, None) == -1
    # rounds per launch: even, 2 .. the halo; at least one launch; rounds count from 1
    for rounds in (1, 3, 7, 0, -2, lib.SPLIT_HALO + 2):
        assert grow(rounds=rounds) == -1
    assert grow(launches=0) == -1 and grow(first=0) == -1
    # a launch reads one map and writes another: seeds, labels and the workspace share no byte with each other, the mask or the word
    assert grow(seeds=l) == -1 and grow(seeds=w) == -1 and grow(labels=w) == -1 and grow(labels=m) == -1 and grow(ws=m) == -1
    assert grow(seeds=l + 4 * 34) == -1 and grow(ws=l - 4 * 34) == -1          # the last pixel of one map on the first of another
    assert grow(changed=l + 8) == -1 and grow(changed=w) == -1
    assert h.wesup_label_cut(m, s, m, 1, 5, 7, None) == -1 and h.wesup_label_cut(m, s, s + 100, 1, 5, 7, None) == -1
    assert h.wesup_label_cut(m, s, m + 34, 1, 5, 7, None) == -1 and h.wesup_label_cut(m, s, s - 34, 1, 5, 7, None) == -1
    # a short workspace
    assert h.wesup_edt_sq(m, s, 1, 5, 7, 400, w, 16, None) == -1
    assert grow(nb=16) == -1
    assert (lib.SPLIT_SEG, lib.SPLIT_ROWS, lib.SPLIT_TILE, lib.SPLIT_HALO) == (64, 4, 32, 8)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'wesup_hip.h')).read()
    for name, v in (('SEG', 64), ('ROWS', 4), ('TILE', 32), ('HALO', 8)):
        assert f'#define WESUP_SPLIT_{name} {v}' in hdr
