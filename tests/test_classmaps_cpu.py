"""Class maps for more than two classes without a GPU: the host functions that are the specification of the
device paths -- ``infer_tile.combine_patches_to_classes`` (soft and hard vote, first maximum) and ``slide.slide_class_scores`` --
the bindings of the five entries of csrc/classmap.hip, the pixel model of a three-class checkpoint and index PNGs."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ['wesup_window_merge_classes', 'wesup_planes_resize_acc', 'wesup_class_argmax_u8', 'wesup_patch_scatter_classes_u8',
           'wesup_label_confusion']


# ------------------------------------------------------------------------------------------ combine_patches_to_classes
def test_a_vote_tie_goes_to_the_lowest_class():
    from wesup_amd import infer_tile as T
    # 4 x 6 image, p = 4: two windows at columns 0 and 2, columns 2 and 3 are covered by both
    assert [l for _, l in T._get_top_left_coordinates(4, 6, 4)] == [0, 2]
    a, b = np.full((4, 4), 2.0), np.full((4, 4), 1.0)
    got = T.combine_patches_to_classes(np.stack([a, b]), 4, 6, 3, votes=True)
    assert got.dtype == np.uint8 and got.shape == (4, 6)
    assert got[0].tolist() == [2, 2, 1, 1, 1, 1]                       # one vote each for 2 and 1: the lower class
    got = T.combine_patches_to_classes(np.stack([b, a]), 4, 6, 3, votes=True)
    assert got[0].tolist() == [1, 1, 1, 1, 2, 2]                       # whichever window comes first
    # an index outside [0, C) or a NaN is a vote for no class: the other window decides, and alone it leaves class 0
    bad = a.copy()
    bad[0, 2], bad[0, 3], bad[0, 0] = 3.0, np.nan, -1.0
    got = T.combine_patches_to_classes(np.stack([bad, a]), 4, 6, 3, votes=True)
    assert got[0].tolist() == [0, 2, 2, 2, 2, 2]
    with pytest.raises(ValueError):
        T.combine_patches_to_classes(np.zeros((2, 4, 4, 3)), 4, 6, 3, votes=True)
    with pytest.raises(ValueError):
        T.combine_patches_to_classes(np.zeros((2, 4, 4)), 4, 6, 3)


def test_a_probability_tie_goes_to_the_first_maximum():
    from wesup_amd import infer_tile as T
    p = np.zeros((1, 2, 2, 3), dtype=np.float32)
    p[0, 0, 0] = [0.4, 0.4, 0.2]
    p[0, 0, 1] = [0.2, 0.4, 0.4]
    p[0, 1, 0] = [0.25, 0.25, 0.5]
    p[0, 1, 1] = [1 / 3, 1 / 3, 1 / 3]
    assert T.combine_patches_to_classes(p, 2, 2, 3).tolist() == [[0, 1], [2, 0]]
    # two windows whose means tie: (0.5 + 0.1) / 2 == (0.1 + 0.5) / 2 exactly
    q = np.zeros((2, 4, 4, 3), dtype=np.float32)
    q[0, ..., 1], q[0, ..., 2] = 0.5, 0.125
    q[1, ..., 1], q[1, ..., 2] = 0.125, 0.5
    got = T.combine_patches_to_classes(q, 4, 6, 3)
    assert got[0].tolist() == [1, 1, 1, 1, 2, 2]
    merged = T.combine_patches_to_image(q, 4, 6)
    assert np.array_equal(got, merged.argmax(axis=-1))


@pytest.mark.parametrize('H,W,p', [(64, 64, 64), (80, 112, 64), (150, 333, 64)])
def test_two_class_hard_vote_is_the_rounded_mean_of_the_rounded_maps(H, W, p):
    """round(mean(round(p))) of the two-class path, the half-to-even tie that goes to 0 included."""
    from wesup_amd import infer_tile as T
    N = len(T._get_top_left_coordinates(H, W, p))
    rs = np.random.RandomState(H + W)
    prob = rs.rand(N, p, p).astype(np.float32)
    want = np.round(T.combine_patches_to_image(np.round(prob), H, W))
    assert (T.combine_patches_to_image(np.round(prob), H, W) == 0.5).any() or N == 1      # split votes do occur
    got = T.combine_patches_to_classes(np.round(prob), H, W, 2, votes=True)
    assert np.array_equal(got, want.astype(np.uint8))


# --------------------------------------------------------------------------------------------------- slide_class_scores
def test_slide_class_scores_against_a_table_counted_by_hand():
    from wesup_amd import slide as S
    G = np.array([[0, 0, 1, 1], [1, 3, 3, 3]], dtype=np.uint8)          # class 2 is in neither map
    P = np.array([[0, 1, 1, 1], [0, 3, 3, 0]], dtype=np.uint8)
    # conf[g][p]: g0 -> p0, p1; g1 -> p1, p1, p0; g3 -> p3, p3, p0
    conf = np.array([[1, 1, 0, 0], [1, 2, 0, 0], [0, 0, 0, 0], [1, 0, 0, 2]])
    acc = 5 / 8
    dice = np.mean([2 * 1 / (2 + 3 + 1e-7), 2 * 2 / (3 + 3 + 1e-7), 2 * 2 / (3 + 2 + 1e-7)])       # classes 0, 1, 3
    from wesup_amd.utils import metrics as M
    assert M.confusion(P, G, 4).tolist() == conf.tolist()
    got = S.slide_class_scores(P, G, 4)
    assert isinstance(got[0], float) and isinstance(got[1], float)
    assert got[0] == acc and abs(got[1] - dice) < 1e-15
    assert S.slide_class_scores(torch.from_numpy(P), torch.from_numpy(G), 4) == got
    with pytest.raises(ValueError):
        S.slide_class_scores(P, G, 3)                                   # class 3 is outside [0, 3)


def test_score_directory_scores_class_maps_as_one_group(tmp_path):
    from PIL import Image
    from wesup_amd import slide as S
    rs = np.random.RandomState(2)
    (tmp_path / 'out').mkdir()
    (tmp_path / 'masks').mkdir()
    pairs = []
    for stem, shape in (('negative-b', (9, 21)), ('other', (8, 8)), ('positive-a', (13, 17))):     # (sorted: the order of the means)
        P, G = rs.randint(0, 3, shape).astype(np.uint8), rs.randint(0, 3, shape).astype(np.uint8)
        Image.fromarray(P).save(tmp_path / 'out' / f'{stem}.png')
        Image.fromarray(G).save(tmp_path / 'masks' / f'{stem}.png')
        pairs.append(S.slide_class_scores(P, G, 3))
    lines = []
    got = S.score_directory(tmp_path / 'out', tmp_path / 'masks', log=lambda *a: lines.append(' '.join(str(v) for v in a)), n_classes=3)
    assert got == {'all': (float(np.mean([s[0] for s in pairs])), float(np.mean([s[1] for s in pairs])))}
    assert lines[1:] == [f'Accuracy: {got["all"][0]}', f'Dice: {got["all"][1]}']
    # a palette mask is read by its indices, not by the luminance of its colours
    mask = np.asarray(Image.open(tmp_path / 'masks' / 'other.png'))
    pal = Image.fromarray(mask, mode='P')
    pal.putpalette([255, 0, 0, 0, 255, 0, 0, 0, 255] + [0] * (253 * 3))
    pal.save(tmp_path / 'masks' / 'other.png')
    assert Image.open(tmp_path / 'masks' / 'other.png').mode == 'P'
    assert S.score_directory(tmp_path / 'out', tmp_path / 'masks', log=lambda *a: None, n_classes=3) == got
    # a prediction is scored against the mask of its own stem: as many files under other names are an error, as is a missing one
    (tmp_path / 'masks' / 'other.png').rename(tmp_path / 'masks' / 'another.png')
    with pytest.raises(ValueError, match='another'):
        S.score_directory(tmp_path / 'out', tmp_path / 'masks', log=lambda *a: None, n_classes=3)
    (tmp_path / 'masks' / 'another.png').unlink()
    with pytest.raises(ValueError):
        S.score_directory(tmp_path / 'out', tmp_path / 'masks', log=lambda *a: None, n_classes=3)


# ------------------------------------------------------------------------------------------------------------- bindings
def test_the_five_entries_are_declared_and_bound():
    from wesup_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'wesup_hip.h')).read()
    for name in ENTRIES:
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), name
        assert name in _lib._SIGS, name
        assert hasattr(_lib.load(), name), name
    assert _lib.ABI_VERSION == 6 and _lib.load().wesup_abi_version() == 6
    assert 'classmap.hip' in open(os.path.join(ROOT, 'wesup_amd', 'csrc', 'Makefile')).read()


def test_entries_refuse_bad_arguments_on_the_host():
    from wesup_amd import _lib
    h = _lib.load()
    assert h.wesup_window_merge_classes(None, None, None, None, None, 8, 8, 3, 1, 1, 8, 0, None) == -1
    assert h.wesup_planes_resize_acc(None, None, 4, 4, 8, 8, 3, 1.0, 0, None) == -1
    assert h.wesup_class_argmax_u8(None, None, 8, 3, None) == -1
    assert h.wesup_patch_scatter_classes_u8(None, None, None, 8, 8, 4, 4, 4, 3, 0, 0, 1, None) == -1
    assert h.wesup_label_confusion(None, None, None, None, 8, 3, None) == -1


def test_ops_wrappers_have_no_cpu_fallback():
    from wesup_amd import _lib, ops
    with pytest.raises(_lib.WesupHipError):
        ops.class_argmax_u8(torch.zeros(4, 3))
    with pytest.raises(_lib.WesupHipError):
        ops.label_confusion(torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8), 3)
    with pytest.raises(_lib.WesupHipError):
        ops.planes_resize_acc(torch.zeros(2, 2, 3), torch.zeros(4, 4, 3))


def test_pixel_model_of_a_three_class_checkpoint(tmp_path):
    from wesup_amd import infer_tile
    from wesup_amd.models.wesup import WESUP
    ck3 = tmp_path / 'ck3.pth'
    torch.save({'model_state_dict': WESUP(n_classes=3).state_dict()}, ck3)
    model = infer_tile._load_pixel_model(str(ck3), 'cpu', multiclass=True)
    assert model.n_classes == 3 and model.classifier[0].weight.shape == (3, 32)
    with pytest.raises(ValueError, match='3-class'):
        infer_tile._load_pixel_model(str(ck3), 'cpu')                     # a class-1 reader still refuses it
    assert infer_tile._load_pixel_model(None, 'cpu', multiclass=True).n_classes == 2
    loaded = torch.load(ck3, map_location='cpu')                          # a checkpoint already read: not read again
    assert infer_tile._load_pixel_model(loaded, 'cpu', multiclass=True).classifier[0].weight.shape == (3, 32)
    with pytest.raises(ValueError, match='3-class'):
        infer_tile._load_pixel_model(loaded, 'cpu')


# ------------------------------------------------------------------------------------------------------------ index PNGs
def test_index_pngs_round_trip(tmp_path):
    from PIL import Image
    from wesup_amd import infer_tile as T
    rs = np.random.RandomState(0)
    maps = [rs.randint(0, 3, (11, 7)).astype(np.uint8), rs.randint(0, 3, (5, 9)).astype(np.uint8)]
    T.save_predictions(maps, ['x/a.jpg', 'x/b.png'], tmp_path / 'o3', n_classes=3)      # a JPEG input: still a PNG of indices
    assert sorted(q.name for q in (tmp_path / 'o3').iterdir()) == ['a.png', 'b.png']
    for m, name in zip(maps, ('a.png', 'b.png')):
        with Image.open(tmp_path / 'o3' / name) as im:
            assert im.format == 'PNG' and np.array_equal(np.asarray(im), m)
    T.save_predictions([np.array([[0., 1.], [1., 1.]])], ['a.png'], tmp_path / 'o2')          # two classes: x 255, as ever
    assert np.asarray(Image.open(tmp_path / 'o2' / 'a.png')).tolist() == [[0, 255], [255, 255]]
    T.save_predictions([np.zeros((8, 8))], ['c.jpg'], tmp_path / 'o2')                        # ... under the input's own name
    assert (tmp_path / 'o2' / 'c.jpg').exists()
