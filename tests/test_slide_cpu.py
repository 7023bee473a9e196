"""Host side of whole-slide evaluation (wesup_amd/slide.py, the mirror of the reference's test_dp2019_pipeline.py): the patch
lattice, the zero-padded cut and the stitch, accuracy / Dice and the region post-processing against the reference's own outputs
(tests/golden/dp2019.npz, written by tools/make_slide_golden.py), the command line, the scoring of PNGs on disk, and the argument
checks of the three library entries of csrc/slide.hip, which answer on the host before any launch.  No GPU here."""
import ctypes
import os
from pathlib import Path

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dp2019.npz')


@pytest.fixture(scope='module')
def lib():
    from wesup_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLDEN)


# ------------------------------------------------------------------------------------------ host functions vs the reference
def test_patches_and_corners_equal_the_reference(gold):
    from wesup_amd import slide as S
    p = int(gold['patch_size'])
    H, W = gold['slide'].shape[:2]
    n_h, n_w = S.patch_grid(H, W, p)
    assert (n_h, n_w) == (3, 3)
    patches = S.split_patches_array(gold['slide'], p)
    mask_patches = S.split_patches_array(gold['mask'], p)
    assert patches.shape == (9, p, p, 3) and patches.dtype == np.uint8 and mask_patches.shape == (9, p, p)
    # the reference walks x in its outer loop; here the lattice is row-major: matched by corner, every corner met once
    corners = [tuple(int(v) for v in c) for c in gold['corners_xy']]
    assert sorted(corners) == sorted((k % n_w * p, k // n_w * p) for k in range(n_h * n_w))
    for i, (x, y) in enumerate(corners):
        k = y // p * n_w + x // p
        assert np.array_equal(patches[k], gold['patches'][i]), (x, y)
        assert np.array_equal(mask_patches[k], gold['mask_patches'][i]), (x, y)
    # padding is zero, content is the slide's
    assert not patches[8][22:].any() and not patches[8][:, 3:].any()
    assert np.array_equal(patches[8][:22, :3], gold['slide'][128:, 128:])


def test_stitch_equals_the_reference(gold):
    from wesup_amd import slide as S
    p = int(gold['patch_size'])
    H, W = gold['slide'].shape[:2]
    n_w = S.patch_grid(H, W, p)[1]
    ordered = np.zeros_like(gold['pred_patches'])
    for i, (x, y) in enumerate(gold['corners_xy']):
        ordered[int(y) // p * n_w + int(x) // p] = gold['pred_patches'][i]
    got = S.combine_single_array(ordered, (H, W))
    assert got.dtype == gold['combined'].dtype == np.float64 and got.shape == (H, W)
    assert np.array_equal(got, gold['combined'])
    # cut and stitch are inverse to each other on the slide's own area
    assert np.array_equal(S.combine_single_array(S.split_patches_array(gold['mask'], p), (H, W)), gold['mask'])
    with pytest.raises(ValueError):
        S.combine_single_array(ordered[:8], (H, W))


def test_accuracy_and_dice_equal_the_reference(gold):
    from wesup_amd import slide as S
    for i in range(3):
        pred, gt = gold[f'pair{i}_pred'], gold[f'pair{i}_gt']
        for neg in (0, 1):
            P, G = (255 - pred, 255 - gt) if neg else (pred, gt)
            acc, dsc = S.accuracy(P, G), S.dice(P, G)
            assert isinstance(acc, np.float64) and isinstance(dsc, np.float64)
            assert acc == gold['scores'][i, neg, 0] and dsc == gold['scores'][i, neg, 1], (i, neg)
            assert S.slide_scores(pred, gt, negative=bool(neg)) == (float(acc), float(dsc))
    # the all-background pair: Dice 0 / (0 + 1e-7), and with both maps inverted 2n / (2n + 1e-7), just below 1
    assert gold['scores'][2, 0, 1] == 0.0 and 1.0 - 1e-9 < gold['scores'][2, 1, 1] < 1.0
    lines = []
    acc, dsc = S.compute_metrics([gold['pair0_pred'], gold['pair1_pred']], [gold['pair0_gt'], gold['pair1_gt']], negative=True,
                                 log=lambda *a: lines.append(' '.join(str(v) for v in a)))
    assert acc == float(np.mean(gold['scores'][:2, 1, 0])) and dsc == float(np.mean(gold['scores'][:2, 1, 1]))
    assert lines == [f'Accuracy: {np.mean(gold["scores"][:2, 1, 0])}', f'Dice: {np.mean(gold["scores"][:2, 1, 1])}']


def test_postprocess_equals_the_reference(gold):
    from wesup_amd import slide as S
    blob = gold['blob'].copy()
    got = S.postprocess(blob, threshold=30)
    assert got.dtype == np.uint8 and np.array_equal(got, gold['blob_post30'])
    assert np.array_equal(blob, gold['blob'])                                          # the argument is left alone
    assert (got != blob).any() and set(np.unique(got)) == {0, 255}


def test_patch_grid_at_exact_multiples():
    from wesup_amd import slide as S
    assert S.patch_grid(128, 64, 64) == (2, 1)             # not the reference's 3 x 2 of range(0, size + 1, patch)
    assert S.patch_grid(129, 65, 64) == (3, 2)
    assert S.patch_grid(50, 70, 64) == (1, 2)
    assert S.patch_grid(50, 60, 64) == (1, 1)              # p > H and p > W: one padded patch
    assert S.patch_grid(3000, 2600, 1000) == (3, 3)
    img = np.arange(128 * 64, dtype=np.uint8).reshape(128, 64)
    patches = S.split_patches_array(img, 64)
    assert patches.shape == (2, 64, 64) and np.array_equal(patches[1], img[64:])
    one = S.split_patches_array(img[:50, :60], 64)
    assert one.shape == (1, 64, 64) and np.array_equal(one[0, :50, :60], img[:50, :60]) and not one[0, 50:].any()
    for bad in ((0, 5, 4), (5, 0, 4), (5, 5, 0)):
        with pytest.raises(ValueError):
            S.patch_grid(*bad)


# ------------------------------------------------------------------------------------------------- the library entries
def test_new_entries_reject_bad_arguments_on_the_host(lib):
    """Null pointers, non-positive sizes, count < 1, first < 0, a mode / align_corners outside {0, 1}, stride < 1:
    WESUP_ERR_INVALID without a launch.  The pointers are 16-byte aligned host addresses that are never dereferenced: every
    call below fails its check first."""
    h = lib.load()
    buf = ctypes.create_string_buffer(256)
    ok = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    INVALID = -1
    # (a) wesup_patch_gather_resize(img, out, H, W, p, h, w, align_corners, first, count, stream)
    assert h.wesup_patch_gather_resize(None, ok, 8, 8, 4, 2, 2, 0, 0, 1, None) == INVALID
    assert h.wesup_patch_gather_resize(ok, None, 8, 8, 4, 2, 2, 0, 0, 1, None) == INVALID
    for sizes in ((0, 8, 4, 2, 2), (8, 0, 4, 2, 2), (8, 8, 0, 2, 2), (8, 8, 4, 0, 2), (8, 8, 4, 2, 0), (-1, 8, 4, 2, 2)):
        assert h.wesup_patch_gather_resize(ok, ok, *sizes, 0, 0, 1, None) == INVALID
    for ac in (-1, 2):
        assert h.wesup_patch_gather_resize(ok, ok, 8, 8, 4, 2, 2, ac, 0, 1, None) == INVALID
    assert h.wesup_patch_gather_resize(ok, ok, 8, 8, 4, 2, 2, 0, -1, 1, None) == INVALID
    assert h.wesup_patch_gather_resize(ok, ok, 8, 8, 4, 2, 2, 0, 0, 0, None) == INVALID
    # (b) wesup_patch_scatter_u8(pred, out, H, W, p, h, w, stride, mode, first, count, stream)
    assert h.wesup_patch_scatter_u8(None, ok, 8, 8, 4, 2, 2, 1, 0, 0, 1, None) == INVALID
    assert h.wesup_patch_scatter_u8(ok, None, 8, 8, 4, 2, 2, 1, 0, 0, 1, None) == INVALID
    for sizes in ((0, 8, 4, 2, 2), (8, 0, 4, 2, 2), (8, 8, 0, 2, 2), (8, 8, 4, 0, 2), (8, 8, 4, 2, 0), (8, 8, -4, 2, 2)):
        assert h.wesup_patch_scatter_u8(ok, ok, *sizes, 1, 0, 0, 1, None) == INVALID
    for stride in (0, -2):
        assert h.wesup_patch_scatter_u8(ok, ok, 8, 8, 4, 2, 2, stride, 0, 0, 1, None) == INVALID
    for mode in (-1, 2):
        assert h.wesup_patch_scatter_u8(ok, ok, 8, 8, 4, 2, 2, 1, mode, 0, 1, None) == INVALID
    assert h.wesup_patch_scatter_u8(ok, ok, 8, 8, 4, 2, 2, 1, 0, -1, 1, None) == INVALID
    assert h.wesup_patch_scatter_u8(ok, ok, 8, 8, 4, 2, 2, 1, 0, 0, 0, None) == INVALID
    # (c) wesup_mask_scores(S, G, out4, n, negative, stream)
    assert h.wesup_mask_scores(None, ok, ok, 16, 0, None) == INVALID
    assert h.wesup_mask_scores(ok, None, ok, 16, 0, None) == INVALID
    assert h.wesup_mask_scores(ok, ok, None, 16, 0, None) == INVALID
    assert h.wesup_mask_scores(ok, ok, ok, 0, 0, None) == INVALID
    assert h.wesup_mask_scores(ok, ok, ok, -5, 1, None) == INVALID
    assert h.wesup_abi_version() == 6                                                  # additions only


def test_wrappers_fail_loudly_without_gpu_tensors(lib):
    import torch
    from wesup_amd import ops
    with pytest.raises(lib.WesupHipError):
        ops.patch_gather_resize(torch.zeros(8, 8, 3, dtype=torch.uint8), 4, 2, 2, 0, 1)
    with pytest.raises(lib.WesupHipError):
        ops.patch_scatter_u8(torch.zeros(1, 2, 2), torch.zeros(8, 8, dtype=torch.uint8), 4, 0)
    with pytest.raises(lib.WesupHipError):
        ops.mask_scores(torch.zeros(8, 8, dtype=torch.uint8), torch.zeros(8, 8, dtype=torch.uint8))
    with pytest.raises(lib.WesupHipError):
        ops.patch_gather_resize(np.zeros((8, 8, 3), dtype=np.uint8), 4, 2, 2, 0, 1)      # not a tensor at all


# ------------------------------------------------------------------------------------------------------- command line
def test_command_line():
    from wesup_amd import slide as S
    a = S.parse_args(['~/data/dp2019/val', '-c', 'records/20190701/checkpoints/ckpt.0100.pth'])
    assert a.data_root == '~/data/dp2019/val' and a.patch_size == 1000 and not a.pixel and not a.skip_infer
    assert a.model == 'wesup' and a.device is None and a.batch is None and a.post_threshold is None
    a = S.parse_args(['d', '-c', 'c.pth', '--pixel', '-p', '500', '--skip-infer', '--batch', '3', '--post-threshold', '1000',
                      '--device', 'cuda:1'])
    assert (a.pixel, a.patch_size, a.skip_infer, a.batch, a.post_threshold, a.device) == (True, 500, True, 3, 1000, 'cuda:1')
    assert S.parse_args(['d', '-c', 'c.pth', '--patch-size', '250', '-m', 'wesup']).patch_size == 250
    for bad in (['d'], ['-c', 'c.pth'], ['d', '-c', 'c.pth', '-m', 'fcn']):            # checkpoint / root required; wesup only
        with pytest.raises(SystemExit):
            S.parse_args(bad)


def test_output_directories_and_stem_groups():
    from wesup_amd import slide as S
    ckpt = 'records/20190701/checkpoints/ckpt.0100.pth'
    assert S.output_dir_for(ckpt) == Path('records/20190701/combined-results-for-ckpt.0100.pth')
    assert S.output_dir_for(ckpt, pixel=True) == Path('records/20190701/combined-results-pixel-for-ckpt.0100.pth')
    assert S.output_dir_for('~/r/ckpts/c.pth') == Path.home() / 'r' / 'combined-results-for-c.pth'
    pos, neg = S.split_stems(['o/positive-b.png', 'o/negative-1.png', 'o/positive-a.png', 'o/other.png', 'o/negative-0.png'])
    assert [p.name for p in pos] == ['positive-a.png', 'positive-b.png']
    assert [p.name for p in neg] == ['negative-0.png', 'negative-1.png']


def test_skip_infer_scores_the_pngs_on_disk(tmp_path):
    from PIL import Image
    from wesup_amd import slide as S
    rs = np.random.RandomState(11)
    root, ckpt = tmp_path / 'val', tmp_path / 'record' / 'checkpoints' / 'ckpt.pth'
    out = tmp_path / 'record' / 'combined-results-for-ckpt.pth'
    (root / 'masks').mkdir(parents=True)
    out.mkdir(parents=True)
    maps = {}
    for stem, shape in (('positive-a', (37, 53)), ('positive-b', (20, 31)), ('negative-c', (41, 29))):
        maps[stem] = ((rs.rand(*shape) < 0.5).astype(np.uint8) * 255, (rs.rand(*shape) < 0.3).astype(np.uint8) * 255)
        Image.fromarray(maps[stem][0]).save(out / f'{stem}.png')
        Image.fromarray(maps[stem][1]).save(root / 'masks' / f'{stem}.png')
    lines = []
    got = S.main(root, ckpt, skip_infer=True, log=lambda *a: lines.append(' '.join(str(v) for v in a)))

    def ref(stems, negative):
        accs, dices = [], []
        for s in stems:
            P, G = maps[s]
            if negative:
                P, G = 255 - P, 255 - G
            accs.append((P == G).mean())
            dices.append(2 * ((G > 0) * (P > 0)).sum() / ((G > 0).sum() + (P > 0).sum() + 1e-7))
        return float(np.mean(accs)), float(np.mean(dices))
    assert got == {'positive': ref(['positive-a', 'positive-b'], False), 'negative': ref(['negative-c'], True)}
    assert lines == ['\nEvaluating positive OA and Dice ...', f'Accuracy: {got["positive"][0]}', f'Dice: {got["positive"][1]}',
                     '\nEvaluating negative OA and Dice ...', f'Accuracy: {got["negative"][0]}', f'Dice: {got["negative"][1]}']
    assert sorted(p.name for p in out.iterdir()) == ['negative-c.png', 'positive-a.png', 'positive-b.png']     # nothing written
    # a prediction without its mask is an error, not a shorter mean
    (root / 'masks' / 'positive-b.png').unlink()
    with pytest.raises(ValueError):
        S.main(root, ckpt, skip_infer=True, log=lambda *a: None)
