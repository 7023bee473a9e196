"""Splitting touching objects on the GPU (csrc/split.hip, ops.edt_sq / label_grow / label_cut / split_objects, the device paths
of split.py and evaluate.py) against the numpy definitions in wesup_amd/split.py.

Everything is integer image processing, so every comparison is EXACT (array_equal for maps, == for the rows of scores)."""
import numpy as np
import pytest
import torch

from _splitcases import (EDT_CASES, RADII, check_properties, disc_scene, random_mask, random_seeds, serpentine, serpentine_ends,
                         write_scene)
from wesup_amd import _lib, evaluate, split
from wesup_amd.utils import metrics as M

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEG, ROWS = _lib.SPLIT_SEG, _lib.SPLIT_ROWS          # the row pass stages ROWS rows of SEG pixels per block
TILE, HALO = _lib.SPLIT_TILE, _lib.SPLIT_HALO        # the growth kernel's tile edge and halo


def _dev(a, dtype=torch.uint8):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype).contiguous()


def _ops():
    from wesup_amd import ops
    return ops


def _edt_equal(F, cap):
    got = _ops().edt_sq(_dev(F), cap)
    assert got.dtype == torch.int32 and tuple(got.shape) == F.shape
    assert np.array_equal(got.cpu().numpy(), split.edt_sq_host(F, cap))


@pytest.mark.parametrize('h,w,dens', EDT_CASES)
def test_edt_sq_cpu_shapes(h, w, dens):
    F = random_mask(h, w, dens, seed=h * 1000 + w)
    for r in RADII:
        _edt_equal(F, r * r)


def test_edt_sq_halo_wider_than_any_tile():
    F = random_mask(70, 300, 0.02, seed=70300)
    _edt_equal(F, 254 * 254)
    _edt_equal(F, 65025)
    sparse = np.ones((70, 300), np.uint8)
    sparse[35, 3] = 0                                 # one zero: the nearest background is up to 296 columns away
    _edt_equal(sparse, 65025)
    _edt_equal(sparse, 100 * 100 + 1)                 # a cap that is no square


@pytest.mark.parametrize('edge', (SEG, TILE, ROWS))
def test_edt_sq_sizes_around_the_segment_and_tile_edges(edge):
    for h in (edge - 1, edge, edge + 1):
        for w in (edge - 1, edge, edge + 1, 2 * SEG + 1):
            F = random_mask(h, w, 0.03, seed=h * 977 + w)
            _edt_equal(F, 17 * 17)
            _edt_equal(F, 3 * 3)


def test_edt_sq_batch_and_thin_images():
    rnd = random_mask(37, 53, 0.05, seed=5)
    B = np.stack([rnd, np.ones_like(rnd), np.zeros_like(rnd)])
    for cap in (1, 9, 400, 65025):
        _edt_equal(B, cap)
    _edt_equal(random_mask(1, 131, 0.05, seed=6), 400)       # H = 1
    _edt_equal(random_mask(131, 1, 0.05, seed=7), 400)       # W = 1
    _edt_equal(np.ones((1, 1), np.uint8), 4)
    ops = _ops()
    for cap in (0, 65026):
        with pytest.raises(_lib.WesupHipError):
            ops.edt_sq(_dev(rnd), cap)


def _grow_equal(F, S, **kw):
    ops = _ops()
    got, launches = ops.label_grow(_dev(F), _dev(S, torch.int32), return_launches=True, **kw)
    want, rounds = split.label_grow_host(F, S, return_rounds=True)
    assert got.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy(), want)
    return got, launches, rounds


def test_label_grow_serpentine():
    F = serpentine()
    a, b = serpentine_ends(F)
    S = np.zeros(F.shape, np.int32)
    S[a] = 1
    got, launches, rounds = _grow_equal(F, S)
    assert np.array_equal(got.cpu().numpy(), F.astype(np.int32))
    assert rounds > 1000 and launches * HALO >= rounds - 2 and launches > 100     # fronts cross many tiles over many launches
    S[b] = 2
    got, _, _ = _grow_equal(F, S)
    L = got.cpu().numpy()
    assert set(np.unique(L[F != 0])) == {1, 2}
    out = _ops().label_cut(_dev(F), got).cpu().numpy()
    assert np.array_equal(out, split.label_cut_host(F, L)) and M.label(out).max() == 2


@pytest.mark.parametrize('density', (0.55, 0.6))
def test_label_grow_noise_batch(density):
    rng = np.random.default_rng(int(density * 100))
    F = (rng.random((3, 97, 131)) < density).astype(np.uint8)
    S = np.stack([random_seeds(F[i], 40, seed=11 + i) for i in range(3)])
    assert (S.max(axis=(1, 2)) > 2 ** 20).all()
    got, _, _ = _grow_equal(F, S)
    L = got.cpu().numpy()
    out = _ops().label_cut(_dev(F), got).cpu().numpy()
    assert np.array_equal(out, split.label_cut_host(F, L))
    for i in range(3):
        check_properties(F[i], S[i], L[i], out[i])


def test_label_grow_seeds_on_tile_corners_and_border():
    h, w = 2 * TILE + 5, 3 * TILE + 1
    F = random_mask(h, w, 0.25, seed=41)
    S = np.zeros((h, w), np.int32)
    lab = 2 ** 30
    for y in (0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, h - 1):
        for x in (0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, 3 * TILE - 1, 3 * TILE, w - 1):
            F[y, x] = 1
            S[y, x] = lab
            lab -= 1237
    S[5, 7], F[5, 7] = 77, 0                          # a seed on the background and a negative seed count as no label
    S[9, 9] = -5
    got, _, _ = _grow_equal(F, S)
    assert got.cpu().numpy()[5, 7] == 0
    full = np.ones((h, w), np.uint8)                  # no background at all: the fronts meet in the open
    _grow_equal(full, S)
    for hh, ww in ((TILE - 1, TILE + 1), (TILE, TILE), (TILE + 1, TILE - 1), (1, 2 * TILE + 3), (2 * TILE + 3, 1)):
        Fs = random_mask(hh, ww, 0.1, seed=hh * 31 + ww)
        Ss = np.zeros((hh, ww), np.int32)
        Ss[0, 0], Ss[hh - 1, ww - 1] = 9, 4
        _grow_equal(Fs, Ss)


def test_label_grow_largest_label():
    """2^31 - 1 is a label like any other: it spreads across tiles, alone and against smaller labels."""
    top = 2 ** 31 - 1
    h, w = TILE + 3, 2 * TILE + 5
    F = random_mask(h, w, 0.1, seed=77)
    F[0], F[:, 0] = 1, 1
    S = np.zeros((h, w), np.int32)
    S[0, 0] = top
    got, _, _ = _grow_equal(F, S)
    L = got.cpu().numpy()
    assert (L[M.label(F) == M.label(F)[0, 0]] == top).all()
    S[0, w - 1], S[h - 1, 0] = top - 1, 3
    got, _, _ = _grow_equal(F, S)
    L = got.cpu().numpy()
    assert {3, top - 1, top} <= set(np.unique(L))
    assert np.array_equal(_ops().label_cut(_dev(F), got).cpu().numpy(), split.label_cut_host(F, L))
    line = np.ones((1, 5), np.uint8)                  # next to unlabelled foreground, nothing else around
    Sl = np.array([[top, 0, 0, 0, 0]], np.int32)
    got, _, _ = _grow_equal(line, Sl)
    assert got.cpu().numpy().tolist() == [[top] * 5]


def test_label_grow_cadences_agree():
    rng = np.random.default_rng(3)
    F = (rng.random((97, 131)) < 0.6).astype(np.uint8)
    S = random_seeds(F, 40, seed=19)
    a, la, _ = _grow_equal(F, S, cadence=1)
    b, lb, _ = _grow_equal(F, S, cadence=5)
    c, _, _ = _grow_equal(F, S, cadence=3, rounds=2)
    assert torch.equal(a, b) and torch.equal(a, c) and lb % 5 == 0 and lb >= la
    ops = _ops()
    for kw in ({'rounds': 3}, {'rounds': HALO + 2}, {'cadence': 0}):
        with pytest.raises(_lib.WesupHipError):
            ops.label_grow(_dev(F), _dev(S, torch.int32), **kw)


def test_label_cut():
    ops = _ops()
    rng = np.random.default_rng(8)
    for shape in ((61, 67), (3, 33, 65)):
        F = (rng.random(shape) < 0.8).astype(np.uint8)
        L = rng.integers(0, 4, size=shape).astype(np.int32) * (2 ** 28)           # few labels: many equal neighbours
        L[rng.random(shape) < 0.3] = 0
        got = ops.label_cut(_dev(F), _dev(L, torch.int32))
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), split.label_cut_host(F, L))
    F = np.ones((4, 6), np.uint8)
    same = np.full((4, 6), 7, np.int32)                                            # equal labels side by side: no cut
    assert ops.label_cut(_dev(F), _dev(same, torch.int32)).cpu().numpy().all()
    junction = np.array([[1, 1, 1, 2, 2, 2],
                         [1, 1, 1, 2, 2, 2],
                         [3, 3, 3, 3, 3, 3],
                         [3, 3, 3, 3, 3, 3]], np.int32)
    want = np.array([[1, 1, 1, 0, 1, 1],
                     [1, 1, 1, 0, 1, 1],
                     [0, 0, 0, 0, 0, 0],
                     [1, 1, 1, 1, 1, 1]], np.uint8)
    assert np.array_equal(split.label_cut_host(F, junction), want)
    assert np.array_equal(ops.label_cut(_dev(F), _dev(junction, torch.int32)).cpu().numpy(), want)


def _split_equal(F, radius):
    ops = _ops()
    out, L = ops.split_objects(_dev(F), radius, return_labels=True)
    want, wantL = split.split_objects(F, radius, return_labels=True)
    out, L = out.cpu().numpy(), L.cpu().numpy()
    assert out.dtype == np.uint8 and np.array_equal(out, want) and np.array_equal(L, wantL)
    assert np.array_equal(ops.split_objects(_dev(F), radius).cpu().numpy(), want)
    r2 = radius * radius
    seeds = M.label(split.edt_sq_host(F, r2) >= r2)
    check_properties(F, seeds, L, out)
    return out, int(seeds.max())


@pytest.mark.parametrize('radius', (12, 16, 20, 31))
def test_split_objects_disc_scene(radius):
    pred, gt = disc_scene()
    out, n_seeds = _split_equal(pred, radius)
    if radius == 31:
        assert n_seeds == 0 and np.array_equal(out, pred)
    else:
        assert n_seeds == 2 and M.label(out).max() == 2
        assert M.detection_f1(out, gt) > 0.9999 and M.object_hausdorff(out, gt) == 4.0
    assert np.array_equal(split.split_objects(pred, radius, device=DEV), out)      # the device path of split.py


def test_split_objects_glas_size_scene():
    rng = np.random.default_rng(522775)
    H, W = 522, 775
    yy, xx = np.mgrid[:H, :W]
    F = np.zeros((H, W), np.uint8)
    for _ in range(25):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(22, 60)
        F[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    n_before = int(M.label(F).max())
    out, n_seeds = _split_equal(F, 20)
    assert n_seeds > n_before and M.label(out).max() >= n_seeds                    # merged discs were separated
    assert np.array_equal(_ops().split_objects(_dev(F), 1).cpu().numpy(), F)       # radius 1: the identity
    B = np.stack([F, F[::-1], np.zeros_like(F)])
    assert np.array_equal(_ops().split_objects(_dev(B), 20).cpu().numpy(), split.split_objects(B, 20))


def test_evaluate_split_on_device(tmp_path):
    pred_dir, gt_dir = write_scene(tmp_path)
    quiet = lambda *a: None
    rows_h, means_h = evaluate.evaluate_split(pred_dir, gt_dir, None, None, 100, quiet, split_radius=16)
    rows_d, means_d = evaluate.evaluate_split(pred_dir, gt_dir, tmp_path / 'new', None, 100, quiet, DEV, split_radius=16)
    assert rows_d == rows_h and means_d == means_h
    assert rows_d[0]['detection_f1'] > 0.9999 and rows_d[0]['object_hausdorff'] == 4.0
    rows_0, _ = evaluate.evaluate_split(pred_dir, gt_dir, None, None, 100, quiet, DEV)
    assert rows_0[0]['detection_f1'] < 0.67                                        # without the flag: today's numbers
    from PIL import Image
    pred, _ = disc_scene()
    assert np.array_equal(np.asarray(Image.open(tmp_path / 'new' / 'scene.png')), split.split_objects(pred, 16) * 255)
