"""Mask post-processing and challenge scoring on the GPU (csrc/regions.hip, ops, utils/metrics_gpu.py, the device paths of
evaluate.py / infer.py / the trainer's validation phase) against scipy / numpy and the CPU functions.

Everything is integer image processing, so every comparison is EXACT -- array_equal for maps and tables, == for the float
metrics (the float formulas are the same host code fed the same integers) -- except against the reference's own outputs in
tests/golden/metrics.npz, where the bar is the CPU test's (1e-9 relative, tests/test_oracle_golden.py)."""
import csv
import math
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
S4 = ndimage.generate_binary_structure(2, 1)
S8 = np.ones((3, 3), dtype=np.int32)


def _dev(a, dtype=torch.uint8):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype).contiguous()


def _same(a, b):
    """== for floats, with nan equal to nan."""
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def _golden_masks(golden_dir):
    out = []
    fx = np.load(os.path.join(golden_dir, 'metrics.npz'))
    for i in range(int(fx['n'])):
        out += [fx[f'S{i}'], fx[f'G{i}']]
    g = np.load(os.path.join(golden_dir, 'postprocess.npz'))
    for i in range(int(g['n'])):
        shape = tuple(int(v) for v in g[f'shape{i}'])
        out.append(np.unpackbits(g[f'in{i}'])[:shape[0] * shape[1]].reshape(shape))
    return out


def _check_labels(mask, value=1):
    from wesup_amd import ops
    for conn, st in ((4, S4), (8, S8)):
        want, n = ndimage.label((np.asarray(mask) != 0) == bool(value), structure=st)
        got, gn = ops.cc_label(_dev(mask), conn, value)
        assert int(gn.cpu()[0]) == n, (mask.shape, conn, int(gn.cpu()[0]), n)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (mask.shape, conn)


# ------------------------------------------------------------------------------------------------ connected components
def test_cc_label_matches_scipy_on_the_fixture_masks(golden_dir):
    for m in _golden_masks(golden_dir):
        _check_labels(m)
        _check_labels(m, value=0)                          # the hole pass labels the background


@pytest.mark.parametrize('density', [0.30, 0.407, 0.593])
def test_cc_label_matches_scipy_on_noise(density):
    """0.407 and 0.593 are the site-percolation thresholds of the 8- and 4-connected lattice: long winding components that
    cross many tiles.  1024 x 1024 has exactly 1024 scan blocks per image, 1025 x 1024 one more: the second round of the scan of
    the block totals holds one value, which the carry of the first must reach (csrc/scan.hpp; last, so the masks of the
    other shapes are the ones they always were)."""
    rs = np.random.RandomState(int(density * 1000))
    for shape in ((522, 775), (1024, 1024), (7, 9), (1025, 1024)):
        m = (rs.rand(*shape) < density).astype(np.uint8)
        _check_labels(m)
        _check_labels(m, value=0)


def test_cc_label_patterns_and_odd_shapes():
    rs = np.random.RandomState(3)
    yy, xx = np.mgrid[0:97, 0:131]
    for m in (((yy + xx) & 1).astype(np.uint8), np.ones((97, 131), np.uint8), np.zeros((97, 131), np.uint8),
              (((yy // 16) + (xx // 16)) & 1).astype(np.uint8), ((yy % 16 == 15) | (xx % 16 == 0)).astype(np.uint8)):
        _check_labels(m)
        _check_labels(m, value=0)
    for shape in ((1, 1), (1, 97), (97, 1), (7, 9), (16, 16), (17, 33)):
        for k in range(3):
            m = (rs.rand(*shape) < (0.3, 0.6, 1.1)[k]).astype(np.uint8)
            _check_labels(m)
            _check_labels(m, value=0)
    _check_labels(np.array([[0]], np.uint8))
    _check_labels(np.array([[7]], np.uint8))              # any non-zero value is foreground


def test_cc_label_batch_of_three_different_images():
    from wesup_amd import ops, synth
    rs = np.random.RandomState(11)
    batch = np.stack([synth.gland_map(1, 200, 260, 6, 10, 30), (rs.rand(200, 260) < 0.5).astype(np.uint8),
                      np.zeros((200, 260), np.uint8)])
    for conn, st in ((4, S4), (8, S8)):
        got, n = ops.cc_label(_dev(batch), conn, 1)
        for b in range(3):
            want, wn = ndimage.label(batch[b], structure=st)
            assert int(n.cpu()[b]) == wn and np.array_equal(got[b].cpu().numpy(), want), (conn, b)
    with pytest.raises(Exception):
        ops.cc_label(_dev(batch), 5, 1)


# ------------------------------------------------------------------------------------------------ small regions
def test_remove_small_regions_matches_the_reference_outputs(golden_dir):
    from wesup_amd import ops
    from wesup_amd.evaluate import remove_small_regions
    g = np.load(os.path.join(golden_dir, 'postprocess.npz'))
    assert int(g['n']) == 6
    for i in range(int(g['n'])):
        shape = tuple(int(v) for v in g[f'shape{i}'])
        n = shape[0] * shape[1]
        m = np.unpackbits(g[f'in{i}'])[:n].reshape(shape)
        want = np.unpackbits(g[f'out{i}'])[:n].reshape(shape)
        got = ops.remove_small_regions(_dev(m), 2000)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), i
        via = remove_small_regions(m.astype(np.float64), device=DEV)
        assert via.dtype == np.float64 and np.array_equal(via, want.astype(np.float64)), i


def test_remove_small_regions_matches_the_cpu_function_at_glas_size():
    from wesup_amd import ops, synth
    from wesup_amd.evaluate import remove_small_regions
    rs = np.random.RandomState(2)
    masks = []
    for seed in range(3):
        m = synth.gland_map(seed, 522, 775)
        m[rs.rand(522, 775) < 0.002] ^= 1                 # specks and pin holes
        for _ in range(12):                                # regions on both sides of either threshold
            y, x, s = rs.randint(0, 460), rs.randint(0, 700), rs.randint(3, 60)
            m[y:y + s, x:x + s] = rs.randint(0, 2)
        masks.append(m)
    for min_size in (2000, 50):
        for m in masks:
            want = remove_small_regions(m, min_size)
            assert (want != m).any()
            assert np.array_equal(ops.remove_small_regions(_dev(m), min_size).cpu().numpy(), want.astype(np.uint8)), min_size
        got = ops.remove_small_regions(_dev(np.stack(masks)), min_size).cpu().numpy()
        for b, m in enumerate(masks):
            assert np.array_equal(got[b], remove_small_regions(m, min_size).astype(np.uint8)), (min_size, b)


# ------------------------------------------------------------------------------------------------ morphology
def test_binary_morph_matches_scipy():
    from wesup_amd import ops, synth
    from wesup_amd.infer import _cross
    rs = np.random.RandomState(4)
    border = np.zeros((61, 83), np.uint8)
    border[:3], border[-2:], border[:, :4], border[:, -1:] = 1, 1, 1, 1
    border[20:44, 30:60] = 1
    frame = np.ones((40, 50), np.uint8)
    frame[6:30, 9:41] = 0
    masks = [synth.gland_map(0, 522, 775), synth.gland_map(1, 200, 260, 8, 8, 30), (rs.rand(120, 150) < 0.5).astype(np.uint8),
             (rs.rand(64, 64) < 0.9).astype(np.uint8), border, frame, np.ones((1, 1), np.uint8), (rs.rand(1, 40) < 0.7).astype(np.uint8),
             (rs.rand(5, 3) < 0.7).astype(np.uint8)]
    line = np.ones((1, 5))
    lopsided = np.zeros((4, 3))
    lopsided[0, 0] = lopsided[3, 1] = lopsided[2, 2] = 1
    for fp in (_cross(9), np.ones((3, 3)), line, lopsided, np.ones((2, 2))):
        for m in masks:
            x = m.astype(np.float64)
            d = _dev(m)
            for op, ref in ((ops.MORPH_OPEN, ndimage.grey_opening), (ops.MORPH_ERODE, ndimage.grey_erosion),
                            (ops.MORPH_DILATE, ndimage.grey_dilation)):
                want = ref(x, footprint=fp)
                got = ops.binary_morph(d, fp, op)
                assert np.array_equal(got.cpu().numpy(), want.astype(np.uint8)), (fp.shape, m.shape, op)
    assert np.array_equal(ops.binary_opening(_dev(np.stack(masks[4:5] * 2)), _cross(9)).cpu().numpy()[1],
                          ndimage.grey_opening(border.astype(np.float64), footprint=_cross(9)).astype(np.uint8))


# ------------------------------------------------------------------------------------------------ tables and lists
def test_contingency_matches_bincount_on_gland_pairs():
    from wesup_amd import ops, synth
    from wesup_amd.utils import metrics as M
    for seed in range(4):
        S, G = synth.gland_pair(seed)
        Sl, Gl = M.label(S).astype(np.int32), M.label(G).astype(np.int32)
        want, nS, nG = M._contingency(Sl, Gl)
        got, status = ops.contingency(_dev(Sl, torch.int32), _dev(Gl, torch.int32), nS, nG)
        assert int(status.cpu()[0]) == 0 and np.array_equal(got.cpu().numpy(), want), seed
    _, status = ops.contingency(_dev(Sl, torch.int32), _dev(Gl, torch.int32), nS - 1, nG)
    assert int(status.cpu()[0]) == 1                       # a label outside the table is reported, not written
    both, st2 = ops.contingency(_dev(np.stack([Sl, Gl]), torch.int32), _dev(np.stack([Gl, Sl]), torch.int32), max(nS, nG), max(nS, nG))
    assert np.array_equal(both[0].cpu().numpy()[:nS + 1, :nG + 1], want) and np.array_equal(both[1].cpu().numpy()[:nG + 1, :nS + 1], want.T)
    with pytest.raises(Exception):
        ops.contingency(_dev(Sl, torch.int32), _dev(Gl, torch.int32), 8191, 8192)


def _boundary(lab):
    p = np.pad(lab, 1, constant_values=-1)
    c = p[1:-1, 1:-1]
    return (lab > 0) & ((p[:-2, 1:-1] != c) | (p[2:, 1:-1] != c) | (p[1:-1, :-2] != c) | (p[1:-1, 2:] != c))


def test_label_sort_matches_a_stable_argsort():
    from wesup_amd import ops, synth
    from wesup_amd.utils import metrics as M
    rs = np.random.RandomState(8)
    maps = [M.label(synth.gland_pair(0)[0]), M.label(rs.rand(150, 170) < 0.35), rs.randint(0, 40, (33, 70)), np.zeros((9, 7), np.int64),
            M.label(rs.rand(300, 300) < 0.3)]
    for lab in maps:
        lab = lab.astype(np.int32)
        L = int(lab.max())
        out = ops.label_sort(_dev(lab, torch.int32), L)
        assert int(out.status.cpu()[0]) == 0
        flat = lab.ravel()
        assert np.array_equal(out.pix.cpu().numpy(), np.argsort(flat, kind='stable'))
        start = out.start.cpu().numpy()
        assert np.array_equal(start, np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=L + 1))]))
        edge = _boundary(lab).ravel()
        key = np.where(edge, flat, L + 1)
        order = np.argsort(key, kind='stable')[:int(edge.sum())]
        bstart = out.bstart.cpu().numpy()
        assert np.array_equal(bstart, np.concatenate([[0], np.cumsum(np.bincount(flat[edge], minlength=L + 1))]))
        assert np.array_equal(out.bpix.cpu().numpy()[:bstart[-1]], order)
    two = np.stack([maps[1], maps[1][::-1]]).astype(np.int32)
    out = ops.label_sort(_dev(two, torch.int32), int(two.max()))
    for b in range(2):
        assert np.array_equal(out.pix[b].cpu().numpy(), np.argsort(two[b].ravel(), kind='stable'))
    assert int(ops.label_sort(_dev(maps[2].astype(np.int32), torch.int32), 20).status.cpu()[0]) == 1


def _d2(A, B):
    a, b = np.argwhere(A).astype(np.int64), np.argwhere(B).astype(np.int64)
    worst = 0
    for i in range(0, len(a), 256):
        worst = max(worst, int(((a[i:i + 256, None, :] - b[None, :, :]) ** 2).sum(-1).min(1).max()))
    return worst


def test_directed_hausdorff_sq_matches_brute_force():
    from wesup_amd import ops
    H, W = 300, 400
    yy, xx = np.mgrid[0:H, 0:W]
    X, Y = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
    X[(yy - 60) ** 2 + (xx - 70) ** 2 <= 30 ** 2] = 1              # ~2 800 pixels
    Y[(yy - 66) ** 2 + (xx - 80) ** 2 <= 31 ** 2] = 1              # overlaps X's 1
    X[100:120, 100:140] = 2
    Y[90:140, 90:160] = 2                                          # X's 2 inside Y's 2: 0 one way, not the other
    X[250, 390] = 3                                                # single pixels, far apart
    Y[5, 3] = 3
    X[200:230, 20:110] = 4                                         # 2 700 pixels, hollow partner below
    Y[195:240, 10:120] = 4
    Y[205:225, 30:100] = 0
    X[290:300, 0:12] = 5                                           # touching two borders
    Y[150, 200:260] = 5                                            # a line
    Y[0:54, 340:400] = 6                                           # 3 240 pixels
    pairs = [(a, b) for a in range(1, 6) for b in range(1, 7)]
    LX, LY = ops.label_sort(_dev(X, torch.int32), 5), ops.label_sort(_dev(Y, torch.int32), 6)
    p = torch.tensor(pairs, dtype=torch.int32, device=DEV)
    fwd = ops.directed_hausdorff_sq(p, LX, LY).cpu().numpy()
    bwd = ops.directed_hausdorff_sq(p.flip(1).contiguous(), LY, LX).cpu().numpy()
    for (a, b), f, r in zip(pairs, fwd, bwd):
        assert f == _d2(X == a, Y == b), (a, b, 'forward')
        assert r == _d2(Y == b, X == a), (a, b, 'backward')
    assert fwd[pairs.index((2, 2))] == 0 and bwd[pairs.index((2, 2))] > 0
    assert fwd[pairs.index((3, 3))] == 245 ** 2 + 387 ** 2
    bad = ops.directed_hausdorff_sq(torch.tensor([[0, 1], [1, 7], [1, 1]], dtype=torch.int32, device=DEV), LX, LY).cpu().numpy()
    assert bad[0] == -1 and bad[1] == -1 and bad[2] == fwd[0]
    assert ops.directed_hausdorff_sq(p[:0], LX, LY).numel() == 0


# ------------------------------------------------------------------------------------------------ metrics
def test_gpu_metrics_match_the_reference_fixture(golden_dir):
    from wesup_amd.utils import metrics_gpu as MG
    fx = np.load(os.path.join(golden_dir, 'metrics.npz'))
    for i in range(int(fx['n'])):
        S, G, want = fx[f'S{i}'], fx[f'G{i}'], fx[f'v{i}']
        sc = MG.challenge_scores(_dev(S), _dev(G))
        for got in ([MG.detection_f1(S, G), MG.object_dice(S, G), MG.object_hausdorff(_dev(S), G), MG.hausdorff(S, _dev(G))],
                    [sc['detection_f1'], sc['object_dice'], sc['object_hausdorff'], MG.hausdorff(_dev(S, torch.float32), G)]):
            for g, w in zip(got, want):
                if np.isnan(w):
                    continue
                assert (np.isinf(w) and np.isinf(g)) or abs(g - w) <= 1e-9 * max(1.0, abs(w)), (i, got, want)
        assert np.array_equal(MG.label(S).cpu().numpy(), ndimage.label(S, structure=S8)[0])


def _eight_pairs():
    from wesup_amd import synth
    H, W = 522, 775
    out = {}
    out['shifted copy + square'] = synth.gland_pair(0)
    out['shifted copy + square 2'] = synth.gland_pair(5)
    out['independent'] = (synth.gland_map(1), synth.gland_map(2))
    S, G = synth.gland_map(3, n=8), synth.gland_map(3, n=8)
    S[:70], G[:70], S[-70:], G[-70:] = 0, 0, 0, 0
    S[5:45, 10:60] = 1                                             # overlaps nothing in G
    G[-50:-8, -90:-20] = 1                                         # overlaps nothing in S
    out['an orphan on each side'] = (S, G)
    S, G = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    S[100:160, 100:300] = 1                                        # overlaps two ground-truth objects by 60 x 40 each
    G[90:170, 60:140] = 1
    G[90:170, 260:340] = 1
    G[300:400, 300:500] = 1                                        # and two segmented objects tie on this one
    S[310:390, 280:330] = 1
    S[310:390, 470:520] = 1
    out['exact overlap ties'] = (S, G)
    out['identical'] = (synth.gland_map(4), synth.gland_map(4))
    out['empty prediction'] = (np.zeros((H, W), np.uint8), synth.gland_map(6))
    out['empty ground truth'] = (synth.gland_map(6), np.zeros((H, W), np.uint8))
    return out


def test_gpu_metrics_equal_the_cpu_functions():
    from wesup_amd.evaluate import score
    from wesup_amd.utils import metrics as M
    from wesup_amd.utils import metrics_gpu as MG
    pairs = _eight_pairs()
    assert len(pairs) == 8
    fallback = ties = 0
    for name, (S, G) in pairs.items():
        C = M._contingency(M.label(S), M.label(G))[0]
        if C.shape[0] > 1 and C.shape[1] > 1:
            fallback += int((M._partner(C)[1:] == 0).any()) + int((M._partner(C.T)[1:] == 0).any())
            top = np.sort(C[1:, 1:], axis=1)
            ties += int(C.shape[1] > 2 and ((top[:, -1] == top[:, -2]) & (top[:, -1] > 0)).any())
        assert MG.detection_f1(S, G) == M.detection_f1(S, G), name
        assert MG.object_dice(_dev(S), _dev(G)) == M.object_dice(S, G), name
        assert MG.hausdorff(S, G) == M.hausdorff(S, G), name
        cpu_oh = float(M.object_hausdorff(S, G)) if S.any() and G.any() else float('nan')         # the guard of evaluate.score
        assert _same(float(MG.object_hausdorff(S, G)), cpu_oh), name
        sc = MG.challenge_scores(_dev(S), _dev(G))
        (row,), _ = score([S], [G])
        assert set(sc) == set(row)
        for k in row:
            assert _same(sc[k], row[k]), (name, k, sc[k], row[k])
        ids = (M.label(G) * 3).astype(np.uint8)                    # an object-id ground truth, as GlaS masks are
        (row_ids,), _ = score([S.astype(np.float64)], [ids])
        (dev_ids,), _ = score([S.astype(np.float64)], [ids], device=DEV)
        assert all(_same(dev_ids[k], row_ids[k]) for k in row_ids), (name, dev_ids, row_ids)
        sc_ids = MG.challenge_scores(S.astype(np.float64), ids)
        assert all(_same(sc_ids[k], row_ids[k]) for k in row_ids), (name, sc_ids, row_ids)
    assert fallback >= 3 and ties >= 1                             # the nearest-object branch and the tie rule were exercised


def test_oversized_table_is_scored_on_the_host_and_said_once(caplog):
    """Thousands of specks against thousands of specks: the table would exceed 2^26 cells, so it is not allocated; the image
    goes through the host functions and the module says so once."""
    import logging
    from wesup_amd import ops
    from wesup_amd.utils import metrics as M
    from wesup_amd.utils import metrics_gpu as MG
    rs = np.random.RandomState(21)
    S, G = (rs.rand(400, 500) < 0.06).astype(np.uint8), (rs.rand(400, 500) < 0.06).astype(np.uint8)
    nS, nG = ndimage.label(S, structure=S8)[1], ndimage.label(G, structure=S8)[1]
    assert (nS + 1) * (nG + 1) > ops.CONTINGENCY_MAX_CELLS and max(nS, nG) < ops.LABEL_SORT_MAX_LABELS
    MG._said.discard('table')
    with caplog.at_level(logging.WARNING, logger='wesup_amd.utils.metrics_gpu'):
        lab = MG._Labelled(S, G)
        assert lab.C is None and (lab.nS, lab.nG) == (nS, nG)
        assert MG.detection_f1(_dev(S), G) == M.detection_f1(S, G)
        assert MG.object_dice(S, _dev(G)) == M.object_dice(S, G)
    assert sum('contingency table' in r.getMessage() for r in caplog.records) == 1


# ------------------------------------------------------------------------------------------------ drivers
def test_evaluate_glas_on_the_device_equals_the_host_driver(tmp_path):
    from PIL import Image
    from wesup_amd.evaluate import evaluate_glas
    rs = np.random.RandomState(0)
    yy, xx = np.mgrid[0:160, 0:200]

    def blobs(k):
        m = np.zeros((160, 200), dtype=np.uint8)
        for j in range(k):
            cy, cx, r = rs.randint(30, 130), rs.randint(30, 170), rs.randint(28, 40)
            m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = j + 1
        return m
    for root in ('host', 'dev'):
        rs = np.random.RandomState(0)
        for split in ('testA', 'testB'):
            os.makedirs(tmp_path / root / 'pred' / split)
            os.makedirs(tmp_path / root / 'gt' / split / 'masks')
            for i in range(2):
                gt = blobs(2)
                pred = (gt > 0).astype(np.uint8)
                pred[5:15, 5:15] = 1                      # a 100-pixel speck: must be removed by the post-processing
                pred[60:64, 90:95] = 0                    # and a pin hole, most likely inside a blob
                Image.fromarray(pred * 255).save(tmp_path / root / 'pred' / split / f'im{i}.bmp')
                Image.fromarray(gt).save(tmp_path / root / 'gt' / split / 'masks' / f'im{i}.bmp')
    host_lines, dev_lines = [], []
    host = evaluate_glas(tmp_path / 'host' / 'pred', tmp_path / 'host' / 'gt', log=host_lines.append)
    dev = evaluate_glas(tmp_path / 'dev' / 'pred', tmp_path / 'dev' / 'gt', log=dev_lines.append, device=DEV)
    assert host == dev and host_lines == dev_lines and set(dev) == {'testA', 'testB'}
    for split in ('testA', 'testB'):
        assert dev[split]['detection_f1'] == pytest.approx(1.0)
        assert list(csv.reader(open(tmp_path / 'host' / 'pred' / f'{split}.csv'))) == \
            list(csv.reader(open(tmp_path / 'dev' / 'pred' / f'{split}.csv')))
        for i in range(2):
            a = np.asarray(Image.open(tmp_path / 'host' / 'pred-new' / split / f'im{i}.bmp'))
            b = np.asarray(Image.open(tmp_path / 'dev' / 'pred-new' / split / f'im{i}.bmp'))
            assert np.array_equal(a, b) and b[10, 10] == 0 and b.max() == 255


def test_predict_with_the_opening_on_the_device_equals_the_default(tmp_path):
    from tests.test_data_cpu import _make_dataset
    from wesup_amd import infer as I
    from wesup_amd.models import initialize_trainer
    _make_dataset(str(tmp_path / 'val'), n=2, H=72, W=88, with_points=False)
    trainer = initialize_trainer('wesup', device=DEV, sp_area=64)
    trainer.model.eval()
    ds = I.SegmentationDataset(tmp_path / 'val', train=False)
    host = I.predict(trainer, ds, scales=(0.5, 1.0), device=DEV)
    dev = I.predict(trainer, ds, scales=(0.5, 1.0), device=DEV, device_post=True)
    assert len(host) == len(dev) == 2
    for a, b in zip(host, dev):
        assert a.dtype == b.dtype and a.shape == b.shape == (72, 88) and np.array_equal(a, b)
    one = I.predict(trainer, ds, scales=(0.5,), device=DEV, device_post=True)             # a single scale is not opened
    assert all(np.array_equal(a, b) for a, b in zip(one, I.predict(trainer, ds, scales=(0.5,), device=DEV)))
    mean_h, rows_h = I.evaluate_predictions(host, ds)
    mean_d, rows_d = I.evaluate_predictions(dev, ds, device=DEV)
    assert all(_same(float(a[k]), float(b[k])) for a, b in zip(rows_h, rows_d) for k in a)
    assert all(_same(mean_h[k], mean_d[k]) for k in mean_h)


def test_validation_phase_fills_the_challenge_columns():
    from oracle import wesup_oracle as orc
    from wesup_amd import synth
    from wesup_amd.models import initialize_trainer
    from wesup_amd.utils import metrics_gpu as MG
    from wesup_amd.utils.metrics import accuracy, dice
    H, W, g = 96, 96, 6
    t = initialize_trainer('wesup', device=DEV, max_superpixels=g * g)
    t.model.load_state_dict({k: torch.from_numpy(v) for k, v in orc.make_weights(3, feat_scale=0.05).items()})
    t.optimizer, t.scheduler = t.get_default_optimizer()
    t.metric_funcs = [accuracy, dice]
    t.kwargs['val_metrics'] = [MG.detection_f1, MG.object_dice, MG.object_hausdorff]
    batches = []
    for i in range(2):
        imgs, labs, pts, pix = synth.make_batch(100 + i, 1, H, W, g)
        batches.append(tuple(torch.from_numpy(a).to(DEV) for a in (imgs, pix, pts, labs)))
    # the train phase is unchanged: no challenge column appears there
    t.model.train(); t.tracker.train()
    t.train_one_iteration('train', *batches[0])
    assert not any('detection_f1' in k or 'object_' in k for k in t.tracker.history)
    t.model.eval(); t.tracker.eval()
    want = []
    for data in batches:
        t.train_one_iteration('val', *data)
        with torch.no_grad():
            input_, target = t.preprocess(*data)
            pred_, target_ = t.postprocess(t.model(input_), target)
        want.append(MG.challenge_scores(pred_[0], target_[0]))
    hist = t.tracker.history
    for k in ('detection_f1', 'object_dice', 'object_hausdorff'):
        assert len(hist['val_' + k]) == 2, sorted(hist)
        for got, w in zip(hist['val_' + k], want):
            assert _same(float(got), float(w[k])), (k, got, w[k])
    assert len(hist['val_accuracy']) == 2 and len(hist['val_dice']) == 2      # the fast metrics are still there
    assert set(t.tracker.epoch_means('val')) >= {'val_detection_f1', 'val_object_dice', 'val_object_hausdorff'}
