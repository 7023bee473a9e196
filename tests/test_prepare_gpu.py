"""Weak-label preparation on the GPU (csrc/prepare.hip, ops.label_stats / sp_vote / spl_paint, the ``device=`` paths of
wesup_amd/prepare.py) against numpy and the host paths, at the smallest shapes where each kernel can go wrong: an odd width,
a single row, a batch whose images have different id counts, one map whose table exceeds the LDS capacity (read from the
library) so that the global-atomics branch runs, L = 0, ids without a pixel, exact ties.

Everything is integer, or a float64 formed the same way on both sides: every comparison is == or array_equal."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
STEMS = ('a', 'b')


def _dev(a, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype).contiguous()


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'prepare.npz'))


@pytest.fixture(scope='module')
def big():
    """One map of 260 x 515 with more ids than either LDS table holds, every id non-empty."""
    from wesup_amd import ops, synth
    cap = max(ops.prepare_lds_entries())
    g = int(np.sqrt(cap)) + 1
    lab = synth.voronoi_labels(3, 260, 515, g).astype(np.int32)
    assert lab.max() + 1 == g * g > cap
    return lab


def _stats_ref(lab, L):
    lab = np.asarray(lab).astype(np.int64)
    H, W = lab.shape
    rows, cols = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    out = np.zeros((L + 1, 3), dtype=np.int64)
    out[:, 0] = np.bincount(lab.ravel(), minlength=L + 1)
    out[:, 1] = np.bincount(lab.ravel(), weights=rows.ravel(), minlength=L + 1).astype(np.int64)
    out[:, 2] = np.bincount(lab.ravel(), weights=cols.ravel(), minlength=L + 1).astype(np.int64)
    return out


def _vote_ref(lab, val, K):
    """numpy's way, in floats: values[sp].mean().round() cast to uint8, nothing painted for an id without pixels."""
    lab = np.asarray(lab).astype(np.int64)
    count = np.bincount(lab.ravel(), minlength=K)
    total = np.bincount(lab.ravel(), weights=val.ravel().astype(np.float64), minlength=K)
    with np.errstate(invalid='ignore', divide='ignore'):
        vote = np.where(count > 0, (total / count).round(), 0).astype(np.uint8)
    painted = vote[lab]
    return painted, int((painted == val).sum())


def _check_stats(lab, L):
    from wesup_amd import ops
    lab = np.asarray(lab)
    batched = lab.ndim == 3
    stats, status = ops.label_stats(_dev(lab), L)
    assert stats.dtype == torch.int64 and tuple(stats.shape) == ((lab.shape[0],) if batched else ()) + (L + 1, 3)
    assert not status.cpu().numpy().any()
    want = np.stack([_stats_ref(m, L) for m in lab]) if batched else _stats_ref(lab, L)
    assert np.array_equal(stats.cpu().numpy(), want)


def _check_vote(lab, val, K):
    from wesup_amd import ops
    lab, val = np.asarray(lab), np.asarray(val)
    batched = lab.ndim == 3
    painted, agree, status = ops.sp_vote(_dev(lab), _dev(val, torch.uint8), K)
    assert painted.dtype == torch.uint8 and painted.shape == tuple(lab.shape) and agree.dtype == torch.int64
    assert not status.cpu().numpy().any()
    refs = [_vote_ref(m, v, K) for m, v in zip(lab, val)] if batched else [_vote_ref(lab, val, K)]
    want = np.stack([r[0] for r in refs]) if batched else refs[0][0]
    assert np.array_equal(painted.cpu().numpy(), want)
    assert agree.cpu().tolist() == [r[1] for r in refs]
    none, agree2, _ = ops.sp_vote(_dev(lab), _dev(val, torch.uint8), K, paint=False)        # the map itself is optional
    assert none is None and agree2.cpu().tolist() == agree.cpu().tolist()


def _values(rs, shape, kind):
    if kind == 'binary':
        return (rs.rand(*shape) < 0.4).astype(np.uint8)
    if kind == 'mask255':
        return (rs.rand(*shape) < 0.5).astype(np.uint8) * 255
    return rs.randint(0, 256, shape).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ label_stats / sp_vote
def _small_maps():
    from wesup_amd import synth
    maps = {'37x53': (synth.voronoi_labels(1, 37, 53, 5).astype(np.int32), 25),
            '1x300': ((np.arange(300, dtype=np.int32) // 7)[None], 43),
            # a batch whose images have 16, 36 and 81 ids: the first two leave ids of the table without a pixel
            '3x96x80': (np.stack([synth.voronoi_labels(2 + i, 96, 80, g) for i, g in enumerate((4, 6, 9))]).astype(np.int32), 81)}
    return maps


@pytest.mark.parametrize('name', ['37x53', '1x300', '3x96x80'])
def test_label_stats_and_sp_vote_on_small_maps(name):
    lab, K = _small_maps()[name]
    rs = np.random.RandomState(len(name))
    _check_stats(lab, K - 1)
    _check_stats(lab, K + 2)                               # labels of the table without a pixel: zeros
    for kind in ('binary', 'mask255', 'many'):
        _check_vote(lab, _values(rs, lab.shape, kind), K)
    _check_vote(lab, _values(rs, lab.shape, 'many'), K + 3)


def test_tables_larger_than_lds_take_the_global_branch(big):
    from wesup_amd import ops
    K = int(big.max()) + 1
    assert K > max(ops.prepare_lds_entries())
    rs = np.random.RandomState(4)
    _check_stats(big, K - 1)
    _check_vote(big, _values(rs, big.shape, 'many'), K)
    _check_vote(big, _values(rs, big.shape, 'binary'), K)
    # the same map folded to few ids: the LDS branch at this size, more than one pass of the grid-stride loop aside
    small = big % 50
    _check_stats(small, 49)
    _check_vote(small, _values(rs, big.shape, 'many'), 50)


def test_single_label_and_capacity_edges():
    from wesup_amd import ops
    cap_stats, cap_vote = ops.prepare_lds_entries()
    zeros = np.zeros((37, 53), dtype=np.int32)
    _check_stats(zeros, 0)                                 # L = 0
    _check_vote(zeros, _values(np.random.RandomState(1), zeros.shape, 'many'), 1)
    # exactly at and one past the capacity: both sides of the threshold between the two kernels
    rs = np.random.RandomState(2)
    for cap, check in ((cap_stats, 'stats'), (cap_vote, 'vote')):
        for n in (cap, cap + 1):
            lab = rs.randint(0, n, (64, 131)).astype(np.int32)
            lab[0, :2] = (0, n - 1)
            if check == 'stats':
                _check_stats(lab, n - 1)
            else:
                _check_vote(lab, _values(rs, lab.shape, 'many'), n)


def test_sp_vote_ties_round_half_to_even():
    from wesup_amd import ops
    lab = np.zeros((4, 10), dtype=np.int32)
    val = np.zeros((4, 10), dtype=np.uint8)
    lab[0, 0:2], val[0, 0:2] = 1, (0, 1)                   # 0.5 -> 0 (even quotient)
    lab[0, 2:4], val[0, 2:4] = 2, (1, 2)                   # 1.5 -> 2 (odd quotient)
    lab[1, 0:4], val[1, 0:4] = 3, (2, 2, 3, 3)             # 2.5 -> 2
    lab[1, 4:8], val[1, 4:8] = 4, (254, 255, 255, 254)     # 254.5 -> 254
    lab[2, 0:3], val[2, 0:3] = 5, (1, 1, 2)                # 1.33 -> 1
    lab[2, 3:6], val[2, 3:6] = 6, (1, 2, 2)                # 1.67 -> 2
    lab[3, :], val[3, :] = 8, 255                          # 7 has no pixel; 255 stays 255
    painted, agree, status = ops.sp_vote(_dev(lab), _dev(val, torch.uint8), 9)
    p = painted.cpu().numpy()
    assert [int(p[lab == k][0]) for k in (1, 2, 3, 4, 5, 6, 8)] == [0, 2, 2, 254, 1, 2, 255]
    _check_vote(lab, val, 9)


@pytest.mark.parametrize('source', ['cc_label', 'slic'])
def test_label_maps_made_on_the_device(source):
    from wesup_amd import ops, synth
    rs = np.random.RandomState(7)
    if source == 'cc_label':
        mask = (rs.rand(2, 61, 83) < 0.45).astype(np.uint8)
        lab, n = ops.cc_label(_dev(mask, torch.uint8), 8, 1)
        K = int(n.max().item()) + 1
    else:
        img = np.stack([synth.synth_image(5 + i, 96, 80) for i in range(2)]).astype(np.float32)
        lab, n = ops.slic(_dev(img, torch.float32), 96 * 80 // 50, 20.0)
        K = int(n.max().item())
    host = lab.cpu().numpy()
    assert host.min() >= 0 and host.max() < K
    stats, status = ops.label_stats(lab, K - 1)
    assert not status.cpu().numpy().any() and np.array_equal(stats.cpu().numpy(), np.stack([_stats_ref(m, K - 1) for m in host]))
    val = _values(rs, host.shape, 'binary')
    painted, agree, _ = ops.sp_vote(lab, _dev(val, torch.uint8), K)
    refs = [_vote_ref(m, v, K) for m, v in zip(host, val)]
    assert np.array_equal(painted.cpu().numpy(), np.stack([r[0] for r in refs])) and agree.cpu().tolist() == [r[1] for r in refs]


def test_labels_outside_the_table_are_reported_not_written():
    from wesup_amd import ops
    lab = np.zeros((2, 9, 13), dtype=np.int32)
    lab[1, 4, 5], lab[1, 0, 0] = 7, -1
    stats, status = ops.label_stats(_dev(lab), 3)
    assert status.cpu().tolist() == [0, 1] and stats.cpu().numpy()[:, 0, 0].tolist() == [117, 115]
    assert not stats.cpu().numpy()[:, 1:].any()
    val = np.full(lab.shape, 3, dtype=np.uint8)
    painted, agree, status = ops.sp_vote(_dev(lab), _dev(val, torch.uint8), 3)
    assert status.cpu().tolist() == [0, 1] and agree.cpu().tolist() == [117, 115]
    assert painted.cpu().numpy()[1, 4, 5] == 0 and painted.cpu().numpy()[1, 0, 1] == 3


# ------------------------------------------------------------------------------------------------ spl_paint
def test_spl_paint_cases():
    from wesup_amd import ops, synth
    from wesup_amd import prepare as P
    seg = synth.voronoi_labels(9, 37, 53, 5).astype(np.int32)
    points = np.array([[3, 4, 0], [3, 5, 2],               # two classes in one superpixel (3, 5 lies beside 3, 4 ...)
                       [20, 30, 1], [20, 30, 1],           # a duplicate
                       [-1, -1, 2], [-37, -53, 1],         # wrapped negatives: the last and the first pixel
                       [36, 0, -1]])                       # a wrapped class
    points[1, :2] = np.argwhere(seg == seg[3, 4])[-1]      # ... made certain: another pixel of that very superpixel
    want = P.spl_mask(seg, points, n_classes=3)
    assert want[3, 4, 0] == 1 and want[3, 4, 2] == 1 and want[..., 1].any()
    assert np.array_equal(P.spl_mask(seg, points, n_classes=3, device=DEV), want)
    assert np.array_equal(P.spl_mask(_dev(seg), points, n_classes=3, device=DEV), want)   # a resident label map
    empty = P.spl_mask(seg, np.zeros((0, 3), dtype=np.int64), n_classes=3, device=DEV)
    assert empty.shape == (37, 53, 3) and empty.dtype == np.uint8 and not empty.any()
    for bad in ([37, 0, 0], [0, -54, 0], [0, 0, 3]):
        with pytest.raises(IndexError):
            P.spl_mask(seg, [bad], n_classes=3, device=DEV)
    # the entry itself reports what the caller should have wrapped, and writes nothing for it
    out, status = ops.spl_paint(_dev(seg), _dev(np.array([[-1, 0, 0], [0, 0, 3], [0, 53, 0]])), 25, 3)
    assert int(status.item()) == 2 and not out.cpu().numpy().any()
    out, status = ops.spl_paint(_dev(seg), _dev(np.array([[0, 0, 0]])), 5, 3)              # K too small for this map
    assert int(status.item()) & 1


# ------------------------------------------------------------------------------------------------ pipelines
@pytest.mark.parametrize('name', ['ring', 'wrap', 'many'])
def test_generate_points_goldens_on_the_device(gold, name):
    from wesup_amd import prepare as P
    rs = np.random.RandomState(int(gold[f'points_{name}_seed']))
    got = P.generate_points(gold[f'points_{name}_mask'], float(gold[f'points_{name}_ratio']), rs, device=DEV)
    assert got.dtype == np.int64 and np.array_equal(got, gold[f'points_{name}'])


def _point_masks():
    rs = np.random.RandomState(21)
    many = np.zeros((120, 150), dtype=np.uint8)            # a few hundred regions of 1 to 50 pixels, three classes
    for _ in range(420):
        h, w = rs.randint(1, 8), rs.randint(1, 8)
        y, x = rs.randint(0, 120 - h + 1), rs.randint(0, 150 - w + 1)
        many[y:y + h, x:x + w] = rs.randint(1, 4)
    border = np.zeros((40, 45), dtype=np.uint8)
    border[:3, :4] = 1                                     # a corner: candidates leave the image on two sides
    border[36:, 20:30] = 2
    border[10:20, 44] = 1
    return {'many': many, 'border': border, 'background only': np.zeros((33, 47), dtype=np.uint8),
            'no background': (1 + (np.arange(35)[:, None] // 9 + np.arange(41)[None] // 11) % 2).astype(np.uint8)}


@pytest.mark.parametrize('name', ['many', 'border', 'background only', 'no background'])
@pytest.mark.parametrize('ratio', [1e-4, 2e-3, 0.05])
def test_generate_points_device_equals_host(name, ratio):
    from wesup_amd import prepare as P
    mask = _point_masks()[name]
    for seed in (0, 1):
        host_rs, dev_rs = np.random.RandomState(seed), np.random.RandomState(seed)
        host = P.generate_points(mask, ratio, host_rs)
        dev = P.generate_points(mask, ratio, dev_rs, device=DEV)
        assert dev.dtype == host.dtype == np.int64 and np.array_equal(dev, host), (name, ratio, seed)
        assert host_rs.randint(1 << 30) == dev_rs.randint(1 << 30)                        # the same number of draws


def test_spl_masks_and_oracle_accuracy_goldens_on_the_device(gold, tmp_path):
    from wesup_amd import prepare as P
    for stem in STEMS:
        rows = np.array([[int(v) for v in line.split(',')] for line in gold[f'root_{stem}_csv'].tobytes().decode().split()])
        got = P.spl_mask(gold[f'root_{stem}_segments'], rows[:, [1, 0, 2]], n_classes=3, device=DEV)
        assert np.array_equal(got, gold[f'root_{stem}_spl']), stem
    for i, stem in enumerate(STEMS):
        mask = gold[f'search_{stem}_mask_half']
        for j, area in enumerate(gold['search_areas']):
            for k, comp in enumerate(gold['search_compactnesses']):
                acc = P.oracle_accuracy(gold[f'search_{stem}_segments_{area}_{comp}'], mask, device=DEV)
                assert isinstance(acc, np.float64) and acc == gold['search_accs'][i, j, k], (stem, area, comp)


def test_generate_spl_masks_with_the_device_slic(gold, tmp_path):
    """The default segmentation: whatever ops.slic returns for the image is what gets painted (SLIC parity itself is not pinned)."""
    from PIL import Image
    from wesup_amd import ops
    from wesup_amd import prepare as P
    root = tmp_path / 'data'
    (root / 'images').mkdir(parents=True)
    (root / 'points').mkdir()
    img = gold['root_a_image']
    Image.fromarray(img).save(root / 'images' / 'a.png')
    (root / 'points' / 'a.csv').write_bytes(gold['root_a_csv'].tobytes())
    written = P.generate_spl_masks(root, n_classes=2, sp_area=60, compactness=20, device=DEV, log=lambda *a: None)
    assert [w.name for w in written] == ['spl-masks']
    x = _dev(img, torch.uint8).permute(2, 0, 1)[None].float().div(255.0).contiguous()
    seg = ops.slic(x, img.shape[0] * img.shape[1] // 60, 20.0)[0][0].cpu().numpy()
    rows = np.array([[int(v) for v in line.split(',')] for line in gold['root_a_csv'].tobytes().decode().split()])
    assert np.array_equal(np.load(written[0] / 'a.npy'), P.spl_mask(seg, rows[:, [1, 0, 2]], n_classes=2))


def test_slic_search_equals_the_host_accuracy_of_the_device_label_maps(tmp_path, monkeypatch):
    from PIL import Image
    from wesup_amd import prepare as P
    rs = np.random.RandomState(33)
    root = tmp_path / 'search'
    (root / 'images').mkdir(parents=True)
    (root / 'masks').mkdir()
    for stem in STEMS:                                     # 192 x 160 files: two 96 x 80 images at the default factor
        coarse = rs.randint(0, 256, (12, 10, 3)).astype(np.uint8)
        img = np.kron(coarse, np.ones((16, 16, 1), dtype=np.uint8)) + rs.randint(0, 8, (192, 160, 3)).astype(np.uint8) // 2
        mask = np.kron((rs.rand(12, 10) < 0.5).astype(np.uint8), np.ones((16, 16), dtype=np.uint8))
        mask[rs.rand(192, 160) < 0.05] ^= 1
        Image.fromarray(img.astype(np.uint8)).save(root / 'images' / f'{stem}.png')
        Image.fromarray(mask).save(root / 'masks' / f'{stem}.png')
    masks = [P.read_image(root / 'masks' / f'{stem}.png', mode=Image.NEAREST) for stem in STEMS]
    assert masks[0].shape == (96, 80)
    recorded = []
    inner = P._slic_resident

    def recording(x, n_segments, compactness):
        labels, n_labels = inner(x, n_segments, compactness)
        recorded.append((n_segments, compactness, labels.cpu().numpy()))
        return labels, n_labels
    monkeypatch.setattr(P, '_slic_resident', recording)
    lines = []
    areas, comps = (50, 90), (10, 40)
    got = P.slic_search(root, areas=areas, compactnesses=comps, device=DEV, log=lines.append)
    assert [(r[0], r[1]) for r in recorded] == [(int(96 * 80 / a), c) for a in areas for c in comps]
    assert all(r[2].shape == (2, 96, 80) for r in recorded)                               # equal sizes: one batch per pair
    want = {}
    for (a, c), (_, _, labels) in zip([(a, c) for a in areas for c in comps], recorded):
        want[(a, c)] = np.mean([P.oracle_accuracy(labels[i], masks[i]) for i in range(2)])
    assert got == want and all(isinstance(v, np.float64) for v in got.values())
    assert lines == ['Reading images and masks ...'] + [P.format_search_line(a, c, want[(a, c)]) for (a, c) in want]
    assert 0.5 <= min(want.values()) <= max(want.values()) <= 1.0          # a binary majority vote is right on half its pixels at least
