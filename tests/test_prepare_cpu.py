"""Host side of weak-label preparation (wesup_amd/prepare.py, the mirror of the reference's scripts/generate_points.py,
generate_spl_masks.py and search_slic_params.py): the host paths against the reference's own outputs (tests/golden/prepare.npz,
written by tools/make_prepare_golden.py), the files they write read back by the datasets, and the argument checks of the library
entries of csrc/prepare.hip, which answer on the host before any launch.  No GPU here."""
import ctypes
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'prepare.npz')
STEMS = ('a', 'b')


@pytest.fixture(scope='module')
def lib():
    from wesup_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLDEN)


def _half_even(num, den):
    q, r = divmod(int(num), int(den))
    return q + 1 if 2 * r > den else q + (q & 1) if 2 * r == den else q


# ------------------------------------------------------------------------------------------------ the fixture's own cases
def test_golden_holds_the_cases_it_is_there_for(gold):
    from scipy import ndimage
    # a region whose six centre tries all miss: the whole +-5 box around the rounded centroid lies outside the ring
    mask = gold['points_ring_mask']
    regions, n = ndimage.label(mask == 1, structure=np.ones((3, 3), dtype=np.int32))
    ring = regions == 1
    ys, xs = np.where(ring)
    cy, cx = int(ys.mean().round()), int(xs.mean().round())
    assert n == 2 and not ring[cy - 5:cy + 6, cx - 5:cx + 6].any() and cy >= 5 and cx >= 5
    assert int(ring.sum() * float(gold['points_ring_ratio'])) == 0                      # one point asked for: the centre path
    # a wrapped negative candidate, returned as drawn
    pts, wrap = gold['points_wrap'], gold['points_wrap_mask']
    neg = pts[(pts[:, :2] < 0).any(axis=1)]
    assert len(neg) >= 1 and all(wrap[r, c] == cls for r, c, cls in neg)
    # several points per region, regions on the border, a few hundred of them
    many = gold['points_many_mask']
    n_regions = sum(ndimage.label(many == c, structure=np.ones((3, 3), dtype=np.int32))[1] for c in (1, 2))
    assert n_regions >= 100 and many[0].any() and many[:, 0].any()
    # every recorded label map of the search: an exact tie with an even and with an odd quotient, and an absent id
    for stem in STEMS:
        m = gold[f'search_{stem}_mask_half']
        for area in gold['search_areas']:
            for comp in gold['search_compactnesses']:
                seg = gold[f'search_{stem}_segments_{area}_{comp}']
                count = np.bincount(seg.ravel())
                total = np.bincount(seg.ravel(), weights=m.ravel()).astype(np.int64)
                ties = [(int(s) // int(c)) & 1 for s, c in zip(total, count) if c and 2 * (s % c) == c]
                assert 0 in ties and 1 in ties and (count == 0).any(), (stem, area, comp)


# ------------------------------------------------------------------------------------------------ points
@pytest.mark.parametrize('name', ['ring', 'wrap', 'many'])
def test_generate_points_equals_the_reference(gold, name):
    from wesup_amd import prepare as P
    rs = np.random.RandomState(int(gold[f'points_{name}_seed']))
    got = P.generate_points(gold[f'points_{name}_mask'], float(gold[f'points_{name}_ratio']), rs)
    assert got.dtype == np.int64 and got.ndim == 2 and got.shape[1] == 3
    assert np.array_equal(got, gold[f'points_{name}'])


def test_generate_points_refuses_what_is_no_class_mask():
    from wesup_amd import prepare as P
    with pytest.raises(ValueError):
        P.generate_points(np.zeros((4, 4, 3), dtype=np.uint8))
    with pytest.raises(ValueError):
        P.generate_points(np.zeros((4, 4), dtype=np.float32))
    # background only, ratio too small for a point: the permutation is drawn all the same, nothing comes back
    rs, rs2 = np.random.RandomState(5), np.random.RandomState(5)
    got = P.generate_points(np.zeros((6, 7), dtype=np.uint8), 1e-4, rs)
    assert got.shape == (0, 3) and got.dtype == np.int64
    rs2.permutation(42)
    assert rs.randint(1 << 30) == rs2.randint(1 << 30)


def _write_root(gold, root):
    from PIL import Image
    (root / 'images').mkdir(parents=True)
    (root / 'masks').mkdir()
    for stem in STEMS:
        Image.fromarray(gold[f'root_{stem}_image']).save(root / 'images' / f'{stem}.png')
        Image.fromarray(gold[f'root_{stem}_mask']).save(root / 'masks' / f'{stem}.png')


def test_points_and_spl_masks_folders_equal_the_reference_and_feed_the_datasets(gold, tmp_path):
    import torch
    from wesup_amd import prepare as P
    from wesup_amd.utils.data import PointSupervisionDataset, WESUPV2Dataset
    root = tmp_path / 'data'
    _write_root(gold, root)
    lines = []
    ratio = float(gold['root_ratio'])
    folder = P.generate_points_dir(root, ratio, seed=int(gold['root_seed']), log=lines.append)
    assert folder.name == str(gold['root_points_dir']) and lines[0] == 'Generating point annotation ...'
    for stem in STEMS:
        assert (folder / f'{stem}.csv').read_bytes() == gold[f'root_{stem}_csv'].tobytes(), stem
    n_points = [len(gold[f'root_{stem}_csv'].tobytes().split()) for stem in STEMS]
    assert lines[1] == f'Average number of points: {np.mean(n_points)}.'

    segments = {gold[f'root_{stem}_image'].shape[:2]: gold[f'root_{stem}_segments'] for stem in STEMS}
    calls = []

    def segment_fn(img, n_segments, compactness):
        assert img.dtype == np.uint8 and img.ndim == 3
        calls.append((n_segments, compactness))
        return segments[img.shape[:2]]
    written = P.generate_spl_masks(root, n_classes=3, segment_fn=segment_fn, log=lines.append)
    assert [w.name for w in written] == [folder.name.replace('points', 'spl-masks')]
    assert calls == [(40 * 52 // 200, 40), (45 * 37 // 200, 40)]
    for stem in STEMS:
        spl = np.load(written[0] / f'{stem}.npy')
        assert spl.dtype == np.uint8 and np.array_equal(spl, gold[f'root_{stem}_spl']), stem
    assert gold['root_b_spl'][..., 2].any()                                             # the third class is really painted

    # the datasets read `points` and `spl-masks`: written under those names they come back as items
    P.generate_points_dir(root, ratio, seed=int(gold['root_seed']), name='points', log=lines.append)
    os.rename(written[0], root / 'spl-masks')
    item = PointSupervisionDataset(root)[0]
    rows = np.array([[int(v) for v in line.split(',')] for line in gold['root_a_csv'].tobytes().decode().split()])
    assert np.array_equal(item[2][:len(rows)].numpy(), rows) and int(item[2][len(rows)][0]) == -1
    img, mask, coords = WESUPV2Dataset(root)[1]
    assert mask.dtype == torch.long and np.array_equal(mask.numpy(), gold['root_b_spl'].transpose(2, 0, 1))
    assert tuple(coords.shape) == (2, 45, 37)


def test_spl_mask_index_rules():
    from wesup_amd import prepare as P
    seg = (np.arange(6)[:, None] // 3) * 2 + np.arange(8)[None] // 4                     # four superpixels
    got = P.spl_mask(seg, [[0, 0, 1], [-1, -1, 0], [5, 7, -1]], n_classes=2)
    want = np.zeros((6, 8, 2), dtype=np.uint8)
    want[:3, :4, 1] = 1
    want[3:, 4:, :] = 1
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert not P.spl_mask(seg, np.zeros((0, 3), dtype=np.int64), 3).any()
    for bad in ([6, 0, 0], [0, 8, 0], [-7, 0, 0], [0, -9, 0], [0, 0, 2], [0, 0, -3]):
        with pytest.raises(IndexError):
            P.spl_mask(seg, [bad], n_classes=2)


# ------------------------------------------------------------------------------------------------ SLIC search
def test_read_image_and_listing_equal_the_reference(gold, tmp_path):
    from PIL import Image
    from wesup_amd import prepare as P
    for stem in STEMS:
        Image.fromarray(gold[f'search_{stem}_image']).save(tmp_path / f'{stem}.png')
        Image.fromarray(gold[f'search_{stem}_mask']).save(tmp_path / f'{stem}-mask.png')
        img = P.read_image(tmp_path / f'{stem}.png')
        mask = P.read_image(tmp_path / f'{stem}-mask.png', mode=Image.NEAREST)
        H, W = gold[f'search_{stem}_image'].shape[:2]
        assert img.shape == (int(H * 0.5), int(W * 0.5), 3) and H % 2 + W % 2 > 0         # odd sizes: int(), not round
        assert np.array_equal(img, gold[f'search_{stem}_image_half'])
        assert np.array_equal(mask, gold[f'search_{stem}_mask_half'])
        assert P.read_image(tmp_path / f'{stem}.png', rescale_factor=1.0).shape == (H, W, 3)
    listing = tmp_path / 'listing'
    listing.mkdir()
    for name in gold['listing_files']:
        (listing / str(name)).touch()
    assert [os.path.basename(p) for p in P.list_images(listing)] == [str(n) for n in gold['listing']]


def test_oracle_accuracy_equals_the_reference(gold):
    from wesup_amd import prepare as P
    for i, stem in enumerate(STEMS):
        mask = gold[f'search_{stem}_mask_half']
        for j, area in enumerate(gold['search_areas']):
            for k, comp in enumerate(gold['search_compactnesses']):
                acc = P.oracle_accuracy(gold[f'search_{stem}_segments_{area}_{comp}'], mask)
                assert isinstance(acc, np.float64) and acc == gold['search_accs'][i, j, k], (stem, area, comp)
    with pytest.raises(ValueError, match='2-D'):
        P.oracle_accuracy(np.zeros((4, 4), dtype=np.int32), np.zeros((4, 4, 3), dtype=np.uint8))


def test_slic_search_prints_the_references_lines(gold, tmp_path):
    from PIL import Image
    from wesup_amd import prepare as P
    root = tmp_path / 'search'
    (root / 'images').mkdir(parents=True)
    (root / 'masks').mkdir()
    for stem in STEMS:
        Image.fromarray(gold[f'search_{stem}_image']).save(root / 'images' / f'{stem}.png')
        Image.fromarray(gold[f'search_{stem}_mask']).save(root / 'masks' / f'{stem}.png')
    shapes = {gold[f'search_{stem}_image_half'].shape[:2]: stem for stem in STEMS}

    def segment_fn(img, n_segments, compactness):
        H, W = img.shape[:2]
        area = [a for a in gold['search_areas'] if int(H * W / a) == n_segments][0]
        return gold[f'search_{shapes[(H, W)]}_segments_{area}_{compactness}']
    lines = []
    areas, comps = [int(v) for v in gold['search_areas']], [int(v) for v in gold['search_compactnesses']]
    got = P.slic_search(root, areas=areas, compactnesses=comps, segment_fn=segment_fn, log=lines.append)
    assert lines == [str(s) for s in gold['search_lines']]
    assert list(got) == [(a, c) for a in areas for c in comps]
    for j, a in enumerate(areas):
        for k, c in enumerate(comps):
            assert got[(a, c)] == np.mean(gold['search_accs'][:, j, k])
    # a mask with channels is refused by name
    Image.fromarray(gold['search_a_image']).save(root / 'masks' / 'a.png')
    with pytest.raises(ValueError, match='a.png'):
        P.slic_search(root, areas=areas, compactnesses=comps, segment_fn=segment_fn, log=lines.append)


def test_rounding_rule_equals_numpys():
    """The integer rule of wesup_sp_vote and of the device centroids against ``mean().round()`` on (sum, count) pairs that a
    uint8 map can produce, ties included."""
    from wesup_amd import prepare as P
    rs = np.random.RandomState(0)
    cnt = rs.randint(1, 5000, 20000).astype(np.int64)
    total = np.minimum(rs.randint(0, 1 << 20, 20000), 255 * cnt).astype(np.int64)
    total[::7] = (2 * rs.randint(0, 255, len(total[::7])) + 1) * cnt[::7] // 2          # many exact halves where cnt is even
    want = (total.astype(np.float64) / cnt).round().astype(np.int64)
    assert np.array_equal(P._round_half_even_div(total, cnt), want)
    assert [_half_even(1, 2), _half_even(3, 2), _half_even(5, 2), _half_even(7, 3)] == [0, 2, 2, 2]


# ------------------------------------------------------------------------------------------------ area.csv
def test_generate_area_feeds_the_area_dataset(gold, tmp_path):
    from wesup_amd import prepare as P
    from wesup_amd.utils.data import AreaConstraintDataset
    root = tmp_path / 'data'
    _write_root(gold, root)
    path = P.generate_area(root, log=lambda *a: None)
    assert path == root / 'area.csv'
    text = path.read_text().split()
    assert text[0] == ',img,area' and [t.split(',')[:2] for t in text[1:]] == [['0', 'a.png'], ['1', 'b.png']]
    ds = AreaConstraintDataset(root)
    want = [float(gold[f'root_{stem}_mask'].mean()) for stem in STEMS]
    assert ds.area_info.tolist() == want
    assert ds[1][3].tolist() == [float(np.float32(want[1]))] * 2


# ------------------------------------------------------------------------------------------------ command line
def test_command_line():
    from wesup_amd import prepare as P
    a = P.parse_args(['points', '~/data/glas/train', '-p', '1e-5', '--seed', '3'])
    assert (a.command, a.root_dir, a.point_ratio, a.seed, a.host) == ('points', '~/data/glas/train', 1e-5, 3, False)
    assert P.parse_args(['points', 'd']).point_ratio == 1e-4 and P.parse_args(['points', 'd', '--host']).host
    a = P.parse_args(['spl-masks', 'd', '--n-classes', '3', '--sp-area', '150', '--compactness', '30'])
    assert (a.data_root, a.n_classes, a.sp_area, a.compactness) == ('d', 3, 150, 30)
    a = P.parse_args(['spl-masks', 'd'])
    assert (a.n_classes, a.sp_area, a.compactness) == (2, 200, 40)
    a = P.parse_args(['slic-search', 'd', '-r', '0.25', '-a', '50,100', '-c', '10'])
    assert (a.dataset_path, a.rescale_factor, a.area, a.compactness) == ('d', 0.25, '50,100', '10')
    a = P.parse_args(['slic-search', 'd'])
    assert (a.rescale_factor, a.area, a.compactness) == (0.5, '50,60,70,80,90,100', '10,20,30,40,50')
    assert P.parse_args(['area', 'd']).root_dir == 'd'
    for bad in ([], ['points'], ['nothing', 'd']):
        with pytest.raises(SystemExit):
            P.parse_args(bad)


# ------------------------------------------------------------------------------------------------ the library entries
def test_new_entries_are_exported_and_the_abi_stays(lib):
    h = lib.load()
    for name in ('wesup_label_stats', 'wesup_sp_vote', 'wesup_spl_paint', 'wesup_sp_vote_workspace_bytes',
                 'wesup_spl_paint_workspace_bytes', 'wesup_prepare_lds_entries'):
        assert name in lib.EXPORTS and hasattr(h, name)
    assert h.wesup_abi_version() == lib.ABI_VERSION == 6                                # additions only
    assert h.wesup_prepare_lds_entries(0) > 0 and h.wesup_prepare_lds_entries(1) > 0 and h.wesup_prepare_lds_entries(2) == 0
    assert h.wesup_sp_vote_workspace_bytes(3, 96, 80, 100) >= 3 * 100 * 8
    assert h.wesup_spl_paint_workspace_bytes(100, 3) >= 300


def test_new_entries_reject_bad_arguments_on_the_host(lib):
    """Null pointers, non-positive sizes, L < 0, K / C <= 0 and shapes whose sums the counters cannot hold: WESUP_ERR_INVALID
    without a launch.  The pointers are 16-byte aligned host addresses that are never dereferenced: every call below fails its
    check first."""
    h = lib.load()
    buf = ctypes.create_string_buffer(256)
    ok = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    INVALID = -1
    big = 1 << 22
    # (a) wesup_label_stats(labels, stats, status, B, H, W, L, stream)
    for ptrs in ((None, ok, ok), (ok, None, ok), (ok, ok, None)):
        assert h.wesup_label_stats(*ptrs, 1, 8, 8, 4, None) == INVALID
    for sizes in ((0, 8, 8, 4), (1, 0, 8, 4), (1, 8, 0, 4), (1, 8, -8, 4), (1, 8, 8, -1), (1, 8, 8, 1 << 26), (70000, 8, 8, 4),
                  (1, big + 1, 8, 4), (1, 8, big + 1, 4), (2, big, big, 4)):
        assert h.wesup_label_stats(ok, ok, ok, *sizes, None) == INVALID, sizes
    # (b) wesup_sp_vote(labels, values, painted, agree, status, B, H, W, K, ws, ws_bytes, stream); painted may be NULL
    for ptrs in ((None, ok, ok, ok, ok), (ok, None, ok, ok, ok), (ok, ok, ok, None, ok), (ok, ok, ok, ok, None)):
        assert h.wesup_sp_vote(*ptrs, 1, 8, 8, 4, ok, 256, None) == INVALID
    assert h.wesup_sp_vote(ok, ok, None, ok, ok, 1, 8, 8, 4, None, 256, None) == INVALID
    for sizes in ((0, 8, 8, 4), (1, 0, 8, 4), (1, 8, 0, 4), (1, 8, 8, 0), (1, 8, 8, -3), (1, 8, 8, (1 << 26) + 1),
                  (1, 4105, 4105, 4), (1, big, 8, 4)):                                  # 255 * 4105^2 >= 2^32
        assert h.wesup_sp_vote(ok, ok, None, ok, ok, *sizes, ok, 1 << 40, None) == INVALID, sizes
        assert h.wesup_sp_vote_workspace_bytes(*sizes) == 0
    assert h.wesup_sp_vote_workspace_bytes(1, 4104, 4104, 4) > 0                       # 255 * 4104^2 < 2^32
    assert h.wesup_sp_vote(ok, ok, None, ok, ok, 1, 8, 8, 4, ok, 8, None) == -3        # a workspace too small: its own code
    # (c) wesup_spl_paint(labels, points, out, status, H, W, K, C, P, ws, ws_bytes, stream); points may be NULL only for P = 0
    for ptrs in ((None, ok, ok, ok), (ok, None, ok, ok), (ok, ok, None, ok), (ok, ok, ok, None)):
        assert h.wesup_spl_paint(*ptrs, 8, 8, 4, 2, 1, ok, 256, None) == INVALID
    assert h.wesup_spl_paint(ok, ok, ok, ok, 8, 8, 4, 2, 1, None, 256, None) == INVALID
    for sizes in ((0, 8, 4, 2, 1), (8, 0, 4, 2, 1), (8, 8, 0, 2, 1), (8, 8, 4, 0, 1), (8, 8, 4, -2, 1), (8, 8, 4, 2, -1),
                  (8, 8, 4, 257, 1), (8, 8, 1 << 25, 4, 1), (big + 1, 8, 4, 2, 1)):
        assert h.wesup_spl_paint(ok, ok, ok, ok, *sizes, ok, 1 << 40, None) == INVALID, sizes
    assert h.wesup_spl_paint_workspace_bytes(0, 2) == 0 and h.wesup_spl_paint_workspace_bytes(4, 0) == 0
    assert h.wesup_abi_version() == 6


def test_wrappers_fail_loudly_without_gpu_tensors(lib):
    import torch
    from wesup_amd import ops
    lab = torch.zeros(8, 8, dtype=torch.int32)
    with pytest.raises(lib.WesupHipError):
        ops.label_stats(lab, 3)
    with pytest.raises(lib.WesupHipError):
        ops.sp_vote(lab, torch.zeros(8, 8, dtype=torch.uint8), 4)
    with pytest.raises(lib.WesupHipError):
        ops.spl_paint(lab, torch.zeros(1, 3, dtype=torch.int32), 4)
    with pytest.raises(lib.WesupHipError):
        ops.label_stats(np.zeros((8, 8), dtype=np.int32), 3)                           # not a tensor at all
