"""Tissue selection on the device (csrc/tissue.hip, the ``*_list`` entries of slide.hip and classmap.hip) against
the host definitions of wesup_amd/slide.py and against the entries the project already had.  Everything here is integers or a
comparison of two runs of the same kernels, so every comparison is exact: there is no tolerance in this file.

Histograms equal ``numpy.bincount`` per patch; total, threshold, counts, list and info equal ``otsu_threshold`` /
``tissue_counts`` / ``select_patches``; the mask equals ``tissue_mask_array``.  A listed patch gets from the list entries the
bits the plain entries give it.  The pipelines with a selection equal the pipelines without one on the kept patches and are 0 on
the others."""
import functools
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = 77
WEIGHT_SEED, FEAT_SCALE, IMAGE_SEED = 3, 1.0, 5
SHIFT = -0.36169204115867615      # tests/test_tiles_gpu.py: centres z1 - z0 of these weights on synth images
CHANNELS = ('luma', 'chroma')


def _u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


# -------------------------------------------------------------------------------------------------------- 1. histograms
def _noise(seed, H, W):
    return np.random.RandomState(seed).randint(0, 256, (H, W, 3)).astype(np.uint8)


def _all_values(H=16, W=16):
    """Every one of the 256 values in each channel, and with them many lumas and chromas."""
    idx = np.arange(H * W).reshape(H, W) % 256
    return np.stack([idx, (idx * 7 + 3) % 256, 255 - idx], axis=2).astype(np.uint8)


def _glass(H, W, every=None):
    """All 255: every lane of a wave on one bin.  ``every``: one pixel per ``every`` changed, so that a wave that takes the
    one-lane path for the rest still has to count the odd pixel for itself."""
    img = np.full((H, W, 3), 255, np.uint8)
    if every:
        flat = img.reshape(-1, 3)
        flat[5::every] = (12, 200, 90)
    return img


# (name, image, p).  An item of the histogram kernel is max(1, 8192 // p) rows of one patch and the grid is at most 2048 blocks
# (_lib.TISSUE_ITEM_PIXELS, _lib.TISSUE_MAX_BLOCKS): 100 x 100 at p = 2 is 2500 patches of one item each, so blocks 0 .. 451 take
# a second item -- the grid-stride loop wraps.  At p = 16 an item is a whole patch, at p = 128 it is 64 rows (two per patch).
HIST_CASES = [
    ('ragged 3 x 4, W * 3 odd', lambda: _noise(1, 37, 53), 16),
    ('p > H', lambda: _noise(2, 20, 300), 128),
    ('1225 patches', lambda: _noise(3, 70, 70), 2),
    ('all 256 values', _all_values, 5),
    ('all 255', lambda: _glass(64, 130), 64),
    ('all 255 but one pixel per 64', lambda: _glass(64, 130, every=64), 64),
    ('the grid wraps', lambda: _noise(4, 100, 100), 2),
    ('rows of 1000 pixels, two items per row strip', lambda: _noise(5, 12, 2003), 1000),
]


@pytest.mark.parametrize('channel', CHANNELS)
@pytest.mark.parametrize('name,make,p', HIST_CASES, ids=[c[0] for c in HIST_CASES])
def test_histograms_equal_bincount_per_patch(name, make, p, channel):
    from wesup_amd import _lib, ops, slide as S
    img = make()
    H, W = img.shape[:2]
    want = S.patch_histograms(img, p, channel)
    assert np.array_equal(want.sum(axis=1), S.patch_areas(H, W, p))
    if name == 'the grid wraps':
        assert want.shape[0] * -(-p // max(1, _lib.TISSUE_ITEM_PIXELS // p)) > _lib.TISSUE_MAX_BLOCKS == 2048
    got = _u32(ops.patch_value_hist(torch.from_numpy(img).to(DEV), p, channel))
    assert got.shape == want.shape
    assert np.array_equal(got, want), (name, channel, int((got != want).sum()))


@pytest.mark.parametrize('channel', CHANNELS)
def test_histograms_of_an_image_at_an_odd_address(channel):
    """A slide that does not start at a multiple of four bytes takes the byte-wise reads."""
    from wesup_amd import ops, slide as S
    img = _noise(6, 37, 53)
    buf = torch.zeros(1 + img.size, dtype=torch.uint8, device=DEV)
    view = buf[1:].view(37, 53, 3)
    view.copy_(torch.from_numpy(img))
    assert view.data_ptr() % 4 == 1 and view.is_contiguous()
    assert np.array_equal(_u32(ops.patch_value_hist(view, 16, channel)), S.patch_histograms(img, 16, channel))


# --------------------------------------------------------------------------------------------------------- 2. selection
def _mottled(seed, H, W, p, share):
    """Glass (250 .. 255, grey) with whole patches of dark, coloured tissue chosen at random: the kept set is as irregular as
    the compaction can meet."""
    rs = np.random.RandomState(seed)
    img = rs.randint(250, 256, (H, W, 1)).repeat(3, axis=2).astype(np.uint8)
    n_h, n_w = -(-H // p), -(-W // p)
    for k in np.nonzero(rs.rand(n_h * n_w) < share)[0]:
        y, x = k // n_w * p, k % n_w * p
        h, w = min(p, H - y), min(p, W - x)
        img[y:y + p, x:x + p] = np.stack([rs.randint(90, 200, (h, w)), rs.randint(10, 80, (h, w)), rs.randint(100, 220, (h, w))], axis=2)
    return img


def _host_selection(img, p, channel, threshold, min_ppm):
    from wesup_amd import slide as S
    hist = S.patch_histograms(img, p, channel)
    total = hist.sum(axis=0)
    t = S.otsu_threshold(total) if threshold < 0 else threshold
    counts = S.tissue_counts(hist, t, channel)
    kept = S.select_patches(counts, S.patch_areas(img.shape[0], img.shape[1], p), min_ppm, flat=t < 0)
    return total, t, counts, kept


def _check_selection(img, p, channel, threshold, min_ppm):
    from wesup_amd import ops
    H, W = img.shape[:2]
    total, t, counts, kept = _host_selection(img, p, channel, threshold, min_ppm)
    img_d = torch.from_numpy(img).to(DEV)
    info, total_d, counts_d, list_d = ops.tissue_select(ops.patch_value_hist(img_d, p, channel), H, W, p, channel, threshold, min_ppm)
    n = len(counts)
    assert np.array_equal(total_d.cpu().numpy(), total)
    assert info.cpu().tolist() == [t, len(kept), n, int(t < 0), 0, 0, 0, 0]
    assert np.array_equal(_u32(counts_d), counts)
    assert list_d.shape == (n,) and list_d[:len(kept)].cpu().tolist() == kept
    return t, kept, n


@pytest.mark.parametrize('channel', CHANNELS)
@pytest.mark.parametrize('given', [False, True], ids=['otsu', 'given'])
def test_selection_across_the_chunk_edges(channel, given):
    """70 x 70 at p = 2: 1225 patches, walked by the compaction 256 at a time (_lib.TISSUE_LIST_CHUNK), so patches 255 | 256,
    511 | 512, 767 | 768 and 1023 | 1024 are the chunk edges the order has to hold across."""
    from wesup_amd import _lib
    assert _lib.TISSUE_LIST_CHUNK == 256
    img = _mottled(7, 70, 70, 2, 0.4)
    threshold = -1 if not given else {'luma': 140, 'chroma': 15}[channel]   # (tissue: luma <= 131, chroma >= 21; glass 250 .., 0)
    t, kept, n = _check_selection(img, 2, channel, threshold, 500000)
    assert n == 1225 and 300 < len(kept) < 700
    for edge in (256, 512, 768, 1024):                                       # kept patches on both sides of every edge
        assert any(edge - 16 <= k < edge for k in kept) and any(edge <= k < edge + 16 for k in kept), edge
    if threshold < 0:
        assert (80 <= t < 250) if channel == 'luma' else (0 <= t < 100)


@pytest.mark.parametrize('channel', CHANNELS)
def test_selection_ragged_lattice_and_the_ppm_rule(channel):
    img = _mottled(8, 37, 53, 16, 0.5)
    img[36, 52] = (150, 30, 160)                                             # one tissue pixel of the corner patch's 25
    for min_ppm in (0, 40000, 40001, 1000000):                               # 1 / 25 is 40000 ppm exactly
        _check_selection(img, 16, channel, -1, min_ppm)


def test_selection_nothing_kept_everything_kept_and_flat():
    bright = np.random.RandomState(9).randint(200, 256, (40, 50, 3)).astype(np.uint8)
    t, kept, n = _check_selection(bright, 16, 'luma', 100, 0)                # no pixel at or below 100
    assert kept == [] and n == 12
    t, kept, n = _check_selection(bright, 16, 'luma', 254, 0)
    assert kept == list(range(12))
    t, kept, n = _check_selection(_noise(10, 40, 50), 16, 'luma', -1, 10000)
    assert kept == list(range(12)) and t >= 0
    for channel in CHANNELS:
        flat = np.full((40, 50, 3), 255, np.uint8)
        t, kept, n = _check_selection(flat, 16, channel, -1, 1000000)        # one level: t = -1, never skipped
        assert t == -1 and kept == list(range(12))
    grey = np.full((40, 50, 3), 31, np.uint8)
    t, kept, n = _check_selection(grey, 16, 'chroma', 0, 0)                  # chroma 0 everywhere, v > 0 nowhere
    assert kept == []


def test_tissue_patches_on_the_device_equals_the_host():
    from wesup_amd import slide as S
    img = _mottled(11, 48, 64, 16, 0.5)
    for kw in ({}, {'channel': 'chroma'}, {'threshold': 200, 'min_fraction': 0.5}):
        host, dev = S.tissue_patches(img, 16, **kw), S.tissue_patches(img, 16, device=DEV, **kw)
        assert (dev.t, dev.n_keep, dev.n, dev.flat) == (host.t, host.n_keep, host.n, host.flat)
        assert dev.list.is_cuda and dev.list.dtype == torch.int32 and dev.list.cpu().tolist() == host.list
        assert np.array_equal(_u32(dev.counts), host.counts)


# -------------------------------------------------------------------------------------------------------------- 3. mask
@pytest.mark.parametrize('channel', CHANNELS)
def test_mask_equals_the_host_mask(channel):
    from wesup_amd import ops, slide as S
    img = _mottled(12, 37, 53, 16, 0.5)
    img[:5] = _noise(13, 5, 53)
    img_d = torch.from_numpy(img).to(DEV)
    for threshold in (-1, 0, 77, 254):
        info = ops.tissue_select(ops.patch_value_hist(img_d, 16, channel), 37, 53, 16, channel, threshold, 10000)[0]
        t = int(info[0].cpu())
        want = S.tissue_mask_array(img, t, channel)
        assert 0 < want.mean() < 255 or threshold in (0, 254)
        assert np.array_equal(ops.tissue_mask(img_d, info, channel).cpu().numpy(), want), (channel, threshold)
    flat = torch.full((9, 7, 3), 200, dtype=torch.uint8, device=DEV)
    info = ops.tissue_select(ops.patch_value_hist(flat, 4, channel), 9, 7, 4, channel, -1, 10000)[0]
    assert int(info[0].cpu()) == -1 and bool((ops.tissue_mask(flat, info, channel) == 255).all())


# ------------------------------------------------------------------------------------------------------ 4. list entries
LATTICE = (150, 131, 64, (48, 40))          # tests/test_slide_gpu.py: 3 x 3, ragged at the far borders
LIST = [7, 2, 8, 0]


def _list(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize('ac', [False, True])
def test_list_gather_equals_the_plain_gather_of_every_listed_patch(ac):
    from wesup_amd import ops
    H, W, p, (h, w) = LATTICE
    img = torch.from_numpy(_noise(14, H, W)).to(DEV)
    single = {k: ops.patch_gather_resize(img, p, h, w, k, 1, align_corners=ac).clone() for k in set(LIST)}
    got = ops.patch_gather_resize(img, p, h, w, 0, 4, align_corners=ac, patch_list=_list(LIST))
    for i, k in enumerate(LIST):
        assert torch.equal(got[i], single[k][0]), (i, k)
    ragged = ops.patch_gather_resize(img, p, h, w, 2, 4, align_corners=ac, patch_list=_list(LIST))      # slots 2, 3, then 3 again
    for i, k in enumerate([8, 0, 0, 0]):
        assert torch.equal(ragged[i], single[k][0]), (i, k)
    out = torch.full((3, 3, h, w), -5.0, device=DEV)                         # a value outside the lattice: the slot is left alone
    ops.patch_gather_resize(img, p, h, w, 0, 3, align_corners=ac, out=out, patch_list=_list([2, 9, -1]))
    assert torch.equal(out[0], single[2][0]) and bool((out[1:] == -5.0).all())


def _pred(seed, count, h, w, classes=0):
    rs = np.random.RandomState(seed)
    if classes:
        a = rs.rand(count, h, w, classes).astype(np.float32)
        return torch.from_numpy(a / a.sum(axis=-1, keepdims=True)).to(DEV)
    a = rs.rand(count, h, w).astype(np.float32)
    a[rs.rand(count, h, w) < 0.1] = 0.5                                      # ties of the rounding
    return torch.from_numpy(a).to(DEV)


@pytest.mark.parametrize('mode', [0, 1])
def test_list_scatter_equals_the_plain_scatter_patch_by_patch(mode):
    from wesup_amd import ops
    H, W, p, (h, w) = LATTICE
    pred = _pred(15 + mode, 4, h, w)
    want = torch.full((H, W), SENTINEL, dtype=torch.uint8, device=DEV)
    for i, k in enumerate(LIST):
        ops.patch_scatter_u8(pred[i:i + 1], want, p, k, mode=mode)
    got = torch.full((H, W), SENTINEL, dtype=torch.uint8, device=DEV)
    ops.patch_scatter_u8(pred, got, p, 0, mode=mode, patch_list=_list(LIST))
    assert torch.equal(got, want)
    untouched = np.ones((H, W), bool)                                        # everything outside the listed patches: the sentinel
    for k in LIST:
        untouched[k // 3 * p:k // 3 * p + p, k % 3 * p:k % 3 * p + p] = False
    assert bool((got.cpu().numpy()[untouched] == SENTINEL).all()) and untouched.any()
    # first = 2 of a list of 4: slots 2 and 3 are pasted, the two behind the list's end are skipped
    want = torch.full((H, W), SENTINEL, dtype=torch.uint8, device=DEV)
    for i, k in enumerate(LIST[2:]):
        ops.patch_scatter_u8(pred[i:i + 1], want, p, k, mode=mode)
    got = torch.full((H, W), SENTINEL, dtype=torch.uint8, device=DEV)
    ops.patch_scatter_u8(pred, got, p, 2, mode=mode, patch_list=_list(LIST))
    assert torch.equal(got, want)
    # values outside the lattice write nothing
    got = torch.full((H, W), SENTINEL, dtype=torch.uint8, device=DEV)
    ops.patch_scatter_u8(pred[:3], got, p, 0, mode=mode, patch_list=_list([9, -1, 1 << 30]))
    assert bool((got == SENTINEL).all())


@pytest.mark.parametrize('mode', [0, 1])
def test_list_scatter_of_classes_equals_the_plain_one(mode):
    from wesup_amd import ops
    H, W, p, (h, w) = LATTICE
    C = 3
    if mode == 0:
        pred = torch.from_numpy(np.random.RandomState(17).randint(0, C, (4, h, w)).astype(np.float32)).to(DEV)
        kw = {'n_classes': C}
    else:
        pred, kw = _pred(18, 4, h, w, classes=C), {}
    want = torch.full((H, W), SENTINEL, dtype=torch.uint8, device=DEV)
    for i, k in enumerate(LIST):
        ops.patch_scatter_classes_u8(pred[i:i + 1], want, p, k, mode=mode, **kw)
    got = torch.full((H, W), SENTINEL, dtype=torch.uint8, device=DEV)
    _, status = ops.patch_scatter_classes_u8(pred, got, p, 0, mode=mode, patch_list=_list(LIST), **kw)
    assert torch.equal(got, want) and int(status.cpu()) == 0
    assert set(np.unique(got.cpu().numpy())) == {0, 1, 2, SENTINEL}
    got = torch.full((H, W), SENTINEL, dtype=torch.uint8, device=DEV)        # outside the lattice: nothing written, status set
    _, status = ops.patch_scatter_classes_u8(pred[:2], got, p, 0, mode=mode, patch_list=_list([9, -3]), **kw)
    assert bool((got == SENTINEL).all()) and int(status.cpu()) != 0
    got = torch.full((H, W), SENTINEL, dtype=torch.uint8, device=DEV)        # behind the list's end: skipped, and no error
    _, status = ops.patch_scatter_classes_u8(pred, got, p, 3, mode=mode, patch_list=_list(LIST), **kw)
    want = torch.full((H, W), SENTINEL, dtype=torch.uint8, device=DEV)
    ops.patch_scatter_classes_u8(pred[:1], want, p, LIST[3], mode=mode, **kw)
    assert torch.equal(got, want) and int(status.cpu()) == 0


# ---------------------------------------------------------------------------------------------------------- 5. pipelines
def _image(seed, H, W):
    from wesup_amd import synth
    return np.ascontiguousarray((synth.synth_image(seed, H, W).transpose(1, 2, 0) * 255).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def _weights():
    from oracle import wesup_oracle as orc
    w = orc.make_weights(WEIGHT_SEED, feat_scale=FEAT_SCALE)
    b = w['classifier.0.bias'].copy()
    b[1] -= np.float32(SHIFT)
    w['classifier.0.bias'] = b
    return w


def _superpixel():
    """(predict(img, batch, **kw) -> map, calls): the superpixel model of tests/test_slide_gpu.py; ``calls`` counts the passes."""
    from wesup_amd import slide as S
    from wesup_amd.models import initialize_trainer
    trainer = initialize_trainer('wesup', device=DEV, sp_area=64)
    trainer.model.load_state_dict({k: torch.from_numpy(v) for k, v in _weights().items()})
    trainer.model.eval()
    calls, inner = [], trainer.preprocess

    def preprocess(x):
        calls.append(x.shape[0])
        return inner(x)
    trainer.preprocess = preprocess
    return (lambda img, batch, **kw: S.slide_predict(trainer, img, 80, (48, 64), batch=batch, device=DEV, **kw)), calls


def _pixel():
    from wesup_amd import slide as S
    from wesup_amd.models.wesup import WESUPPixelInference
    model = WESUPPixelInference().to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in _weights().items()})
    model.eval()
    calls, inner = [], model.forward_per_resolution

    def forward(x):
        calls.append(x.shape[0])
        return inner(x)
    model.forward_per_resolution = forward
    return (lambda img, batch, **kw: S.slide_pixel_predict(model, img, 80, 0.6, batch=batch, device=DEV, **kw)), calls


@pytest.mark.parametrize('make', [_superpixel, _pixel], ids=['superpixel', 'pixel'])
def test_pipeline_with_a_selection_equals_the_pipeline_without(make):
    from wesup_amd import slide as S
    predict, calls = make()
    H, W, p = 150, 131, 80                                                   # the 2 x 2 lattice of tests/test_slide_gpu.py
    img = _image(IMAGE_SEED, H, W)
    # every patch kept (threshold 254, any tissue pixel at all): the same passes, the same bytes
    everything = {'threshold': 254, 'min_fraction': 0.0}
    assert S.tissue_patches(img, p, **everything).list == [0, 1, 2, 3]
    for batch in (1, 3):
        assert np.array_equal(predict(img, batch, skip_background=everything), predict(img, batch)), batch
    # patches 1 and 2 are glass
    img[:80, 80:] = 255
    img[80:, :80] = 255
    sel = S.tissue_patches(img, p)
    assert sel.list == [0, 3] and 0 <= sel.t < 255
    full = predict(img, 1)
    del calls[:]
    got = predict(img, 1, skip_background=True)
    assert calls == [1, 1]                                                   # n_keep passes of one patch
    assert got.shape == (H, W) and got.dtype == np.uint8
    assert np.array_equal(got[:80, :80], full[:80, :80]) and np.array_equal(got[80:, 80:], full[80:, 80:])
    assert not got[:80, 80:].any() and not got[80:, :80].any()
    assert got[:80, :80].any() or got[80:, 80:].any()                        # not vacuous: the kept patches predict something
    del calls[:]
    nothing = predict(np.full((H, W, 3), 255, np.uint8), 1, skip_background={'threshold': 100})
    assert nothing.shape == (H, W) and not nothing.any() and calls == []     # nothing kept: no forward at all


# ------------------------------------------------------------------------------------------------------------- 6. driver
def test_driver_skips_background_and_writes_the_tissue_masks(tmp_path):
    from PIL import Image
    from wesup_amd import slide as S
    root, ckpt = tmp_path / 'val', tmp_path / 'record' / 'checkpoints' / 'ckpt.0001.pth'
    (root / 'images').mkdir(parents=True)
    (root / 'masks').mkdir()
    ckpt.parent.mkdir(parents=True)
    torch.save({'epoch': 0, 'model_state_dict': {k: torch.from_numpy(v) for k, v in _weights().items()}}, ckpt)
    sizes = {'positive-a': (100, 90), 'negative-b': (70, 120)}
    rs = np.random.RandomState(4)
    for seed, (stem, (H, W)) in enumerate(sizes.items()):
        img = _image(20 + seed, H, W)
        img[:, 80:] = 255                                                    # the patches of the second column are glass
        Image.fromarray(img).save(root / 'images' / f'{stem}.jpg', quality=95)
        Image.fromarray((rs.rand(H, W) < 0.5).astype(np.uint8) * 255).save(root / 'masks' / f'{stem}.png')
    for pixel, name in ((False, 'combined-results-for-ckpt.0001.pth'), (True, 'combined-results-pixel-for-ckpt.0001.pth')):
        lines, masks = [], tmp_path / f'tissue-{int(pixel)}'
        got = S.main(root, ckpt, pixel=pixel, patch_size=80, device=DEV, batch=2, skip_background=True, tissue_masks=masks,
                     log=lambda *a: lines.append(' '.join(str(v) for v in a)))
        out = tmp_path / 'record' / name
        assert sorted(q.name for q in out.iterdir()) == sorted(q.name for q in masks.iterdir()) == ['negative-b.png', 'positive-a.png']
        text = '\n'.join(lines)
        for stem, shape in sizes.items():
            written = np.asarray(Image.open(out / f'{stem}.png'))
            assert written.shape == shape and written.dtype == np.uint8 and set(np.unique(written)) <= {0, 255}
            assert not written[:, 80:].any()                                 # skipped: background
            decoded = np.asarray(Image.open(root / 'images' / f'{stem}.jpg').convert('RGB'))
            host = S.tissue_patches(decoded, 80)
            n = host.n
            assert f'{stem}: tissue threshold {host.t} (luma), {host.n_keep} of {n} patches kept' in text
            assert host.n_keep == n // 2
            mask = np.asarray(Image.open(masks / f'{stem}.png'))
            assert np.array_equal(mask, S.tissue_mask_array(decoded, host.t))
            gt = np.asarray(Image.open(root / 'masks' / f'{stem}.png'))
            group, negative = ('negative', True) if stem.startswith('negative-') else ('positive', False)
            assert got[group] == S.slide_scores(written, gt, negative=negative)
        assert text.count('Accuracy: ') == 2 and text.count('Dice: ') == 2
        assert len(re.findall(r'patches kept', text)) == 2
