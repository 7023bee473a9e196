"""Whole-slide evaluation on the device (wesup_amd/slide.py, csrc/slide.hip) against what the project already had.

Kernels.  ``patch_gather_resize`` against ``F.interpolate`` on the CPU of the zero-padded patch (pad first, then resize: the
neighbour clamp is at the patch border and texels beyond the slide are 0) at GATHER_BAR = 1e-6 absolute on data in [0, 1] -- the
pixel-resize bar of tests/test_pixel_resolution_gpu.py: fewer than eight fp32 roundings of values <= 1 give < 5e-7, doubled;
bit for bit where a resize is none (same size) and, with align_corners, against ``ops.image_resize_u8`` of a patch that lies
inside the slide.  ``patch_scatter_u8`` mode 0 bit for bit against round -> nearest ``F.interpolate`` -> paste -> crop on the
host, mode 1 against the bilinear ``F.interpolate`` outside pixels whose interpolated value is within 1e-6 of 0.5 (the same
bar; at most 1 % of the map).  ``mask_scores``: the four integer counts equal numpy's.

Pipelines.  ``slide_predict`` / ``slide_pixel_predict`` at batch 1 equal the per-patch paths (``infer.predict_single_image`` on
the gathered tensor; ``pixel_infer.pixel_predict`` of the zero-padded patch) bit for bit; at another batch size the
convolutions tile differently and a probability moves by ~2e-6 (tests/test_tiles_gpu.py), so the maps are compared outside
AMBIGUOUS pixels -- single-patch probability within 1e-5 of 0.5, the bar of test_tiles_gpu.py -- which may be at most 1 % of
the slide.  Weights and the bias shift: those of tests/test_tiles_gpu.py (the shift centres the superpixel logits; the test
asserts that both classes cover at least 10 % of the witness map)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tol                # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dp2019.npz')
GATHER_BAR = 1e-6          # absolute, data in [0, 1]
ROUND_GUARD = 1e-6         # mode 1: |v - 0.5| below this may round either way
AMBIGUOUS = 1e-5           # |p - 0.5| below this: the rounded value may differ between two batch sizes
MAX_AMBIGUOUS_SHARE = 0.01
WEIGHT_SEED, FEAT_SCALE, IMAGE_SEED = 3, 1.0, 5
SHIFT = -0.36169204115867615      # tests/test_tiles_gpu.py: centres z1 - z0 of these weights on synth images
SENTINEL = 77

# (H, W, p, (h, w)): the issue's lattices -- 3 x 3 with 22 valid lines / 3 valid columns at the far border; an upscale; a resize
# that is none; one patch padded on both sides; no padding at all -- and one where every kernel's grid-stride loop wraps (more
# than 4096 blocks of 256: 4 x 1040 x 1040 outputs of the gather, 4 x 520 x 520 lattice pixels of the scatter).  That one doubles
# the patch: at align_corners = 0 the source coordinate 0.5 * (dst + 0.5) - 0.5 is then exact in fp32.  At a ratio that is not,
# one ulp of a coordinate near 519 is 6e-5, and whether the reference fuses the multiply with the subtraction would decide a
# comparison at 1e-6 (the bar was worked out for coordinates below 64).
LATTICES = [(150, 131, 64, (48, 40)), (150, 131, 16, (24, 20)), (150, 131, 64, (64, 64)), (50, 70, 64, (48, 40)),
            (128, 64, 64, (48, 40)), (700, 900, 520, (1040, 1040))]


@functools.lru_cache(maxsize=None)
def _all_bytes_image(H, W):
    rs = np.random.RandomState(H * 1000 + W)
    img = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    img.reshape(-1)[rs.permutation(img.size)[:256]] = np.arange(256, dtype=np.uint8)
    assert len(np.unique(img)) == 256
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _padded_unit_patches(H, W, p):
    """(N, 3, p, p) fp32 on the CPU: the zero-padded patches of the slide, ``/ 255.f`` (never written to)."""
    from wesup_amd import slide as S
    patches = S.split_patches_array(_all_bytes_image(H, W), p)
    return torch.from_numpy(patches.astype(np.float32) / np.float32(255)).permute(0, 3, 1, 2).contiguous()


def _corner(k, n_w, p):
    return k // n_w * p, k % n_w * p


# ------------------------------------------------------------------------------------------------------------ 1. gather
@pytest.mark.parametrize('ac', [0, 1])
@pytest.mark.parametrize('H,W,p,size', LATTICES)
def test_gather_resize_against_interpolate_of_the_padded_patch(H, W, p, size, ac):
    from wesup_amd import ops
    from wesup_amd import slide as S
    n_h, n_w = S.patch_grid(H, W, p)
    N = n_h * n_w
    unit = _padded_unit_patches(H, W, p)
    want = F.interpolate(unit, size=size, mode='bilinear', align_corners=bool(ac))
    img_d = torch.from_numpy(_all_bytes_image(H, W)).to(DEV)
    got = ops.patch_gather_resize(img_d, p, size[0], size[1], 0, N, align_corners=bool(ac))
    assert got.shape == (N, 3, *size) and got.dtype == torch.float32
    err = float((got.cpu() - want).abs().max())
    print(f'gather {H}x{W} p{p} -> {size} align_corners={ac}: max abs err {err:.3e}')
    assert _tol.within(f'slide gather {H}x{W} p{p}->{size} ac{ac}', 'slide_gather_resize', err, GATHER_BAR, 'abs, data in [0,1]')
    if size == (p, p):                                     # a resize that is none: the padded patch / 255.f bit for bit
        assert torch.equal(got.cpu(), unit)
    if ac:                                                 # a patch inside the slide: the whole-image resize of it, bit for bit
        inside = [k for k in range(N) if _corner(k, n_w, p)[0] + p <= H and _corner(k, n_w, p)[1] + p <= W]
        assert inside or (H < p or W < p)
        for k in inside[:4]:
            y, x = _corner(k, n_w, p)
            patch = img_d[y:y + p, x:x + p].contiguous()
            assert torch.equal(got[k], ops.image_resize_u8(patch, *size)[0]), k
    # a pass somewhere inside the lattice, into a buffer that is reused
    buf = torch.full((2, 3, *size), float('nan'), device=DEV)
    first = max(N - 2, 0)
    assert ops.patch_gather_resize(img_d, p, size[0], size[1], first, 2, align_corners=bool(ac), out=buf) is buf
    for i in range(2):
        assert torch.equal(buf[i], got[min(first + i, N - 1)]), i


def test_gather_ragged_pass_repeats_the_last_patch():
    from wesup_amd import ops
    H, W, p, size = 150, 131, 64, (48, 40)
    img_d = torch.from_numpy(_all_bytes_image(H, W)).to(DEV)
    for ac in (False, True):
        full = ops.patch_gather_resize(img_d, p, *size, 0, 9, align_corners=ac)
        tail = ops.patch_gather_resize(img_d, p, *size, 8, 4, align_corners=ac)
        assert tail.shape == (4, 3, *size)
        for i in range(4):
            assert torch.equal(tail[i], full[8]), (ac, i)


def test_gather_border_patch_is_padded_not_clamped():
    """The trap: along the last valid row / column of a border patch the neighbour beyond the slide is 0, not the edge texel."""
    from wesup_amd import ops
    img = np.full((70, 70, 3), 255, dtype=np.uint8)
    got = ops.patch_gather_resize(torch.from_numpy(img).to(DEV), 64, 128, 128, 3, 1, align_corners=True)[0, 0].cpu()
    # patch 3 has 6 valid lines / columns; an upscale by ~2 puts an output between texel 5 (1.0) and texel 6 (0, padding)
    assert float(got[:10, :10].min()) > 1.0 - 1e-6 and float(got[14:, :].max()) == 0.0 and float(got[:, 14:].max()) == 0.0
    assert 0.0 < float(got[11, 0]) < 1.0 and 0.0 < float(got[0, 11]) < 1.0


# ----------------------------------------------------------------------------------------------------------- 2. scatter
def _scatter_reference(pred, H, W, p, mode, first, sentinel=SENTINEL):
    """pred (count, h, w) fp32 on the CPU -> ((H, W) uint8 map, (H, W) fp32 interpolated values; NaN where nothing is written)."""
    from wesup_amd import slide as S
    n_h, n_w = S.patch_grid(H, W, p)
    out = np.full((n_h * p, n_w * p), sentinel, dtype=np.uint8)
    val = np.full((n_h * p, n_w * p), np.nan, dtype=np.float32)
    for n in range(pred.shape[0]):
        k = first + n
        if k >= n_h * n_w:
            continue
        if mode == 0:
            v = F.interpolate(pred[n][None, None].round(), size=(p, p), mode='nearest')[0, 0]
        else:
            v = F.interpolate(pred[n][None, None], size=(p, p), mode='bilinear', align_corners=True)[0, 0]
            val[k // n_w * p:k // n_w * p + p, k % n_w * p:k % n_w * p + p] = v.numpy()
            v = v.round()
        y, x = _corner(k, n_w, p)
        out[y:y + p, x:x + p] = (255 * v).numpy().astype(np.int32).astype(np.uint8)
    return out[:H, :W], val[:H, :W]


def _random_pred(seed, count, h, w, ties):
    rs = np.random.RandomState(seed)
    pred = rs.rand(count, h, w, 2).astype(np.float32)
    if ties:                                                # ties of the rounding: half to even (0.5 -> 0, 1.5 -> 2)
        flat = pred.reshape(-1)
        flat[rs.permutation(flat.size)[:flat.size // 16]] = np.float32(0.5)
        flat[rs.permutation(flat.size)[:flat.size // 16]] = np.float32(1.5)
        flat[rs.permutation(flat.size)[:flat.size // 16]] = np.float32(1.0)
    return torch.from_numpy(pred)


@pytest.mark.parametrize('H,W,p,size', LATTICES)
def test_scatter_nearest_equals_round_interpolate_paste_crop(H, W, p, size):
    from wesup_amd import ops
    from wesup_amd import slide as S
    n_h, n_w = S.patch_grid(H, W, p)
    N = n_h * n_w
    size = size if max(size) <= 600 else (260, 300)                         # (the scatter's grid follows p, not the prediction's size)
    both = _random_pred(H + W + p, N, *size, ties=True)                    # (N, h, w, 2)
    both_d = both.to(DEV)
    for stride in (1, 2):
        pred = both[..., 1].contiguous()
        pred_d = both_d[..., 1].contiguous() if stride == 1 else both_d[..., 1]      # stride 2: class 1 read in place
        out = torch.full((H, W), SENTINEL, dtype=torch.uint8, device=DEV)
        assert ops.patch_scatter_u8(pred_d, out, p, 0, mode=0) is out
        want, _ = _scatter_reference(pred, H, W, p, 0, 0)
        assert np.array_equal(out.cpu().numpy(), want), (stride, int((out.cpu().numpy() != want).sum()))
        assert SENTINEL not in np.unique(want)                               # the lattice covers the slide
        # a pass in the middle of the lattice, and the last one, touch only their own patches
        for first, count in ((N // 2, 1), (max(N - 2, 0), 2)):
            out.fill_(SENTINEL)
            ops.patch_scatter_u8(pred_d[first:first + count], out, p, first, mode=0)
            want, _ = _scatter_reference(pred[first:first + count], H, W, p, 0, first)
            assert np.array_equal(out.cpu().numpy(), want), (stride, first, count)
            assert N == 1 or count >= N or (want == SENTINEL).any()
    if N > 1:                                                                # more predictions than patches are left: not written
        out.fill_(SENTINEL)
        ops.patch_scatter_u8(both_d[:2, :, :, 0].contiguous(), out, p, N - 1, mode=0)
        want, _ = _scatter_reference(both[:2, :, :, 0].contiguous(), H, W, p, 0, N - 1)
        assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize('H,W,p,size', LATTICES)
def test_scatter_bilinear_against_interpolate(H, W, p, size):
    from wesup_amd import ops
    from wesup_amd import slide as S
    n_h, n_w = S.patch_grid(H, W, p)
    N = n_h * n_w
    size = size if max(size) <= 600 else (260, 300)
    both = _random_pred(H * W + p, N, *size, ties=False)
    both_d = both.to(DEV)
    for stride in (1, 2):
        pred_d = both_d[..., 1].contiguous() if stride == 1 else both_d[..., 1]
        out = torch.full((H, W), SENTINEL, dtype=torch.uint8, device=DEV)
        ops.patch_scatter_u8(pred_d, out, p, 0, mode=1)
        want, val = _scatter_reference(both[..., 1].contiguous(), H, W, p, 1, 0)
        near = np.abs(val - 0.5) < ROUND_GUARD
        share = float(near.mean())
        got = out.cpu().numpy()
        print(f'scatter bilinear {H}x{W} p{p} <- {size} stride {stride}: {int((got != want).sum())} pixels differ, '
              f'{int(near.sum())} within {ROUND_GUARD} of 0.5')
        assert share <= 0.01, share
        assert set(np.unique(got)) <= {0, 255}
        assert np.array_equal(got[~near], want[~near]), int(((got != want) & ~near).sum())
    out.fill_(SENTINEL)                                                      # one patch: the others keep the sentinel
    ops.patch_scatter_u8(both_d[N - 1:, :, :, 1], out, p, N - 1, mode=1)
    want, val = _scatter_reference(both[N - 1:, :, :, 1].contiguous(), H, W, p, 1, N - 1)
    near = np.abs(val - 0.5) < ROUND_GUARD
    assert np.array_equal(out.cpu().numpy()[~near], want[~near])


# ------------------------------------------------------------------------------------------------------------ 3. scores
def _counts(S, G, negative):
    if negative:
        S, G = 255 - S, 255 - G
    return [int((S == G).sum()), int(((S > 0) & (G > 0)).sum()), int((S > 0).sum()), int((G > 0).sum())]


@pytest.mark.parametrize('n', [1, 15, 16, 63, 65, 4099, 150 * 131, 4096 * 256 * 16 + 4099])
def test_mask_scores_equal_numpy(n):
    from wesup_amd import ops
    rs = np.random.RandomState(n % 65521)
    kinds = {'random': lambda: (rs.rand(n) < 0.5).astype(np.uint8) * 255, 'zeros': lambda: np.zeros(n, dtype=np.uint8),
             'full': lambda: np.full(n, 255, dtype=np.uint8), 'bytes': lambda: rs.randint(0, 256, n).astype(np.uint8)}
    out = torch.full((4,), -1, dtype=torch.int64, device=DEV)                  # zeroed by the entry
    pairs = (('random', 'random'), ('zeros', 'zeros'), ('full', 'full'), ('zeros', 'full'), ('random', 'zeros'), ('bytes', 'bytes'))
    for ks, kg in (pairs if n < 1 << 20 else pairs[-1:]):                    # (the large size: the grid-stride loop, one pair)
        S, G = kinds[ks](), kinds[kg]()
        S_d, G_d = torch.from_numpy(S).to(DEV), torch.from_numpy(G).to(DEV)
        for negative in (False, True):
            got = ops.mask_scores(S_d, G_d, negative, out=out)
            assert got is out and got.cpu().tolist() == _counts(S, G, negative), (ks, kg, negative)
    if n > 1:                                                                # maps that do not start on a 16-byte boundary
        got = ops.mask_scores(S_d[1:], G_d[1:], True)
        assert got.dtype == torch.int64 and got.cpu().tolist() == _counts(S[1:], G[1:], True)


def test_slide_scores_equal_the_reference():
    from wesup_amd import slide as S
    gold = np.load(GOLDEN)
    for i in range(3):
        pred, gt = gold[f'pair{i}_pred'], gold[f'pair{i}_gt']
        for neg in (0, 1):
            got = S.slide_scores(pred, gt, negative=bool(neg), device=DEV)
            assert isinstance(got[0], float) and isinstance(got[1], float)
            assert got == (float(gold['scores'][i, neg, 0]), float(gold['scores'][i, neg, 1])), (i, neg)
            on_device = S.slide_scores(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), negative=bool(neg))
            assert on_device == got
    post = S.postprocess(gold['blob'], threshold=30, device=DEV)              # the device's two-sided clean-up
    assert post.dtype == np.uint8 and np.array_equal(post, gold['blob_post30'])


# ------------------------------------------------------------------------------------------------------- 4. pipelines
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


def _trainer(**kwargs):
    from wesup_amd.models import initialize_trainer
    trainer = initialize_trainer('wesup', device=DEV, **kwargs)
    trainer.model.load_state_dict({k: torch.from_numpy(v) for k, v in _weights().items()})
    trainer.model.eval()
    return trainer


def _paste(patch_maps, H, W, p):
    from wesup_amd import slide as S
    return S.combine_single_array(np.stack(patch_maps), (H, W))


class _OnePatchDataset:
    """What infer.predict reads of a SegmentationDataset, for one image (an all-zero mask: predict_single_image's postprocess
    takes the argmax of one)."""
    def __init__(self, img_u8):
        self.img = torch.from_numpy(img_u8.astype(np.float32) / np.float32(255)).permute(2, 0, 1)

    def __len__(self):
        return 1

    def __getitem__(self, i):
        return self.img

    def to_reference_item(self, raw):
        return raw, torch.zeros(2, *raw.shape[1:])


def test_superpixel_pipeline_against_the_per_patch_path():
    from wesup_amd import infer as I
    from wesup_amd import ops
    from wesup_amd import slide as S
    H, W, p, size = 150, 131, 80, (48, 64)
    img = _image(IMAGE_SEED, H, W)
    trainer = _trainer(sp_area=64)
    img_d = torch.from_numpy(img).to(DEV)
    n_h, n_w = S.patch_grid(H, W, p)
    assert (n_h, n_w) == (2, 2)
    maps, probs = [], []
    for k in range(n_h * n_w):                                                # the witness: one patch at a time
        x = ops.patch_gather_resize(img_d, p, *size, k, 1).clone()
        mask = torch.zeros(1, 2, *size, device=DEV)
        pred = I.predict_single_image(trainer, x, mask, (p, p))               # untouched: F.interpolate nearest on the device
        maps.append((pred[0, 0].cpu().numpy() * 255).astype(np.uint8))
        with torch.no_grad():
            inp, _ = trainer.preprocess(x)
            prob = trainer.model(inp)[:1].clone()
        probs.append(F.interpolate(prob[None], size=(p, p), mode='nearest')[0, 0].cpu().numpy())
    witness = _paste(maps, H, W, p).astype(np.uint8)
    amb = np.abs(_paste(probs, H, W, p) - 0.5) < AMBIGUOUS
    zeros, ones, share = float((witness == 0).mean()), float((witness == 255).mean()), float(amb.mean())
    print(f'witness map: {zeros:.3f} of the pixels at 0, {ones:.3f} at 255; ambiguous pixels {share:.5f} of the slide')
    assert zeros >= 0.10 and ones >= 0.10, (zeros, ones)                      # not vacuous
    assert share <= MAX_AMBIGUOUS_SHARE, share
    one = S.slide_predict(trainer, img, p, size, batch=1, device=DEV)
    assert one.shape == (H, W) and one.dtype == np.uint8
    assert np.array_equal(one, witness), int((one != witness).sum())
    got = S.slide_predict(trainer, img, p, size, batch=3, device=DEV)         # passes of 3 + 1
    differ = got != witness
    print(f'batch 3: {int(differ.sum())} pixels differ from the witness, {int((differ & ~amb).sum())} of them outside ambiguous pixels')
    assert got.shape == (H, W) and got.dtype == np.uint8 and set(np.unique(got)) <= {0, 255}
    assert np.array_equal(got[~amb], witness[~amb]), int((differ & ~amb).sum())
    kept = S.slide_predict(trainer, img_d, p, size, batch=3, device=DEV, keep_on_device=True)
    assert kept.is_cuda and kept.dtype == torch.uint8 and np.array_equal(kept.cpu().numpy(), got)
    # the interior patch as infer.predict sees it (F.interpolate of the whole patch on the device: the input differs by <= 1e-6
    # and SLIC may move, so no pixel comparison): same shape, dtype and value set once saved as infer.save_predictions does
    ref = I.predict(trainer, _OnePatchDataset(img[:p, :p]), input_size=size, device=DEV)[0]
    ref = ref.astype('uint8') * 255
    mine = one[:p, :p]
    print(f'interior patch: {float((ref == mine).mean()):.4f} of the pixels equal infer.predict\'s')
    assert ref.shape == mine.shape and ref.dtype == mine.dtype and set(np.unique(ref)) | set(np.unique(mine)) <= {0, 255}


def test_pixel_pipeline_against_pixel_infer_of_the_padded_patches():
    from wesup_amd import pixel_infer as PI
    from wesup_amd import slide as S
    from wesup_amd.models.wesup import WESUPPixelInference
    H, W, p, scale = 150, 131, 80, 0.6
    img = _image(IMAGE_SEED, H, W)
    model = WESUPPixelInference().to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in _weights().items()})
    model.eval()
    probs = [PI.pixel_predict(model, patch, (scale,), device=DEV) for patch in S.split_patches_array(img, p)]
    prob = _paste(probs, H, W, p)
    witness = (_paste([np.round(q) for q in probs], H, W, p) * 255).astype(np.uint8)
    amb = np.abs(prob - 0.5) < AMBIGUOUS
    share = float(amb.mean())
    print(f'pixel witness: {float((witness == 0).mean()):.3f} of the pixels at 0, {float((witness == 255).mean()):.3f} at 255; '
          f'ambiguous pixels {share:.5f} of the slide')
    assert share <= MAX_AMBIGUOUS_SHARE, share
    one = S.slide_pixel_predict(model, img, p, scale, batch=1, device=DEV)
    assert one.shape == (H, W) and one.dtype == np.uint8
    assert np.array_equal(one, witness), int((one != witness).sum())
    got = S.slide_pixel_predict(model, img, p, scale, batch=2, device=DEV)
    differ = got != witness
    print(f'pixel batch 2: {int(differ.sum())} pixels differ from the witness, {int((differ & ~amb).sum())} outside ambiguous pixels')
    assert np.array_equal(got[~amb], witness[~amb]), int((differ & ~amb).sum())


# ---------------------------------------------------------------------------------------------------------- 5. driver
def test_driver_writes_and_scores_the_combined_maps(tmp_path):
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
        Image.fromarray(_image(20 + seed, H, W)).save(root / 'images' / f'{stem}.jpg', quality=95)
        Image.fromarray((rs.rand(H, W) < 0.5).astype(np.uint8) * 255).save(root / 'masks' / f'{stem}.png')
    for pixel, name in ((False, 'combined-results-for-ckpt.0001.pth'), (True, 'combined-results-pixel-for-ckpt.0001.pth')):
        lines = []
        got = S.main(root, ckpt, pixel=pixel, patch_size=80, device=DEV, batch=2,
                     log=lambda *a: lines.append(' '.join(str(v) for v in a)))
        out = tmp_path / 'record' / name
        assert sorted(q.name for q in out.iterdir()) == ['negative-b.png', 'positive-a.png']
        for stem, shape in sizes.items():
            written = np.asarray(Image.open(out / f'{stem}.png'))
            assert written.shape == shape and written.dtype == np.uint8 and set(np.unique(written)) <= {0, 255}
            gt = np.asarray(Image.open(root / 'masks' / f'{stem}.png'))
            group, negative = ('negative', True) if stem.startswith('negative-') else ('positive', False)
            assert got[group] == S.slide_scores(written, gt, negative=negative)              # numpy, of what was written
            assert got[group] == S.slide_scores(written, gt, negative=negative, device=DEV)
        text = '\n'.join(lines)
        assert 'Evaluating positive OA and Dice ...' in text and 'Evaluating negative OA and Dice ...' in text
        assert text.count('Accuracy: ') == 2 and text.count('Dice: ') == 2
        assert f'Accuracy: {got["positive"][0]}' in text and f'Dice: {got["negative"][1]}' in text
        assert not (tmp_path / 'val-patches').exists() and not (tmp_path / 'record' / 'results-for-ckpt.0001.pth').exists()
        again = S.main(root, ckpt, pixel=pixel, skip_infer=True, log=lambda *a: None)          # re-scores what is on disk
        assert again == got
