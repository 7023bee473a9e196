"""Window inference with the image resident on the device (infer_tile.predict_array_batched / pixel_predict_array_batched,
csrc/tiles.hip) against the per-window path it stands beside (predict_array / pixel_predict_array, untouched).

The two kernels are held to the host functions bit for bit: the gather to ``_to_tensor`` over ``divide_image_to_patches`` for
all 256 byte values, the merge to ``combine_patches_to_image`` (same adds in the same order on fp64, one IEEE division).  The
batched paths are equal to the per-window ones at batch 1; at another batch size the convolutions tile differently and a
painted probability moves by ~2e-6 (profiles/tolerances_shards_multiscale.json), so the rounded maps are compared outside
AMBIGUOUS pixels -- pixels where some covering window's single-run probability lies within 1e-5 of 0.5, the bar of the shard
tests for floats, batched against single -- and those must be at most 1 % of the image.

Weights: oracle.make_weights(3), the seed of smoke(), at feat_scale 1.0.  Random weights put every superpixel on one side of 0.5, which would make the
comparison of rounded maps vacuous; classifier.0.bias[1] is therefore lowered by SHIFT, the median of the logit difference
z1 - z0 over the superpixels of window 0 of the 150 x 333 image (measured once with these seeds, kept here as a constant), and
the test asserts that at least 10 % of the per-window map is 0 and at least 10 % is 1.  (The median of 63 values is one of them:
that superpixel's probability is 0.5 to rounding, so the 150 x 333 case always has a few ambiguous pixels to mask.)"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tol                # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SIZES = [(64, 64, 64), (80, 112, 64), (128, 192, 64), (150, 333, 64), (522, 775, 464)]
WEIGHT_SEED, FEAT_SCALE, IMAGE_SEED = 3, 1.0, 5
SHIFT = -0.36169204115867615      # median z1 - z0 over the 63 superpixels of window 0 (see the module docstring)
AMBIGUOUS = 1e-5     # |p - 0.5| below this: the rounded value may differ between two batch sizes
MAX_AMBIGUOUS_SHARE = 0.01


def _image(seed, H, W):
    from wesup_amd import synth
    return np.ascontiguousarray((synth.synth_image(seed, H, W).transpose(1, 2, 0) * 255).astype(np.uint8))


def _all_bytes_image(seed, H, W):
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    img.reshape(-1)[rs.permutation(img.size)[:256]] = np.arange(256, dtype=np.uint8)
    assert len(np.unique(img)) == 256
    return img


def _weights(shift=None):
    from oracle import wesup_oracle as orc
    w = orc.make_weights(WEIGHT_SEED, feat_scale=FEAT_SCALE)
    b = w['classifier.0.bias'].copy()
    b[1] -= np.float32(SHIFT if shift is None else shift)
    w['classifier.0.bias'] = b
    return w


def _trainer(weights, **kwargs):
    from wesup_amd.models import initialize_trainer
    trainer = initialize_trainer('wesup', device=DEV, **kwargs)
    trainer.model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    trainer.model.eval()
    return trainer


def _per_window(trainer, img, p):
    """The per-window path by hand: (painted probabilities (N,p,p) fp32, SLIC label maps (N,p,p) int32), one window at a time."""
    from wesup_amd import infer_tile as T
    probs, labels = [], []
    with torch.no_grad():
        for patch in T.divide_image_to_patches(img, p):
            x = T._to_tensor(patch, DEV)
            labels.append(trainer.slic(x)[0][0].cpu().numpy())
            inp, _ = trainer.preprocess(x)
            probs.append(trainer.model(inp)[0].cpu().numpy())
    return np.stack(probs), np.stack(labels)


def _ambiguous_map(probs, H, W):
    """Pixels of the image where some covering window's probability is within AMBIGUOUS of 0.5."""
    from wesup_amd import infer_tile as T
    near = (np.abs(probs.astype(np.float64) - 0.5) < AMBIGUOUS).astype(np.float64)
    return T.combine_patches_to_image(near, H, W) > 0


def _batched_slic_equals_single(trainer, img, p, batch, single_labels):
    from wesup_amd import infer_tile as T
    from wesup_amd import ops
    H, W = img.shape[:2]
    tops, lefts = T.window_grid(H, W, p)
    N = len(tops) * len(lefts)
    passes, batch = T.window_batches(N, batch)
    img_d = torch.from_numpy(img).to(DEV)
    for first, valid in passes:
        x = ops.window_gather(img_d, tops, lefts, p, first, batch)
        lab = trainer.slic(x)[0].cpu().numpy()
        for i in range(batch):                           # the padded tail repeats the last window
            assert np.array_equal(lab[i], single_labels[min(first + i, N - 1)]), (batch, first, i)


# ------------------------------------------------------------------------------------------------------------ 1. gather
@pytest.mark.parametrize('H,W,p', SIZES)
def test_window_gather_equals_to_tensor_of_the_host_windows(H, W, p):
    from wesup_amd import infer_tile as T
    from wesup_amd import ops
    img = _all_bytes_image(H * 1000 + W, H, W)
    tops, lefts = T.window_grid(H, W, p)
    N = len(tops) * len(lefts)
    want = torch.cat([T._to_tensor(patch, DEV).contiguous() for patch in T.divide_image_to_patches(img, p)])
    img_d = torch.from_numpy(img).to(DEV)
    got = ops.window_gather(img_d, tops, lefts, p, 0, N)
    assert got.shape == (N, 3, p, p) and got.dtype == torch.float32
    assert torch.equal(got, want)
    # a range that runs past the end repeats the last window; one that starts inside the lattice starts there
    first = max(N - 2, 0)
    tail = ops.window_gather(img_d, tops, lefts, p, first, 5)
    for i in range(5):
        assert torch.equal(tail[i], want[min(first + i, N - 1)]), i


def test_window_gather_scales_every_byte_like_aten():
    """All 256 byte values through ``_to_tensor`` on the device and through the kernel: the same 256 floats."""
    from wesup_amd import infer_tile as T
    from wesup_amd import ops
    img = np.arange(256, dtype=np.uint8).repeat(3).reshape(16, 16, 3)
    want = T._to_tensor(img, DEV).contiguous()
    got = ops.window_gather(torch.from_numpy(img).to(DEV), [0], [0], 16, 0, 1)
    assert torch.equal(got, want)
    assert torch.equal(got[0, 0].reshape(-1).cpu(), torch.arange(256, dtype=torch.float32) * torch.tensor(1.0 / 255.0).float())


def test_a_patch_size_that_is_not_a_multiple_of_four():
    """The gather stores four pixels at a time when the patch size allows it, one at a time otherwise: the other form, and the
    merge at the same odd size."""
    from wesup_amd import infer_tile as T
    from wesup_amd import ops
    H, W, p = 75, 101, 37
    img = _all_bytes_image(7, H, W)
    tops, lefts = T.window_grid(H, W, p)
    N = len(tops) * len(lefts)
    want = torch.cat([T._to_tensor(patch, DEV).contiguous() for patch in T.divide_image_to_patches(img, p)])
    assert torch.equal(ops.window_gather(torch.from_numpy(img).to(DEV), tops, lefts, p, 0, N + 1)[:N], want)
    pred = np.random.RandomState(8).rand(N, p, p, 2).astype(np.float32)
    got = ops.window_merge(torch.from_numpy(pred).to(DEV), tops, lefts, H, W, round_first=True)
    assert np.array_equal(got.cpu().numpy(), T.combine_patches_to_image(np.round(pred), H, W))


# ------------------------------------------------------------------------------------------------------------- 2. merge
@pytest.mark.parametrize('C', [1, 2])
@pytest.mark.parametrize('H,W,p', SIZES)
def test_window_merge_equals_the_host_merge(H, W, p, C):
    from wesup_amd import infer_tile as T
    from wesup_amd import ops
    tops, lefts = T.window_grid(H, W, p)
    N = len(tops) * len(lefts)
    rs = np.random.RandomState(H + W + C)
    pred = rs.rand(N, p, p, C).astype(np.float32)
    flat = pred.reshape(-1)
    flat[rs.permutation(flat.size)[:flat.size // 16]] = np.float32(0.5)       # ties of the rounding: half to even
    flat[rs.permutation(flat.size)[:flat.size // 16]] = np.float32(1.0)
    pred_d = torch.from_numpy(pred).to(DEV)
    for round_first in (False, True):
        host = T.combine_patches_to_image(np.round(pred) if round_first else pred, H, W).reshape(H, W, C)
        got = ops.window_merge(pred_d, tops, lefts, H, W, round_first=round_first)
        assert got.shape == (H, W, C) and got.dtype == torch.float64
        assert np.array_equal(got.cpu().numpy(), host), (round_first, float(np.abs(got.cpu().numpy() - host).max()))
    # the (N,p,p) form of a one-channel prediction
    if C == 1:
        got = ops.window_merge(pred_d[..., 0].contiguous(), tops, lefts, H, W)
        assert np.array_equal(got.cpu().numpy(), T.combine_patches_to_image(pred[..., 0], H, W))


# ------------------------------------------------------------------------------- 3. superpixel path against per-window
def test_batched_superpixel_path_against_the_per_window_path():
    from wesup_amd import infer_tile as T
    H, W, p = 150, 333, 64
    img = _image(IMAGE_SEED, H, W)
    trainer = _trainer(_weights(), sp_area=64)
    single = T.predict_array(trainer, img, p, device=DEV)
    probs, labels = _per_window(trainer, img, p)
    assert len(probs) == 18
    assert np.array_equal(single, T.combine_patches_to_image(np.round(probs), H, W))
    zeros, ones = float((single == 0).mean()), float((single == 1).mean())
    amb = _ambiguous_map(probs, H, W)
    share = float(amb.mean())
    print(f'per-window map: {zeros:.3f} of the pixels at 0, {ones:.3f} at 1; ambiguous pixels {share:.5f} of the image')
    assert zeros >= 0.10 and ones >= 0.10, (zeros, ones)                      # not vacuous
    assert share <= MAX_AMBIGUOUS_SHARE, share
    # batch 1: the same inputs through the same kernels
    assert np.array_equal(T.predict_array_batched(trainer, img, p, batch=1, device=DEV), single)
    for batch in (3, 4):                                                       # 18 windows: batch 4 has a ragged tail
        _batched_slic_equals_single(trainer, img, p, batch, labels)
        got = T.predict_array_batched(trainer, img, p, batch=batch, device=DEV)
        assert got.shape == (H, W) and got.dtype == np.float64
        differ = got != single
        print(f'batch {batch}: {int(differ.sum())} pixels differ from the per-window map, {int((differ & ~amb).sum())} of them '
              f'outside ambiguous pixels')
        assert np.array_equal(got[~amb], single[~amb]), (batch, int((differ & ~amb).sum()))


# ------------------------------------------------------------------------------------------------------- 4. pixel path
def test_batched_pixel_path_against_the_per_window_path():
    from wesup_amd import infer_tile as T
    from wesup_amd.models.wesup import WESUPPixelInference
    H, W, p = 150, 270, 64                                                     # 3 x 5 windows: batch 2 has a ragged tail
    img = _image(IMAGE_SEED + 1, H, W)
    model = WESUPPixelInference().to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in _weights().items()})
    model.eval()
    single = T.pixel_predict_array(model, img, p, device=DEV)
    assert single.shape == (H, W) and single.min() >= 0.0 and single.max() <= 1.0
    assert np.array_equal(T.pixel_predict_array_batched(model, img, p, batch=1, device=DEV), single)
    with pytest.raises(ValueError):
        model(torch.zeros(2, 3, p, p, device=DEV))                             # forward itself still takes one image
    for batch in (2, 3):
        got = T.pixel_predict_array_batched(model, img, p, batch=batch, device=DEV)
        err = float(np.abs(got - single).max())
        print(f'pixel path, batch {batch}: max |p_batched - p_single| = {err:.3e}')
        assert _tol.within(f'tiles pixel 150x270 p64 batch {batch}', 'window inference, pixel probabilities, batched vs single',
                           err, 1e-5, 'max |p_batch - p_single| of the merged class-1 probability (scale 1)'), (batch, err)


# ---------------------------------------------------------------------------------------- 5. determinism and a real size
def test_batched_path_is_deterministic_at_a_real_size(tmp_path):
    from PIL import Image
    from wesup_amd import infer_tile as T
    H, W, p = 1000, 1400, 464
    img = _image(IMAGE_SEED + 2, H, W)
    trainer = _trainer(_weights())                                             # default sp_area
    a = T.predict_array_batched(trainer, img, p, batch=4, device=DEV)
    b = T.predict_array_batched(trainer, img, p, batch=4, device=DEV)
    assert a.shape == (H, W) and np.array_equal(a, b)
    one = T.predict_array_batched(trainer, img, p, batch=1, device=DEV)
    probs, _ = _per_window(trainer, img, p)
    assert np.array_equal(one, T.combine_patches_to_image(np.round(probs), H, W))
    amb = _ambiguous_map(probs, H, W)
    share = float(amb.mean())
    print(f'1000x1400: ambiguous pixels {share:.5f} of the image; {int((a != one).sum())} pixels differ between batch 4 and 1')
    assert share <= MAX_AMBIGUOUS_SHARE, share
    assert np.array_equal(a[~amb], one[~amb]), int(((a != one) & ~amb).sum())
    (tmp_path / 'd' / 'images').mkdir(parents=True)
    Image.fromarray(img).save(tmp_path / 'd' / 'images' / 'slide.png')
    preds = T.infer(trainer, tmp_path / 'd', p, output_dir=tmp_path / 'out', device=DEV, batch=4)
    assert len(preds) == 1 and np.array_equal(preds[0], a)
    saved = np.asarray(Image.open(tmp_path / 'out' / 'slide.png'))
    assert np.array_equal(saved, a.astype('uint8') * 255)
