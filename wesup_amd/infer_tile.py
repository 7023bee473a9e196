"""Window-based inference on images larger than the network input (reference infer_tile.py:23-181 and
pixel_infer_tile.py:41-60).

Same strategy as the reference: ``ceil(H / patch) x ceil(W / patch)`` windows whose top-left corners are spread evenly
with ``np.linspace`` (so neighbouring windows overlap when the size is not a multiple of the patch), every window goes
through the model on its own, and overlapping predictions are merged by the mean over the covering windows.  The
window functions are numpy and pinned to the reference's own outputs (tests/golden/tiles.npz); the per-window forward
is the HIP path (``trainer.preprocess`` with the GPU SLIC -> ``WESUP.forward`` -> ``postprocess``, or
``WESUPPixelInference`` for the pixel-wise variant).

``predict_array_batched`` / ``pixel_predict_array_batched`` (``--batch N``) are the same inference with the image resident on
the device: windows cut by ``ops.window_gather``, ``batch`` of them per pass through the network, one ``ops.window_merge``
(equal to ``combine_patches_to_image`` bit for bit) and one copy to the host per image."""
import argparse
import math
from pathlib import Path

import numpy as np
import torch

from . import _lib, ops
from .models import initialize_trainer


def window_grid(height, width, patch_size):
    """Rows and columns of the window lattice: ``ceil(size / patch)`` windows per axis, first window at 0, last window
    flush with the far border, the others spread evenly in between (positions truncated to integers, which is what
    ``np.linspace(..., dtype=int)`` does in infer_tile.py:26-29)."""
    def axis(size):
        if size < patch_size:
            raise ValueError(f'image {height}x{width} is smaller than the patch size {patch_size}')
        return np.linspace(0, size - patch_size, math.ceil(size / patch_size), dtype=int)
    return axis(height), axis(width)


def _get_top_left_coordinates(height, width, patch_size):
    """(top, left) of every window, row-major (the order of infer_tile.py:23-31)."""
    tops, lefts = window_grid(height, width, patch_size)
    return [(int(t), int(l)) for t in tops for l in lefts]


def divide_image_to_patches(img, patch_size):
    """(H, W, 3) uint8 image -> (N, patch_size, patch_size, 3) possibly overlapping windows (infer_tile.py:34-57)."""
    if img.ndim != 3 or img.shape[-1] != 3:
        raise AssertionError('expected an (H, W, 3) image')            # the reference asserts (infer_tile.py:46)
    tops, lefts = window_grid(img.shape[0], img.shape[1], patch_size)
    span = np.arange(patch_size)
    rows = (tops[:, None] + span)[:, None, :, None]                    # (n_h, 1, p, 1)
    cols = (lefts[:, None] + span)[None, :, None, :]                   # (1, n_w, 1, p)
    windows = img[rows, cols]                                          # one gather: (n_h, n_w, p, p, 3)
    return windows.reshape(-1, patch_size, patch_size, 3).astype(np.uint8)


def combine_patches_to_image(patches, target_height, target_width):
    """Merge window predictions (N, p, p[, C]) into one (H, W[, C]) map: the value of a pixel is the mean over the
    windows that cover it (the reference keeps it as a running mean with a per-pixel overlap count,
    infer_tile.py:60-91; here: per-pixel sum and count, divided once -- equal up to float rounding)."""
    patches = np.asarray(patches, dtype=np.float64)
    flat = patches.ndim == 3
    if flat:
        patches = patches[..., None]
    p = patches.shape[1]
    total = np.zeros((target_height, target_width, patches.shape[-1]))
    cover = np.zeros((target_height, target_width, 1))
    for window, (top, left) in zip(patches, _get_top_left_coordinates(target_height, target_width, p)):
        total[top:top + p, left:left + p] += window
        cover[top:top + p, left:left + p] += 1.0
    merged = total / cover                                              # every pixel lies in at least one window
    return merged[..., 0] if flat else np.squeeze(merged)


def _to_tensor(patch, device):
    """uint8 (h, w, 3) -> float (1, 3, h, w) in [0, 1] (torchvision's to_tensor, infer_tile.py:111)."""
    return torch.from_numpy(np.ascontiguousarray(patch)).to(device).permute(2, 0, 1).float().div_(255.).unsqueeze(0)


def predict_array(trainer, img, patch_size, device='cuda'):
    """Window-based superpixel prediction of one (H, W, 3) uint8 image -> (H, W) float map (infer_tile.py:94-119)."""
    patches = divide_image_to_patches(img, patch_size)
    predictions = []
    with torch.no_grad():
        for patch in patches:
            input_, _ = trainer.preprocess(_to_tensor(patch, device))
            prediction = trainer.postprocess(trainer.model(input_))
            predictions.append(prediction.detach().cpu().numpy()[..., np.newaxis])
    predictions = np.concatenate(predictions)
    return combine_patches_to_image(predictions, img.shape[0], img.shape[1])


def pixel_predict_array(model, img, patch_size, device='cuda'):
    """Window-based pixel-wise prediction with WESUPPixelInference -> (H, W) class-1 probability
    (pixel_infer_tile.py:41-60; the caller rounds)."""
    patches = divide_image_to_patches(img, patch_size)
    predictions = []
    with torch.no_grad():
        for patch in patches:
            pred = model(_to_tensor(patch, device))
            predictions.append(np.expand_dims(pred.detach().cpu().numpy()[..., 1], 0))
    predictions = np.concatenate(predictions)
    return combine_patches_to_image(predictions, img.shape[0], img.shape[1])


def window_batches(n_windows, batch):
    """The passes of a batched run over ``n_windows`` windows: ``(first, valid)`` per pass and the batch size used for every
    pass, ``min(batch, n_windows)``.  Each pass asks for ``batch`` windows starting at ``first``; only the first ``valid`` are
    kept -- the tail of a ragged last pass repeats the last window (``ops.window_gather``), so that every pass of an image has
    one shape and the engine keeps one set of buffers."""
    n_windows, batch = int(n_windows), int(batch)
    if n_windows < 1 or batch < 1:
        raise ValueError(f'{n_windows} windows in batches of {batch}')
    batch = min(batch, n_windows)
    return [(first, min(batch, n_windows - first)) for first in range(0, n_windows, batch)], batch


def _upload(img, device):
    """(H, W, 3) image -> uint8 tensor on the device, uploaded once (the cast is divide_image_to_patches')."""
    img = np.asarray(img)
    if img.ndim != 3 or img.shape[-1] != 3:
        raise AssertionError('expected an (H, W, 3) image')
    return torch.from_numpy(np.ascontiguousarray(img.astype(np.uint8, copy=False))).to(device)


def _keep(dst, src, first, valid):
    """dst[first : first + valid] = src[:valid] for contiguous fp32 tensors of one row size: a device copy on the current
    stream (the engine hands out the same prediction buffer at the next pass)."""
    row = dst[0].numel()
    assert src[0].numel() == row and dst.is_contiguous() and src.is_contiguous() and dst.dtype == src.dtype == torch.float32
    _lib.call('wesup_copy', ops._p(dst[first]), ops._p(src), valid * row * 4, ops._stream())


def predict_array_batched(trainer, img, patch_size, batch=4, device='cuda'):
    """``predict_array`` with the image resident on the device: one upload, ``batch`` windows per pass (``ops.window_gather``
    -> ``trainer.preprocess`` with the batched GPU SLIC -> ``trainer.model``), the painted probabilities of all windows kept
    in one (N, p, p, 1) device buffer, one ``ops.window_merge(round_first=True)`` and ONE copy to the host.  Nothing between
    the upload and that copy waits for the device.  Returns the same (H, W) float64 map: equal to ``predict_array`` bit for
    bit at ``batch=1``; at another batch size the convolutions tile differently and a probability moves by ~2e-6, which can
    turn a pixel whose probability sits at 0.5 (tests/test_tiles_gpu.py).

    A trainer with a CPU ``slic_fn`` still segments window by window on the host inside ``preprocess`` (one round trip per
    window); only the forward pass is batched then."""
    p = int(patch_size)
    H, W = img.shape[:2]
    tops, lefts = window_grid(H, W, p)
    passes, batch = window_batches(len(tops) * len(lefts), batch)
    img_d = _upload(img, device)
    kept = torch.empty(len(tops) * len(lefts), p, p, 1, dtype=torch.float32, device=img_d.device)
    x = torch.empty(batch, 3, p, p, dtype=torch.float32, device=img_d.device)
    with torch.no_grad():
        for first, valid in passes:
            ops.window_gather(img_d, tops, lefts, p, first, batch, out=x)
            input_, _ = trainer.preprocess(x)
            _keep(kept, trainer.model(input_), first, valid)
        merged = ops.window_merge(kept, tops, lefts, H, W, round_first=True)
    return merged.view(H, W).cpu().numpy()


def pixel_predict_array_batched(model, img, patch_size, batch=2, device='cuda'):
    """``pixel_predict_array`` with the image resident on the device: ``batch`` windows per
    ``WESUPPixelInference.forward_batch`` (mind its memory: ~3.6 GB per 464 x 464 window), class 1 of every window kept on
    the device, one ``ops.window_merge`` of the probabilities and one copy to the host (the caller rounds)."""
    p = int(patch_size)
    H, W = img.shape[:2]
    tops, lefts = window_grid(H, W, p)
    passes, batch = window_batches(len(tops) * len(lefts), batch)
    img_d = _upload(img, device)
    kept = torch.empty(len(tops) * len(lefts), p, p, 1, dtype=torch.float32, device=img_d.device)
    x = torch.empty(batch, 3, p, p, dtype=torch.float32, device=img_d.device)
    with torch.no_grad():
        for first, valid in passes:
            ops.window_gather(img_d, tops, lefts, p, first, batch, out=x)
            pred = model.forward_batch(x)                                 # (batch, p, p, C)
            kept[first:first + valid, :, :, 0].copy_(pred[:valid, :, :, 1])     # a strided device copy, no arithmetic
        merged = ops.window_merge(kept, tops, lefts, H, W, round_first=False)
    return merged.view(H, W).cpu().numpy()


def predict(trainer, img_path, patch_size, device='cuda', batch=None):
    """One image file -> (H, W) map; ``batch=None`` is the per-window path, a number the device-resident one."""
    from PIL import Image
    img = np.asarray(Image.open(img_path).convert('RGB'))
    if batch is None:
        return predict_array(trainer, img, patch_size, device=device)
    return predict_array_batched(trainer, img, patch_size, batch=batch, device=device)


def save_predictions(predictions, img_paths, output_dir='predictions'):
    from PIL import Image
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    for pred, img_path in zip(predictions, img_paths):
        Image.fromarray(pred.astype('uint8') * 255).save(output_dir / Path(img_path).name)


def infer(trainer, data_dir, patch_size, output_dir=None, device='cuda', batch=None):
    """Window-based inference on ``data_dir/images`` (infer_tile.py:143-162)."""
    trainer.model.eval()
    data_dir = Path(data_dir).expanduser()
    img_paths = sorted((data_dir / 'images').iterdir())
    predictions = [predict(trainer, p, patch_size, device=device, batch=batch) for p in img_paths]
    if output_dir is not None:
        save_predictions(predictions, img_paths, output_dir)
    return predictions


def pixel_infer(model, data_dir, patch_size, output_dir=None, device='cuda', batch=None):
    """Pixel-wise window inference on ``data_dir/images`` (pixel_infer_tile.py:41-60): the merged class-1 probabilities are
    rounded here, before they are saved."""
    from PIL import Image
    model.eval()
    data_dir = Path(data_dir).expanduser()
    img_paths = sorted((data_dir / 'images').iterdir())
    predictions = []
    for path in img_paths:
        img = np.asarray(Image.open(path).convert('RGB'))
        if batch is None:
            merged = pixel_predict_array(model, img, patch_size, device=device)
        else:
            merged = pixel_predict_array_batched(model, img, patch_size, batch=batch, device=device)
        predictions.append(merged.round())
    if output_dir is not None:
        save_predictions(predictions, img_paths, output_dir)
    return predictions


def _load_pixel_model(checkpoint, device):
    from .models.wesup import WESUPPixelInference
    model = WESUPPixelInference().to(device)
    if checkpoint is not None:
        from .models import require_two_class_checkpoint
        require_two_class_checkpoint(checkpoint, 'tile / pixel inference')
        model.load_state_dict(torch.load(checkpoint, map_location=device)['model_state_dict'])
    return model


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('data_dir')
    ap.add_argument('--model-type', default='wesup')
    ap.add_argument('--patch-size', type=int, default=464)          # infer_tile.py:165
    ap.add_argument('--checkpoint')
    ap.add_argument('--output-dir')
    ap.add_argument('--device', default='cuda')
    ap.add_argument('--batch', type=int, default=None,
                    help='windows per pass of the device-resident path (default: the per-window path)')
    ap.add_argument('--pixel', action='store_true',
                    help='pixel-wise inference with WESUPPixelInference (pixel_infer_tile.py)')
    a = ap.parse_args(argv)
    output_dir = a.output_dir
    if output_dir is None and a.checkpoint is not None:
        output_dir = Path(a.checkpoint).expanduser().parent.parent / 'results'
    if a.pixel:
        model = _load_pixel_model(a.checkpoint, a.device)
        pixel_infer(model, a.data_dir, a.patch_size, output_dir, device=a.device, batch=a.batch)
        return
    trainer = initialize_trainer(a.model_type, device=a.device)
    if a.checkpoint is not None:
        from .models import require_two_class_checkpoint
        require_two_class_checkpoint(a.checkpoint, 'tile inference')
        trainer.load_checkpoint(a.checkpoint)
    infer(trainer, a.data_dir, a.patch_size, output_dir, device=a.device, batch=a.batch)


if __name__ == '__main__':
    main()
