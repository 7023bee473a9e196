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
(equal to ``combine_patches_to_image`` bit for bit) and one copy to the host per image.

A model of more than two classes gives a class map, (H, W) uint8 class indices: ``predict_array_classes`` /
``pixel_predict_array_classes`` and their ``_batched`` forms, which ``infer`` / ``pixel_infer`` take for ``n_classes > 2``.  The
pixel-wise paths merge the C probabilities as class 1 is merged above and take the first maximum (a soft vote); on the superpixel
paths every covering window votes with the class index it painted and the first maximum of the counts wins (a hard vote);
``combine_patches_to_classes`` states both.

Test-time augmentation (``--tta {flips,rot,d4}``, ``views=`` on all eight forms): every window is predicted under
each view of a list -- quarter turns and their mirror images, ``apply_view`` -- every prediction is turned back and the mean runs
over windows x views (``combine_views_to_image`` / ``combine_views_to_classes``, the specification).  The superpixel model is
segmented afresh under every view, so the views' tessellations differ and their mean resolves boundaries below superpixel size;
with two classes it merges un-rounded probabilities under views.  The device-resident forms hand the list on as ``views=``: the
same ``ops.window_gather`` cuts and turns in one kernel, the same ``ops.window_merge`` / ``ops.window_merge_classes`` merge through
the inverse index (no views is their one-upright-view case).  V views cost V times the forward work; what they gain in accuracy
has not been measured here (no trained checkpoint)."""
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


def combine_patches_to_classes(patches, target_height, target_width, n_classes, votes=False):
    """The class map of merged window predictions -> (H, W) uint8.  ``votes=False``: patches (N, p, p, C) probabilities; the
    argmax of ``combine_patches_to_image`` (np.argmax: the first maximum).  ``votes=True``: patches (N, p, p) class indices; every
    covering window votes -- the argmax of ``combine_patches_to_image`` over the one-hot votes, so a tie of the counts goes to the
    lowest class.  A vote outside [0, n_classes) (or a NaN) counts for no class.  With two classes the hard vote is
    ``round(combine_patches_to_image(round(p)))``: the mean of the rounded values is above 0.5 exactly when class 1 has more
    votes, and np.round takes the tie at 0.5 to 0."""
    C = int(n_classes)
    patches = np.asarray(patches)
    if votes:
        if patches.ndim != 3:
            raise ValueError(f'votes: expected (N, p, p) class indices, got {patches.shape}')
        idx = np.rint(patches.astype(np.float64))
        patches = (idx[..., None] == np.arange(C, dtype=np.float64)).astype(np.float64)      # (a NaN equals no class)
    elif patches.ndim != 4 or patches.shape[-1] != C:
        raise ValueError(f'expected (N, p, p, {C}) probabilities, got {patches.shape}')
    merged = combine_patches_to_image(patches, target_height, target_width).reshape(target_height, target_width, C)
    return merged.argmax(axis=-1).astype(np.uint8)


# ------------------------------------------------------------------ test-time augmentation over the dihedral group
# View v = r + 4 f: a left-right mirror first when f, then r counter-clockwise quarter turns.  4 is the left-right mirror, 6 the
# up-down mirror, 2 the half turn.  These host functions are the specification of the device path.
VIEW_SETS = {'none': (0,), 'flips': (0, 2, 4, 6), 'rot': (0, 1, 2, 3), 'd4': (0, 1, 2, 3, 4, 5, 6, 7)}


def check_views(views):
    """A view list as a tuple: 1 to 8 distinct indices in [0, 8), in any order; anything else is a ValueError."""
    try:
        out = tuple(int(v) for v in views)
        exact = all(v == w for v, w in zip(out, views))
    except (TypeError, ValueError):
        raise ValueError(f'views {views!r}: expected 1 to 8 distinct view indices in [0, 8)') from None
    if not exact or not 1 <= len(out) <= 8 or len(set(out)) != len(out) or any(not 0 <= v < 8 for v in out):
        raise ValueError(f'views {views!r}: expected 1 to 8 distinct view indices in [0, 8)')
    return out


def _view(v):
    v = int(v)
    if not 0 <= v < 8:
        raise ValueError(f'view {v}: expected an index in [0, 8)')
    return v & 3, v >> 2


def apply_view(a, v):
    """View ``v`` of a square (p, p[, ...]) array: the mirror first, then the quarter turns, on the first two axes."""
    r, f = _view(v)
    return np.rot90(a[:, ::-1] if f else a, k=r, axes=(0, 1))


def invert_view(b, v):
    """What ``apply_view(., v)`` was applied to: the quarter turns back, then the mirror."""
    r, f = _view(v)
    x = np.rot90(b, k=-r, axes=(0, 1))
    return x[:, ::-1] if f else x


def combine_views_to_image(patches, views, target_height, target_width):
    """``combine_patches_to_image`` over windows x views: patches (N, V, p, p[, C]), every prediction in the space of its view ->
    (H, W[, C]) fp64.  ``total`` starts at 0.0; for every window in row-major order, and inside it for every view in the order
    of ``views``, ``invert_view(patch, v)`` is added; one division by ``cover * V``.  The order is part of the definition: sums
    of probabilities that span many binades are not associative."""
    views = check_views(views)
    patches = np.asarray(patches, dtype=np.float64)
    flat = patches.ndim == 4
    if flat:
        patches = patches[..., None]
    if patches.ndim != 5 or patches.shape[1] != len(views) or patches.shape[2] != patches.shape[3]:
        raise ValueError(f'expected (N, {len(views)}, p, p[, C]) predictions, got {patches.shape}')
    p = patches.shape[2]
    total = np.zeros((target_height, target_width, patches.shape[-1]))
    cover = np.zeros((target_height, target_width, 1))
    for window, (top, left) in zip(patches, _get_top_left_coordinates(target_height, target_width, p)):
        for patch, v in zip(window, views):
            total[top:top + p, left:left + p] += invert_view(patch, v)
        cover[top:top + p, left:left + p] += 1.0
    merged = total / (cover * len(views))                               # every pixel lies in at least one window
    return merged[..., 0] if flat else np.squeeze(merged)


def combine_views_to_classes(patches, views, target_height, target_width, n_classes, votes=False):
    """``combine_patches_to_classes`` over the same windows x views -> (H, W) uint8.  ``votes=False``: patches (N, V, p, p, C)
    probabilities, the first maximum of the per-class means.  ``votes=True``: patches (N, V, p, p) class indices; every
    (window, view) votes, a tie goes to the lowest class, an invalid index counts for nothing."""
    C = int(n_classes)
    patches = np.asarray(patches)
    if votes:
        if patches.ndim != 4:
            raise ValueError(f'votes: expected (N, V, p, p) class indices, got {patches.shape}')
        idx = np.rint(patches.astype(np.float64))
        patches = (idx[..., None] == np.arange(C, dtype=np.float64)).astype(np.float64)      # (a NaN equals no class)
    elif patches.ndim != 5 or patches.shape[-1] != C:
        raise ValueError(f'expected (N, V, p, p, {C}) probabilities, got {patches.shape}')
    merged = combine_views_to_image(patches, views, target_height, target_width).reshape(target_height, target_width, C)
    return merged.argmax(axis=-1).astype(np.uint8)


def _to_tensor(patch, device):
    """uint8 (h, w, 3) -> float (1, 3, h, w) in [0, 1] (torchvision's to_tensor, infer_tile.py:111)."""
    return torch.from_numpy(np.ascontiguousarray(patch)).to(device).permute(2, 0, 1).float().div_(255.).unsqueeze(0)


def _host_windows(img, patch_size, stain, device, forward, views=None):
    """The per-window walk: the stain round trip, the cut on the host, ``forward(window tensor)`` -> numpy array with a leading
    axis of 1 for every window under ``torch.no_grad()``.  Returns (the (N, ...) concatenation, H, W).  With ``views``: every
    window goes through ``forward`` once per view, as ``apply_view(window, v)``, and the array is (N, V, ...): every prediction in
    the space of its view."""
    img = _stained(img, stain, device)
    with torch.no_grad():
        if views is None:
            predictions = [forward(_to_tensor(patch, device)) for patch in divide_image_to_patches(img, patch_size)]
        else:
            predictions = [np.concatenate([forward(_to_tensor(apply_view(patch, v), device)) for v in check_views(views)])[np.newaxis]
                           for patch in divide_image_to_patches(img, patch_size)]
    return np.concatenate(predictions), img.shape[0], img.shape[1]


def _merge_host(merge, merge_views, walk, views, *args, **kw):
    """The merge of a per-window form: ``walk`` is ``_host_windows``' (predictions, H, W)."""
    pred, H, W = walk
    if views is None:
        return merge(pred, H, W, *args, **kw)
    return merge_views(pred, check_views(views), H, W, *args, **kw)


def predict_array(trainer, img, patch_size, device='cuda', stain=None, views=None):
    """Window-based superpixel prediction of one (H, W, 3) uint8 image -> (H, W) float map (infer_tile.py:94-119).

    ``views`` (a view list, ``VIEW_SETS``): test-time augmentation.  Every window is segmented and predicted once per view; what
    is merged are the UN-ROUNDED painted class-1 probabilities of all windows x views (a soft vote,
    ``combine_views_to_image``) -- without views every window is rounded first, which is the reference's behaviour and stays.
    The caller rounds the merged map once (``infer`` does)."""
    def forward(x):
        input_, _ = trainer.preprocess(x)
        pred = trainer.model(input_)
        if views is None:
            pred = trainer.postprocess(pred)
        return pred.detach().cpu().numpy()[..., np.newaxis]
    return _merge_host(combine_patches_to_image, combine_views_to_image, _host_windows(img, patch_size, stain, device, forward, views),
                       views)


def pixel_predict_array(model, img, patch_size, device='cuda', stain=None, views=None):
    """Window-based pixel-wise prediction with WESUPPixelInference -> (H, W) class-1 probability
    (pixel_infer_tile.py:41-60; the caller rounds).  ``views``: the mean over windows x views."""
    def forward(x):
        return np.expand_dims(model(x).detach().cpu().numpy()[..., 1], 0)
    return _merge_host(combine_patches_to_image, combine_views_to_image, _host_windows(img, patch_size, stain, device, forward, views),
                       views)


def _n_classes(model):
    return int(getattr(model, 'n_classes', None) or 2)


def _check_status(status, n_classes, what):
    """Raise when a device path met a painted class index outside [0, n_classes) (the status word of the class-map entries, read
    once, after the map has been copied back)."""
    if int(status.cpu()) != 0:
        raise RuntimeError(f'{what}: the model painted a class index outside [0, {n_classes})')


def predict_array_classes(trainer, img, patch_size, device='cuda', stain=None, views=None):
    """``predict_array`` for a model of more than two classes -> (H, W) uint8 class map: every window's painted class indices
    (what ``trainer.model`` returns for C > 2) come to the host and vote (``combine_patches_to_classes(votes=True)``).  ``views``:
    every (window, view) votes (``combine_views_to_classes``)."""
    def forward(x):
        input_, _ = trainer.preprocess(x)
        return trainer.model(input_).detach().cpu().numpy()                                # (1, p, p) class indices
    return _merge_host(combine_patches_to_classes, combine_views_to_classes, _host_windows(img, patch_size, stain, device, forward, views),
                       views, _n_classes(trainer.model), votes=True)


def pixel_predict_array_classes(model, img, patch_size, device='cuda', stain=None, views=None):
    """``pixel_predict_array`` for a model of more than two classes -> (H, W) uint8 class map: all C probabilities of every
    window (and view) are merged on the host, then the first maximum."""
    def forward(x):
        return model(x).detach().cpu().numpy()[np.newaxis]                                 # (1, p, p, C)
    return _merge_host(combine_patches_to_classes, combine_views_to_classes, _host_windows(img, patch_size, stain, device, forward, views),
                       views, _n_classes(model))


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


def _upload(img, device, stain=None):
    """(H, W, 3) image -> uint8 tensor on the device, uploaded once (the cast is divide_image_to_patches').  ``stain`` (a
    wesup_amd.stain.StainNormalizer): fitted once on the resident tensor and applied in place, in front of every window gather."""
    img = np.asarray(img)
    if img.ndim != 3 or img.shape[-1] != 3:
        raise AssertionError('expected an (H, W, 3) image')
    img_d = torch.from_numpy(np.ascontiguousarray(img.astype(np.uint8, copy=False))).to(device)
    if stain is not None:
        stain(img_d, out=img_d)
    return img_d


def _stained(img, stain, device):
    """The per-window paths cut their windows on the host: one upload, one normalisation, one copy back in front of them."""
    if stain is None:
        return img
    return _upload(img, device, stain).cpu().numpy()


def _keep(dst, src, first, valid):
    """dst[first : first + valid] = src[:valid] for contiguous fp32 tensors of one row size: a device copy on the current
    stream (the engine hands out the same prediction buffer at the next pass)."""
    row = dst[0].numel()
    assert src[0].numel() == row and dst.is_contiguous() and src.is_contiguous() and dst.dtype == src.dtype == torch.float32
    _lib.call('wesup_copy', ops._p(dst[first]), ops._p(src), valid * row * 4, ops._stream())


def _resident_windows(img, patch_size, batch, stain, device, forward, tail, keep=_keep, views=None):
    """The device-resident walk: one upload, the lattice, ``batch`` windows per pass -- ``ops.window_gather`` into one reused
    input, ``forward(x)`` -> (batch, p, p, *tail) fp32 under ``torch.no_grad()``, ``keep`` of the pass's valid windows.  Nothing
    in it waits for the device.  Returns (the (N, p, p, *tail) device buffer of all windows, tops, lefts, H, W).

    With ``views`` (V of them) a view is one more index on the slot axis: N * V slots, slot ``s`` window ``s // V`` under view
    ``views[s % V]``, ``batch`` SLOTS per pass cut and turned by ``ops.window_gather(views=...)``, and the buffer is
    (N, V, p, p, *tail), every prediction in the space of its view.  It grows V-fold: the pixel-wise model at C = 16, p = 464,
    16 windows and all eight views keeps 16 * 8 * 464 * 464 * 16 * 4 bytes, about 1.8 GB."""
    p = int(patch_size)
    H, W = img.shape[:2]
    tops, lefts = window_grid(H, W, p)
    N = len(tops) * len(lefts)
    lead = (N,) if views is None else (N, len(check_views(views)))       # (the buffer has a V axis only under views)
    passes, batch = window_batches(math.prod(lead), batch)
    img_d = _upload(img, device, stain)                              # (a stain fit happens once, on the upright image)
    kept = torch.empty(*lead, p, p, *tail, dtype=torch.float32, device=img_d.device)
    slots = kept.view(-1, p, p, *tail)                               # (kept itself without views)
    x = torch.empty(batch, 3, p, p, dtype=torch.float32, device=img_d.device)
    with torch.no_grad():
        for first, valid in passes:
            ops.window_gather(img_d, tops, lefts, p, first, batch, out=x, views=views)
            keep(slots, forward(x), first, valid)
    return kept, tops, lefts, H, W


def predict_array_batched(trainer, img, patch_size, batch=4, device='cuda', stain=None, views=None):
    """``predict_array`` with the image resident on the device: one upload, ``batch`` windows per pass (``ops.window_gather``
    -> ``trainer.preprocess`` with the batched GPU SLIC -> ``trainer.model``), the painted probabilities of all windows kept
    in one (N, p, p, 1) device buffer, one ``ops.window_merge(round_first=True)`` and ONE copy to the host.  Nothing between
    the upload and that copy waits for the device.  Returns the same (H, W) float64 map: equal to ``predict_array`` bit for
    bit at ``batch=1``; at another batch size the convolutions tile differently and a probability moves by ~2e-6, which can
    turn a pixel whose probability sits at 0.5 (tests/test_tiles_gpu.py).

    ``views``: ``predict_array``'s test-time augmentation on the device -- ``batch`` (window, view) slots per pass, the un-rounded
    painted probabilities of all N x V slots kept (V times the memory and the forward work), ONE ``ops.window_merge(views=...)``
    that reads every view through its inverse index, one copy.  Equal to ``predict_array(views=...)`` bit for bit at ``batch=1``; the
    three other ``_batched`` forms take ``views`` the same way.

    A trainer with a CPU ``slic_fn`` still segments window by window on the host inside ``preprocess`` (one round trip per
    window); only the forward pass is batched then."""
    def forward(x):
        input_, _ = trainer.preprocess(x)
        return trainer.model(input_)
    kept, tops, lefts, H, W = _resident_windows(img, patch_size, batch, stain, device, forward, (1,), views=views)
    merged = ops.window_merge(kept, tops, lefts, H, W, round_first=views is None, views=views)
    return merged.view(H, W).cpu().numpy()


def pixel_predict_array_batched(model, img, patch_size, batch=2, device='cuda', stain=None, views=None):
    """``pixel_predict_array`` with the image resident on the device: ``batch`` windows per
    ``WESUPPixelInference.forward_batch`` (mind its memory: ~3.6 GB per 464 x 464 window), class 1 of every window kept on
    the device, one ``ops.window_merge`` of the probabilities and one copy to the host (the caller rounds)."""
    def keep_class_1(kept, pred, first, valid):                           # pred (batch, p, p, C)
        kept[first:first + valid, :, :, 0].copy_(pred[:valid, :, :, 1])         # a strided device copy, no arithmetic
    kept, tops, lefts, H, W = _resident_windows(img, patch_size, batch, stain, device, model.forward_batch, (1,), keep_class_1,
                                                views=views)
    merged = ops.window_merge(kept, tops, lefts, H, W, round_first=False, views=views)
    return merged.view(H, W).cpu().numpy()


def predict_array_classes_batched(trainer, img, patch_size, batch=4, device='cuda', stain=None, views=None):
    """``predict_array_classes`` with the image resident on the device (``predict_array_batched`` for C > 2): the painted class
    indices of all windows kept in one (N, p, p) device buffer, one ``ops.window_merge_classes(votes=True)`` and ONE copy of the
    (H, W) uint8 map to the host.  Equal to ``predict_array_classes`` bit for bit at ``batch=1``."""
    def forward(x):
        input_, _ = trainer.preprocess(x)
        return trainer.model(input_)
    C = _n_classes(trainer.model)
    kept, tops, lefts, H, W = _resident_windows(img, patch_size, batch, stain, device, forward, (), views=views)
    merged, status = ops.window_merge_classes(kept, tops, lefts, H, W, n_classes=C, votes=True, views=views)
    merged = merged.cpu().numpy()
    _check_status(status, C, 'predict_array_classes_batched')            # (behind the copy: no wait of its own)
    return merged


def pixel_predict_array_classes_batched(model, img, patch_size, batch=2, device='cuda', stain=None, views=None):
    """``pixel_predict_array_classes`` with the image resident on the device: the (p, p, C) probabilities of every window kept on
    the device, one ``ops.window_merge_classes`` (the fp64 means per class live in registers: no (H, W, C) tensor) and one copy
    of the (H, W) uint8 map to the host."""
    def forward(x):
        return model.forward_batch(x).contiguous()                        # (batch, p, p, C)
    kept, tops, lefts, H, W = _resident_windows(img, patch_size, batch, stain, device, forward, (_n_classes(model),), views=views)
    merged, _ = ops.window_merge_classes(kept, tops, lefts, H, W, views=views)      # (probabilities: nothing comes in as an index)
    return merged.cpu().numpy()


def _form_kwargs(device, batch, stain, views=None):
    """The keywords of a form: ``batch`` only for the device-resident ones, ``stain`` and ``views`` only when there are any."""
    kw = {'device': device} if batch is None else {'batch': batch, 'device': device}
    if stain is not None:                                   # (--stain-normalize: fitted once per image, applied on the device)
        kw['stain'] = stain
    if views is not None:                                   # (--tta: every window under every view of the list)
        kw['views'] = check_views(views)
    return kw


def predict(trainer, img_path, patch_size, device='cuda', batch=None, stain=None, views=None):
    """One image file -> (H, W) map; ``batch=None`` is the per-window path, a number the device-resident one.  A model of more
    than two classes gives the uint8 class map of the ``_classes`` forms.  ``views``: a two-class map is the un-rounded mean
    over windows x views (``predict_array``)."""
    from PIL import Image
    img = np.asarray(Image.open(img_path).convert('RGB'))
    C = _n_classes(getattr(trainer, 'model', None))
    form = {(False, True): predict_array, (False, False): predict_array_batched,
            (True, True): predict_array_classes, (True, False): predict_array_classes_batched}[C > 2, batch is None]
    return form(trainer, img, patch_size, **_form_kwargs(device, batch, stain, views))


def save_predictions(predictions, img_paths, output_dir='predictions', n_classes=2):
    """One image per prediction.  Two classes: {0, 255} under the input's own name, as ever.  More: the class indices themselves
    as ``<stem>.png`` whatever the input is called (as ``infer.save_predictions``) -- under the name of a ``.jpg`` input a lossy
    format would blur the indices."""
    from PIL import Image
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    for pred, img_path in zip(predictions, img_paths):
        if n_classes == 2:
            Image.fromarray(pred.astype('uint8') * 255).save(output_dir / Path(img_path).name)
        else:
            Image.fromarray(pred.astype('uint8')).save(output_dir / Path(img_path).with_suffix('.png').name, format='PNG')


def infer(trainer, data_dir, patch_size, output_dir=None, device='cuda', batch=None, stain=None, views=None):
    """Window-based inference on ``data_dir/images`` (infer_tile.py:143-162).  Under ``views`` a two-class map is the mean of
    un-rounded probabilities and is rounded here, once (np.round: a tie at 0.5 goes to 0), as ``pixel_infer`` does."""
    trainer.model.eval()
    data_dir = Path(data_dir).expanduser()
    img_paths = sorted((data_dir / 'images').iterdir())
    kw = {k: v for k, v in (('stain', stain), ('views', views)) if v is not None}
    predictions = [predict(trainer, p, patch_size, device=device, batch=batch, **kw) for p in img_paths]
    if views is not None and _n_classes(trainer.model) == 2:
        predictions = [np.round(pred) for pred in predictions]
    if output_dir is not None:
        save_predictions(predictions, img_paths, output_dir, n_classes=_n_classes(trainer.model))
    return predictions


def pixel_infer(model, data_dir, patch_size, output_dir=None, device='cuda', batch=None, stain=None, views=None):
    """Pixel-wise window inference on ``data_dir/images`` (pixel_infer_tile.py:41-60): the merged class-1 probabilities are
    rounded here, before they are saved.  A model of more than two classes gives class maps."""
    from PIL import Image
    model.eval()
    data_dir = Path(data_dir).expanduser()
    img_paths = sorted((data_dir / 'images').iterdir())
    C = _n_classes(model)
    form = {(False, True): pixel_predict_array, (False, False): pixel_predict_array_batched,
            (True, True): pixel_predict_array_classes, (True, False): pixel_predict_array_classes_batched}[C > 2, batch is None]
    kw = _form_kwargs(device, batch, stain, views)
    predictions = []
    for path in img_paths:
        merged = form(model, np.asarray(Image.open(path).convert('RGB')), patch_size, **kw)
        predictions.append(merged if C > 2 else merged.round())
    if output_dir is not None:
        save_predictions(predictions, img_paths, output_dir, n_classes=C)
    return predictions


def _load_pixel_model(checkpoint, device, multiclass=False):
    """The pixel-wise model of a checkpoint.  A caller that reads the class-1 probability keeps ``multiclass=False``: a checkpoint
    of more than two classes is refused.  One that dispatches on ``model.n_classes`` (the command-line tools) passes ``True`` and
    gets the model with the checkpoint's class count.  ``checkpoint``: a path, or the dict ``torch.load`` made of one; a file is
    read once."""
    from .models.wesup import WESUPPixelInference
    n_classes = 2
    if checkpoint is not None:
        if not isinstance(checkpoint, dict):
            checkpoint = torch.load(checkpoint, map_location=device)
        if multiclass:
            from .models import checkpoint_n_classes
            n_classes = checkpoint_n_classes(checkpoint)
        else:
            from .models import require_two_class_checkpoint
            require_two_class_checkpoint(checkpoint, 'tile / pixel inference')
    model = WESUPPixelInference(n_classes=n_classes).to(device)
    if checkpoint is not None:
        model.load_state_dict(checkpoint['model_state_dict'])
    return model


def parse_args(argv=None):
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
    ap.add_argument('--tta', choices=sorted(VIEW_SETS), default='none',
                    help='test-time augmentation: every window under the views of this set (flips: upright, half turn and the two '
                         'mirrors; rot: the four quarter turns; d4: all eight), merged on the device with --batch; V times the '
                         'forward work')
    from .stain import add_argument
    add_argument(ap)
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    kw = {}
    if a.stain_normalize is not None:                # --stain-normalize [TARGET]: off by default, nothing of it is touched
        from .stain import make_normalizer
        kw['stain'] = make_normalizer(a.stain_normalize, a.device)
    if a.tta != 'none':                              # --tta: off by default, nothing of it is touched
        kw['views'] = VIEW_SETS[a.tta]
    output_dir = a.output_dir
    if output_dir is None and a.checkpoint is not None:
        output_dir = Path(a.checkpoint).expanduser().parent.parent / 'results'
    if a.pixel:
        if a.checkpoint is None:                     # (no checkpoint: no class count to read, the two-class default)
            model = _load_pixel_model(None, a.device)
        else:
            model = _load_pixel_model(a.checkpoint, a.device, multiclass=True)
        pixel_infer(model, a.data_dir, a.patch_size, output_dir, device=a.device, batch=a.batch, **kw)
        return
    if a.checkpoint is None:
        trainer = initialize_trainer(a.model_type, device=a.device)
    else:
        from .models import checkpoint_n_classes
        trainer = initialize_trainer(a.model_type, device=a.device, n_classes=checkpoint_n_classes(a.checkpoint))
        trainer.load_checkpoint(a.checkpoint)
    infer(trainer, a.data_dir, a.patch_size, output_dir, device=a.device, batch=a.batch, **kw)


if __name__ == '__main__':
    main()
