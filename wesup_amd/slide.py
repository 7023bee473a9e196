"""Whole-slide evaluation: the DP2019 patch pipeline (mirror of the reference's ``test_dp2019_pipeline.py``).

A slide of ``DATA_ROOT/images/*.jpg`` is cut into a lattice of zero-padded ``patch_size`` x ``patch_size`` patches, every patch
is predicted at ``input_size`` = (400, 400) by the superpixel model (``infer.py``) or, with ``--pixel``, at scale 0.4 by the
pixel-wise model (``pixel_infer.py``), the predictions are pasted into a slide-size map, cropped, written as PNG and scored
against ``DATA_ROOT/masks/*.png``: overall accuracy and Dice for the ``positive-*`` slides and, with both maps inverted, for
the others (``negative-*``).

    python -m wesup_amd.slide DATA_ROOT -c CKPT [--pixel] [-p 1000] [--skip-infer] [--batch N] [--post-threshold T] [--device D]
                              [--skip-background [FRAC]] [--tissue-channel luma|chroma] [--tissue-threshold otsu|INT]
                              [--tissue-masks DIR]

The slide is uploaded once as uint8 and comes back once as a uint8 map: per pass of ``batch`` patches
``ops.patch_gather_resize`` (cut + resize) -> the model -> ``ops.patch_scatter_u8`` (resize back + round + paste), nothing
in between waits for the device.

A checkpoint of more than two classes gives class maps: ``ops.patch_scatter_classes_u8`` pastes class indices,
the PNGs hold them as they are, and all slides are scored as one group against class-index masks from the C x C confusion table
(``slide_class_scores``; ``ops.label_confusion`` on the device).

Two deliberate deviations from the reference:

* **No extra patch at exact multiples.**  The reference cuts at ``range(0, size + 1, patch_size)``, which asks for one more,
  entirely empty patch when a side is an exact multiple of the patch size (width 128, patch 64: corners 0, 64 and 128); its own
  ``combine_single`` drops what such a patch predicts.  The lattice here is the ``ceil(size / patch_size)`` one that
  ``combine_single`` assumes.
* **No JPEG round trip.**  The reference writes the patches as JPEG and reads them back for inference; here they are cut from
  the decoded slide.  No ``-patches`` folder, no ``info.csv`` and no ``results-for-...`` folder are written.

The reference defines ``postprocess`` but never calls it; it is opt-in here (``--post-threshold``).

``--skip-background`` (no counterpart in the reference, off by default) puts a tissue decision in front of the
walk: one read of the resident slide gives per-patch histograms of a pixel value, Otsu's threshold over their sum says which
pixels are tissue, and only patches with enough of them are predicted; the others are background in the map.  The host
definitions (``pixel_value``, ``patch_histograms``, ``otsu_threshold``, ``select_patches``) are below, the kernels in
``csrc/tissue.hip`` equal them bit for bit."""
import argparse
import math
from pathlib import Path

import numpy as np
import torch

from . import ops
from .infer_tile import _check_status, _load_pixel_model, _n_classes, _upload, window_batches
from .pixel_infer import target_size

PATCH_SIZE = 1000              # test_dp2019_pipeline.py:122
INPUT_SIZE = (400, 400)        # test_dp2019_pipeline.py:152
PIXEL_SCALE = 0.4              # test_dp2019_pipeline.py:149


# ------------------------------------------------------------------------------------------------------ host functions
def patch_grid(height, width, patch_size):
    """``(n_h, n_w)`` of the patch lattice: ``ceil(size / patch_size)`` per axis; patch k (row-major) has its corner at
    ``(k // n_w * patch_size, k % n_w * patch_size)``.  Not the reference's ``range(0, size + 1, patch_size)``, which has
    one more (empty) patch at exact multiples (see the module docstring); a patch larger than the slide is one padded patch."""
    height, width, patch_size = int(height), int(width), int(patch_size)
    if height < 1 or width < 1 or patch_size < 1:
        raise ValueError(f'a {height} x {width} slide in patches of {patch_size}')
    return math.ceil(height / patch_size), math.ceil(width / patch_size)


def split_patches_array(img, patch_size):
    """(H, W[, C]) array -> (n_h * n_w, p, p[, C]) zero-padded patches in lattice order (``split`` of
    test_dp2019_pipeline.py:37-56 without the files): the host witness of ``ops.patch_gather_resize``."""
    img = np.asarray(img)
    p = int(patch_size)
    n_h, n_w = patch_grid(img.shape[0], img.shape[1], p)
    ext = np.zeros((n_h * p, n_w * p) + img.shape[2:], dtype=img.dtype)
    ext[:img.shape[0], :img.shape[1]] = img
    ext = ext.reshape((n_h, p, n_w, p) + img.shape[2:])
    return np.ascontiguousarray(np.swapaxes(ext, 1, 2)).reshape((n_h * n_w, p, p) + img.shape[2:])


def combine_single_array(patches, original_size):
    """(n_h * n_w, p, p) patch predictions in lattice order -> the (H, W) float64 map: pasted into the padded lattice and
    cropped (``combine_single``, test_dp2019_pipeline.py:158-172)."""
    patches = np.asarray(patches)
    height, width = original_size
    p = patches.shape[1]
    n_h, n_w = patch_grid(height, width, p)
    if patches.shape[0] != n_h * n_w or patches.shape[2] != p:
        raise ValueError(f'{patches.shape} patches for a {n_h} x {n_w} lattice of {p}')
    final = np.zeros((n_h * p, n_w * p))
    for k, patch in enumerate(patches):
        y, x = k // n_w * p, k % n_w * p
        final[y:y + p, x:x + p] = patch
    return final[:height, :width]


def accuracy(P, G):
    """test_dp2019_pipeline.py:74-75."""
    return (P == G).mean()


def dice(S, G, epsilon=1e-7):
    """test_dp2019_pipeline.py:78-81."""
    S, G = S > 0, G > 0
    return 2 * (G * S).sum() / (G.sum() + S.sum() + epsilon)


def postprocess(pred, threshold=1000, device=None):
    """test_dp2019_pipeline.py:84-97 on a {0, 255} map: 8-connected foreground regions smaller than ``threshold`` pixels become
    0, then background regions of the result smaller than ``threshold`` become 255.  That is ``evaluate.remove_small_regions``
    (its loop over region 0, the other class as a whole, writes the value those pixels already have); with ``device`` it is
    ``wesup_remove_small_regions`` there.  Returns a new array of ``pred``'s dtype (the reference rewrites its argument)."""
    from .evaluate import remove_small_regions
    pred = np.asarray(pred)
    return (remove_small_regions(pred, threshold, device) * 255).astype(pred.dtype)


def _log_means(scores, log):
    """The mean accuracy and the mean Dice of per-slide ``(accuracy, dice)`` pairs, as floats, behind the reference's two lines."""
    acc, dsc = np.mean([s[0] for s in scores]), np.mean([s[1] for s in scores])
    log('Accuracy:', acc)
    log('Dice:', dsc)
    return float(acc), float(dsc)


def compute_metrics(predictions, gts, negative=False, log=print, device=None):
    """test_dp2019_pipeline.py:100-111: the mean overall accuracy and the mean Dice of the pairs, both maps inverted first with
    ``negative``; prints the reference's two lines and returns the two numbers."""
    return _log_means([slide_scores(pred, gt, negative, device) for pred, gt in zip(predictions, gts)], log)


# ------------------------------------------------------------------------------- tissue selection: the host definitions
# DESIGN.md 3.19.  Plain numpy and Python ints; csrc/tissue.hip equals every one of them bit for bit.
TISSUE_CHANNELS = ('luma', 'chroma')
SKIP_MIN_FRACTION = 0.01       # the interface's default for ``min_fraction``: a round number, not a measured optimum


def pixel_value(img, channel='luma'):
    """(H, W, 3) uint8 -> (H, W) uint8, the value the tissue decision looks at: ``luma`` (77 R + 150 G + 29 B + 128) >> 8 (tissue is
    darker than glass), ``chroma`` max(R, G, B) - min(R, G, B) (tissue is more coloured than glass)."""
    if channel not in TISSUE_CHANNELS:
        raise ValueError(f'channel {channel!r}, expected one of {TISSUE_CHANNELS}')
    a = np.asarray(img).astype(np.int64)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f'expected an (H, W, 3) image, got {a.shape}')
    if channel == 'luma':
        return ((77 * a[..., 0] + 150 * a[..., 1] + 29 * a[..., 2] + 128) >> 8).astype(np.uint8)
    return (a.max(axis=2) - a.min(axis=2)).astype(np.uint8)


def patch_areas(height, width, patch_size):
    """(n,) int64: the pixels of every patch of the lattice that lie inside the slide (a border patch has fewer than p * p)."""
    p = int(patch_size)
    n_h, n_w = patch_grid(height, width, p)
    hs = np.minimum((np.arange(n_h) + 1) * p, int(height)) - np.arange(n_h) * p
    ws = np.minimum((np.arange(n_w) + 1) * p, int(width)) - np.arange(n_w) * p
    return (hs[:, None] * ws[None, :]).reshape(-1).astype(np.int64)


def patch_histograms(img, patch_size, channel='luma'):
    """(n, 256) int64: ``hist[k][v]`` = the slide pixels of patch ``k`` whose ``pixel_value`` is ``v``.  Only pixels inside the
    slide are counted, never the zero padding: a row sums to ``patch_areas``."""
    v = pixel_value(img, channel)
    p = int(patch_size)
    n_h, n_w = patch_grid(v.shape[0], v.shape[1], p)
    hist = np.zeros((n_h * n_w, 256), dtype=np.int64)
    for k in range(n_h * n_w):
        y, x = k // n_w * p, k % n_w * p
        hist[k] = np.bincount(v[y:y + p, x:x + p].reshape(-1), minlength=256)
    return hist


def otsu_threshold(total):
    """Otsu's threshold of a 256-bin histogram, stated so that a device can repeat it bit for bit.  With N = sum h and
    S = sum i h_i, for t = 0 .. 254 ascending: w0 = sum_{i <= t} h_i, s0 = sum_{i <= t} i h_i, D = w0 (N - w0); a t with D = 0 is
    skipped; num = |S w0 - s0 N| exactly (Python ints), x = float(num >> 64) * 2^64 + float(num mod 2^64), q = x * x / float(D) --
    six fp64 operations, none contracted.  Returns the first t whose q is the largest under a strict >, or -1 when no t has
    D > 0 (a one-level histogram).  q is the between-class variance times N^2, so this is the usual argmax; two levels give the
    lower one (every t between them scores the same, the first wins).  Where rounding makes it differ from the exact rational
    argmax, this statement is the definition (tests/test_tissue_cpu.py checks 300 seeded histograms: no difference)."""
    h = [int(v) for v in np.asarray(total).reshape(-1)]
    if len(h) != 256 or min(h) < 0:
        raise ValueError('expected 256 non-negative counts')
    N, S = sum(h), sum(i * v for i, v in enumerate(h))
    best, best_q, w0, s0 = -1, 0.0, 0, 0
    for t in range(255):
        w0 += h[t]
        s0 += t * h[t]
        D = w0 * (N - w0)
        if D == 0:
            continue
        num = abs(S * w0 - s0 * N)
        x = float(num >> 64) * 18446744073709551616.0 + float(num & ((1 << 64) - 1))
        q = x * x / float(D)
        if best < 0 or q > best_q:
            best, best_q = t, q
    return best


def tissue_counts(hist, t, channel='luma'):
    """(n,) int64 tissue pixels per patch from its histogram: ``luma`` v <= t, ``chroma`` v > t, ``t = -1`` every pixel."""
    hist = np.asarray(hist, dtype=np.int64)
    t = int(t)
    if channel not in TISSUE_CHANNELS:
        raise ValueError(f'channel {channel!r}, expected one of {TISSUE_CHANNELS}')
    if t < 0:
        return hist.sum(axis=1)
    return hist[:, :t + 1].sum(axis=1) if channel == 'luma' else hist[:, t + 1:].sum(axis=1)


def min_ppm_of(min_fraction):
    ppm = int(round(float(min_fraction) * 1e6))
    if not 0 <= ppm <= 1000000:
        raise ValueError(f'min_fraction {min_fraction} outside [0, 1]')
    return ppm


def select_patches(counts, areas, min_ppm, flat=False):
    """The kept patches in ascending order: ``count_k >= 1`` and ``count_k * 10^6 >= min_ppm * area_k`` in integers; every patch
    when ``flat`` (t = -1: a slide of one level is never skipped)."""
    min_ppm = int(min_ppm)
    if not 0 <= min_ppm <= 1000000:
        raise ValueError(f'min_ppm {min_ppm} outside [0, 10^6]')
    counts, areas = [int(c) for c in counts], [int(a) for a in areas]
    if len(counts) != len(areas):
        raise ValueError(f'{len(counts)} counts for {len(areas)} patches')
    return [k for k, (c, a) in enumerate(zip(counts, areas)) if flat or (c >= 1 and c * 1000000 >= min_ppm * a)]


def tissue_mask_array(img, t, channel='luma'):
    """(H, W) uint8 host mask: 255 where the pixel is tissue under threshold ``t``, 0 elsewhere."""
    v = pixel_value(img, channel)
    tissue = np.ones(v.shape, bool) if int(t) < 0 else (v <= int(t) if channel == 'luma' else v > int(t))
    return (tissue * 255).astype(np.uint8)


class TissuePatches:
    """What ``tissue_patches`` found: ``t`` the threshold (-1: a flat slide), ``n_keep`` of ``n`` patches kept, ``list`` their
    indices in ascending order (an int32 device tensor of length ``n_keep`` on the device, a Python list on the host),
    ``counts`` the tissue pixels per patch (a device tensor of uint32 bits, or an int64 array), ``flat``, and on the device
    ``info``, the (8,) int32 block ``ops.tissue_mask`` reads ``t`` from."""

    def __init__(self, t, n_keep, n, list, counts, flat, channel, info=None):
        self.t, self.n_keep, self.n, self.list, self.counts, self.flat = int(t), int(n_keep), int(n), list, counts, bool(flat)
        self.channel, self.info = channel, info

    def __repr__(self):
        return f'TissuePatches(t={self.t}, kept {self.n_keep} of {self.n}, channel={self.channel!r})'


def _threshold_arg(threshold):
    """``'otsu'`` (or None) -> -1, an int 0 .. 254 -> itself."""
    if threshold is None or threshold == 'otsu':
        return -1
    t = int(threshold)
    if not 0 <= t <= 254:
        raise ValueError(f'threshold {threshold!r}: "otsu" or an int in 0 .. 254')
    return t


def tissue_patches(img, p, channel='luma', threshold='otsu', min_fraction=SKIP_MIN_FRACTION, device=None):
    """Which patches of a slide's lattice hold tissue -> ``TissuePatches``.  A pixel is tissue when its
    ``pixel_value`` is on the tissue side of ``threshold`` (``'otsu'`` over the whole slide's histogram, or an int 0 .. 254); a
    patch is kept when at least one and at least ``min_fraction`` (rounded to ppm) of its in-slide pixels are tissue.  The
    default ``min_fraction`` is an interface default, not a measured optimum.

    Without a device (and for a host array) the host definitions of this module run.  With ``device``, or for a slide that is a
    device tensor already, ``ops.patch_value_hist`` reads the slide once and ``ops.tissue_select`` does the rest there; then ONE
    32-byte copy of ``info`` to the host tells ``n_keep``, which sizes the passes of the walk.  That copy is the only wait for the
    device the selection adds per slide."""
    if channel not in TISSUE_CHANNELS:
        raise ValueError(f'channel {channel!r}, expected one of {TISSUE_CHANNELS}')
    given, min_ppm, p = _threshold_arg(threshold), min_ppm_of(min_fraction), int(p)
    on_device = isinstance(img, torch.Tensor) and img.is_cuda
    if device is None and not on_device:
        img = img.numpy() if isinstance(img, torch.Tensor) else np.asarray(img)
        hist = patch_histograms(img, p, channel)
        t = otsu_threshold(hist.sum(axis=0)) if given < 0 else given
        counts = tissue_counts(hist, t, channel)
        kept = select_patches(counts, patch_areas(img.shape[0], img.shape[1], p), min_ppm, flat=t < 0)
        return TissuePatches(t, len(kept), len(counts), kept, counts, t < 0, channel)
    img_d = _resident(img, device)
    H, W = img_d.shape[:2]
    hist = ops.patch_value_hist(img_d, p, channel)
    info, _, counts, plist = ops.tissue_select(hist, H, W, p, channel, given, min_ppm)
    t, n_keep, n, flat = info.cpu().tolist()[:4]                   # the one read-back: 32 bytes
    return TissuePatches(t, n_keep, n, plist[:n_keep], counts, flat, channel, info)


# ------------------------------------------------------------------------------------------------ device-resident path
def _resident(img_u8, device, stain=None):
    """``stain`` (wesup_amd.stain.StainNormalizer): one strided fit of the whole slide and one pass over it, in place on the
    uploaded tensor (a tensor the caller owns is normalised into a copy); an invalid fit -- empty glass, the near-white
    ``negative-*`` slides -- leaves the slide as it is."""
    if isinstance(img_u8, torch.Tensor) and img_u8.is_cuda:
        return img_u8 if stain is None else stain(img_u8)
    return _upload(img_u8, device, stain)


def _selection(img_d, p, skip_background):
    """``skip_background`` of the two predict functions -> the ``TissuePatches`` of the resident slide (as the gather will read
    it: after ``stain``), or None: ``None`` / ``False`` no selection, ``True`` the defaults, a dict the parameters of
    ``tissue_patches`` (``channel``, ``threshold``, ``min_fraction``)."""
    if skip_background is None or skip_background is False:
        return None
    if isinstance(skip_background, TissuePatches):
        return skip_background
    kw = {} if skip_background is True else dict(skip_background)
    unknown = set(kw) - {'channel', 'threshold', 'min_fraction'}
    if unknown:
        raise ValueError(f'skip_background: unknown parameters {sorted(unknown)}')
    return tissue_patches(img_d, p, **kw)


def _patch_walk(img_d, p, size, batch, keep_on_device, align_corners, forward, paste, select=None):
    """The walk over the patches of a resident slide: the lattice, per pass of ``batch`` patches ``ops.patch_gather_resize`` to
    ``size`` into one reused input -> ``forward(x)`` -> ``paste(the predictions of the pass's valid patches, out, first)`` into the
    (H, W) uint8 map; nothing in it waits for the device.  Returns the map on the host, or the device tensor with
    ``keep_on_device``.

    ``select`` (a ``TissuePatches`` of this slide): the map starts as zeros, the passes are ``window_batches(n_keep, batch)`` over
    ``select.list`` -- slot ``first + i`` of a pass is patch ``list[first + i]``, a ragged last pass repeats the last listed
    patch -- and ``paste`` gets the list as its fourth argument.  With nothing kept the zero map is returned and ``forward`` is
    never called."""
    h, w = size
    H, W = img_d.shape[:2]
    n_h, n_w = patch_grid(H, W, p)
    if select is not None:
        if select.n != n_h * n_w:
            raise ValueError(f'a selection over {select.n} patches for a {n_h} x {n_w} lattice')
        out = torch.zeros(H, W, dtype=torch.uint8, device=img_d.device)        # skipped patches: background, class 0
        if select.n_keep == 0:
            return out if keep_on_device else out.cpu().numpy()
        passes, batch = window_batches(select.n_keep, batch)
        extra = {'patch_list': select.list}
    else:
        passes, batch = window_batches(n_h * n_w, batch)
        out = torch.empty(H, W, dtype=torch.uint8, device=img_d.device)        # (the lattice covers every pixel)
        extra = {}
    x = torch.empty(batch, 3, h, w, dtype=torch.float32, device=img_d.device)
    with torch.no_grad():
        for first, valid in passes:
            ops.patch_gather_resize(img_d, p, h, w, first, batch, align_corners=align_corners, out=x, **extra)
            paste(forward(x)[:valid], out, first, **extra)
    return out if keep_on_device else out.cpu().numpy()


def slide_predict(trainer, img_u8, patch_size=PATCH_SIZE, input_size=INPUT_SIZE, batch=4, device='cuda', keep_on_device=False,
                  stain=None, skip_background=None):
    """Superpixel prediction of a whole (H, W, 3) uint8 slide -> (H, W) uint8 map in {0, 255}: what the reference gets from
    ``split_patches`` -> ``infer(input_size=...)`` -> ``combine_single``, with the slide resident on the device.  One upload;
    per pass of ``batch`` patches ``ops.patch_gather_resize`` -> ``trainer.preprocess`` (batched GPU SLIC) -> ``trainer.model``
    -> ``ops.patch_scatter_u8`` (round, nearest resize to the patch, paste, crop); one copy back, or the device tensor with
    ``keep_on_device``.  At ``batch=1`` equal to the per-patch path bit for bit; at another batch size the convolutions tile
    differently and a pixel whose probability sits at 0.5 can turn (tests/test_slide_gpu.py).  A model of more than two classes
    gives the (H, W) uint8 map of class indices (``ops.patch_scatter_classes_u8``).

    ``skip_background`` (``True``, or a dict of ``tissue_patches``' ``channel`` / ``threshold`` / ``min_fraction``; DESIGN.md
    3.19): the tissue patches of the resident slide -- after ``stain`` -- are found on the device and only they are predicted;
    a skipped patch is 0 in the map (background, class 0).  One 32-byte read-back per slide.  Off by default."""
    p = int(patch_size)
    size = tuple(int(s) for s in input_size)
    img_d = _resident(img_u8, device, stain)
    select = _selection(img_d, p, skip_background)
    C = _n_classes(trainer.model)

    def forward(x):
        input_, _ = trainer.preprocess(x)
        return trainer.model(input_)
    if C > 2:                                        # the painted class indices, pasted as they are
        status = torch.zeros(1, dtype=torch.int32, device=img_d.device)

        def paste(pred, out, first, **kw):
            ops.patch_scatter_classes_u8(pred, out, p, first, n_classes=C, mode=0, status=status, **kw)
    else:
        def paste(pred, out, first, **kw):
            ops.patch_scatter_u8(pred, out, p, first, mode=0, **kw)
    result = _patch_walk(img_d, p, size, batch, keep_on_device, False, forward, paste, select)
    if C > 2:                                        # one word over all passes, read once, behind the map
        _check_status(status, C, 'slide_predict')
    return result


def slide_pixel_predict(model, img_u8, patch_size=PATCH_SIZE, scale=PIXEL_SCALE, batch=2, device='cuda', keep_on_device=False,
                        stain=None, skip_background=None):
    """Pixel-wise prediction of a whole slide -> (H, W) uint8 map in {0, 255}: ``pixel_infer`` with ``scales=(scale,)`` on every
    zero-padded patch, pasted and cropped.  Per pass ``ops.patch_gather_resize(align_corners=True)`` to
    ``pixel_infer.target_size`` -> ``model.forward_per_resolution`` -> ``ops.patch_scatter_u8`` reading class 1 in place
    (bilinear back to the patch, round, paste).  A model of more than two classes gives the map of class indices: all C
    planes bilinear back to the patch, the first maximum pasted (``ops.patch_scatter_classes_u8``).  ``skip_background``: as
    in ``slide_predict``."""
    p = int(patch_size)
    size = target_size(p, p, scale)
    if min(size) < 1:
        raise ValueError(f'scale {scale} leaves nothing of a {p} x {p} patch')
    img_d = _resident(img_u8, device, stain)
    select = _selection(img_d, p, skip_background)
    if _n_classes(model) > 2:                        # all C planes resized back, the first maximum pasted
        # (mode 1 takes probabilities: nothing comes in as an index and the word is never set -- one for all passes, not read)
        status = torch.zeros(1, dtype=torch.int32, device=img_d.device)

        def paste(probs, out, first, **kw):          # probs (valid, h, w, C)
            ops.patch_scatter_classes_u8(probs, out, p, first, mode=1, status=status, **kw)
    else:
        def paste(probs, out, first, **kw):
            ops.patch_scatter_u8(probs[:, :, :, 1], out, p, first, mode=1, **kw)
    return _patch_walk(img_d, p, size, batch, keep_on_device, True, model.forward_per_resolution, paste, select)


def _resident_u8(a, device):
    """A map for the scores on ``device``: a tensor moved there, anything else uploaded as uint8."""
    if isinstance(a, torch.Tensor):
        return a.to(device).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.uint8, copy=False))).to(device)


def slide_class_scores(pred, gt, n_classes, device=None):
    """``(accuracy, dice)`` of two uint8 class-index maps as Python floats, by the definitions of DESIGN.md 3.12: the trace of
    the confusion table over the pixels, and the mean over the classes present in either map of 2 n_cc / (row_c + col_c + eps)
    (``utils.metrics.accuracy_from_confusion`` / ``dice_from_confusion``).  With ``device`` (or for maps that are device tensors
    already) the table is ``ops.label_confusion``'s, otherwise ``utils.metrics.confusion``'s: integers either way, the same
    numbers.  A class index outside [0, n_classes) is an error on both paths."""
    from .utils import metrics as M
    C = int(n_classes)
    on_device = isinstance(pred, torch.Tensor) and pred.is_cuda
    if device is None and not on_device:
        conf = M.confusion(pred.cpu() if isinstance(pred, torch.Tensor) else pred, gt.cpu() if isinstance(gt, torch.Tensor) else gt, C)
    else:
        device = pred.device if on_device else device
        table, status = ops.label_confusion(_resident_u8(pred, device), _resident_u8(gt, device), C)
        conf = table.cpu().numpy()
        if int(status.cpu()) != 0:
            raise ValueError(f'class index outside [0, {C})')
    return M.accuracy_from_confusion(conf), M.dice_from_confusion(conf)


def slide_scores(pred_u8, gt_u8, negative=False, device=None):
    """``(accuracy, dice)`` of two uint8 maps as Python floats, both inverted first with ``negative``.  With ``device`` (or for
    maps that are device tensors already) the four pixel counts come from ``ops.mask_scores`` and the two float64 formulas of
    ``accuracy`` / ``dice`` are applied to them on the host: the same numbers as numpy's."""
    on_device = isinstance(pred_u8, torch.Tensor) and pred_u8.is_cuda
    if device is None and not on_device:
        P, G = np.asarray(pred_u8), np.asarray(gt_u8.cpu() if isinstance(gt_u8, torch.Tensor) else gt_u8)
        if negative:
            P, G = 255 - P, 255 - G
        return float(accuracy(P, G)), float(dice(P, G))
    device = pred_u8.device if on_device else device
    P, G = _resident_u8(pred_u8, device), _resident_u8(gt_u8, device)
    eq, inter, sum_s, sum_g = (int(v) for v in ops.mask_scores(P, G, negative).cpu().tolist())
    return eq / P.numel(), 2 * inter / (sum_g + sum_s + 1e-7)


# ------------------------------------------------------------------------------------------------------------- driver
def output_dir_for(checkpoint, pixel=False):
    """``combined-results[-pixel]-for-<checkpoint name>`` beside the checkpoint's parent directory
    (test_dp2019_pipeline.py:136-137,154-155)."""
    ckpt = Path(checkpoint).expanduser()
    return ckpt.parent.parent / (f'combined-results-pixel-for-{ckpt.name}' if pixel else f'combined-results-for-{ckpt.name}')


def split_stems(paths):
    """The two groups the reference scores (test_dp2019_pipeline.py:203-219): ``positive-*`` and ``negative-*``, each sorted."""
    paths = sorted(Path(p) for p in paths)
    return ([p for p in paths if p.name.startswith('positive-')], [p for p in paths if p.name.startswith('negative-')])


def _read_gray(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert('L'))


def _read_classes(path):
    """A class-index PNG as it is stored: the bytes of a grey ('L') image, the palette INDICES of a palette ('P') one, which is how
    label masks are often written -- ``convert('L')`` would turn those into the luminance of their colours."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im if im.mode in ('L', 'P') else im.convert('L'))


def score_directory(output_dir, gt_dir, log=print, device=None, n_classes=2):
    """The scoring half of the reference (test_dp2019_pipeline.py:197-219) on the combined PNGs of ``output_dir`` against the
    masks of ``gt_dir``.  Returns ``{'positive': (accuracy, dice), 'negative': (accuracy, dice)}`` (a group without slides is
    left out).

    With ``n_classes > 2`` the PNGs and the masks are class-index maps and ALL of them are scored as one group: the inversion
    that tells the negative slides from the positive ones swaps foreground and background, which has no meaning for class
    indices.  A prediction is scored against the mask of its own stem.  Returns ``{'all': (accuracy, dice)}``, the means of
    ``slide_class_scores`` over the slides."""
    if int(n_classes) > 2:
        preds, gts = sorted(Path(output_dir).glob('*.png')), sorted(Path(gt_dir).glob('*.png'))
        log('\nEvaluating OA and Dice ...')
        if [p.stem for p in preds] != [g.stem for g in gts]:
            raise ValueError(f'predictions {[p.stem for p in preds]} in {output_dir} but masks {[g.stem for g in gts]} in {gt_dir}')
        if not preds:
            return {}
        scores = [slide_class_scores(_read_classes(p), _read_classes(g), n_classes, device) for p, g in zip(preds, gts)]
        return {'all': _log_means(scores, log)}
    pos_pred, neg_pred = split_stems(Path(output_dir).glob('*.png'))
    pos_gt, neg_gt = split_stems(Path(gt_dir).glob('*.png'))
    result = {}
    for name, preds, gts, negative in (('positive', pos_pred, pos_gt, False), ('negative', neg_pred, neg_gt, True)):
        log(f'\nEvaluating {name} OA and Dice ...')
        if len(preds) != len(gts):
            raise ValueError(f'{len(preds)} {name} predictions in {output_dir} but {len(gts)} masks in {gt_dir}')
        if preds:
            result[name] = compute_metrics([_read_gray(p) for p in preds], [_read_gray(p) for p in gts], negative, log, device)
    return result


def main(data_root, checkpoint, model_type='wesup', pixel=False, patch_size=PATCH_SIZE, skip_infer=False, device=None, batch=None,
         post_threshold=None, log=print, stain_normalize=None, skip_background=None, tissue_masks=None, geojson=None,
         measure=None, simplify=None):
    """test_dp2019_pipeline.py:114-219 without its patch files: predict every slide of ``data_root/images/*.jpg`` (unless
    ``skip_infer``), write the combined PNGs, score them against ``data_root/masks``.  Returns ``score_directory``'s result.

    The class count is the checkpoint's.  For more than two classes the PNGs hold class indices, the masks are read as class
    indices and ``post_threshold`` (a clean-up of binary maps) is refused.  Under ``skip_infer`` the checkpoint only names the
    output directory and need not exist: without the file the PNGs on disk are scored as two-class maps.

    ``skip_background`` (``True`` or a dict of ``tissue_patches``' parameters): only the tissue patches of a slide
    are predicted, the others are 0 in its map; one log line per slide tells the threshold and how many patches were kept.
    ``tissue_masks``: a directory that gets every slide's tissue mask (255 tissue, 0 glass) as ``<stem>.png``; needs
    ``skip_background``.
    ``geojson``: a directory that gets the outlines of every combined map as ``<stem>.geojson``: the objects of
    the binary map as it is written (after ``post_threshold``), for more than two classes the objects of every class.
    ``measure``: a directory that gets the measurements of the same objects as ``<stem>.csv``, one row per object (DESIGN.md
    3.22).
    ``simplify``: the outlines of ``geojson`` are simplified within that many pixels; one log line per slide tells
    the vertex counts, the flagged rings and the pixels that change when the simplified polygons are filled back."""
    from PIL import Image
    data_root = Path(data_root).expanduser()
    output_dir = output_dir_for(checkpoint, pixel)
    output_dir.mkdir(parents=True, exist_ok=True)
    if device is None:
        device = 'cuda'
    C, loaded = 2, None
    if not skip_infer or Path(checkpoint).expanduser().is_file():
        from .models import checkpoint_n_classes
        loaded = torch.load(Path(checkpoint).expanduser(), map_location='cpu')      # read once: the class count, the pixel model
        C = checkpoint_n_classes(loaded)
    if C > 2 and post_threshold is not None:
        raise ValueError('--post-threshold removes small regions of a binary map: undefined for class indices')
    skipping = skip_background not in (None, False)
    if tissue_masks is not None and not skipping:
        raise ValueError('--tissue-masks writes the masks of --skip-background')
    if simplify is not None and geojson is None:
        raise ValueError('--simplify is the tolerance of the outlines that --geojson writes')
    if not skip_infer:
        log('\nMaking inference ...')
        if pixel:
            if model_type != 'wesup':
                raise ValueError('--pixel is the wesup model\'s pixel-wise inference')
            model = _load_pixel_model(loaded, device, multiclass=True)
            model.eval()
        else:
            from .models import initialize_trainer
            trainer = initialize_trainer(model_type, device=device, n_classes=C)
            trainer.load_checkpoint(checkpoint)
            trainer.model.eval()
        kw = {}
        if stain_normalize not in (None, False):               # --stain-normalize [TARGET]: off by default
            from .stain import make_normalizer
            kw['stain'] = make_normalizer(stain_normalize, device)
        stain = kw.get('stain')
        for path in sorted((data_root / 'images').glob('*.jpg')):
            img = np.asarray(Image.open(path).convert('RGB'))
            if skipping:                                       # select on the slide as the gather reads it: after the stain
                img = _resident(img, device, stain)
                sel = _selection(img, int(patch_size), skip_background)
                kw = {'skip_background': sel}                  # (the resident slide is stained already)
                log(f'{path.stem}: tissue threshold {sel.t} ({sel.channel}), {sel.n_keep} of {sel.n} patches kept')
                if tissue_masks is not None:
                    Path(tissue_masks).mkdir(parents=True, exist_ok=True)
                    mask = ops.tissue_mask(img, sel.info, sel.channel).cpu().numpy()
                    Image.fromarray(mask).save(Path(tissue_masks) / f'{path.stem}.png', format='PNG')
            if pixel:
                combined = slide_pixel_predict(model, img, patch_size, PIXEL_SCALE, batch=batch or 2, device=device, **kw)
            else:
                combined = slide_predict(trainer, img, patch_size, INPUT_SIZE, batch=batch or 4, device=device, **kw)
            if post_threshold is not None:
                combined = postprocess(combined, post_threshold, device)
            Image.fromarray(combined).save(output_dir / f'{path.stem}.png', format='PNG')
            if geojson is not None:
                from . import contour
                if simplify is None:
                    polys = (contour.classmap_polygons(combined, C, device) if C > 2 else contour.mask_polygons(combined, device))
                else:
                    stats = {}
                    polys = (contour.classmap_polygons(combined, C, device, simplify=simplify, stats=stats) if C > 2 else
                             contour.mask_polygons(combined, device, simplify=simplify, stats=stats))
                    log(f'{path.stem}: ' + contour.simplify_log(stats, simplify))
                contour.write_geojson(Path(geojson).expanduser() / f'{path.stem}.geojson', polys)
            if measure is not None:
                from . import measure as measure_mod
                rows = []
                for k in (range(1, C) if C > 2 else (0,)):
                    inst = measure_mod._instances(combined == k if C > 2 else combined, device)
                    rows += measure_mod.object_rows(inst, f'{path.stem}.png', device, k)[0]
                measure_mod.write_csv(Path(measure).expanduser() / f'{path.stem}.csv', rows)
        log(f'Combined results saved to {output_dir}.')
    return score_directory(output_dir, data_root / 'masks', log, device if not skip_infer else None, n_classes=C)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('data_root')
    ap.add_argument('-m', '--model', choices=['wesup'], default='wesup')
    ap.add_argument('--pixel', action='store_true', default=False)
    ap.add_argument('--skip-infer', action='store_true', default=False, help='score the combined PNGs already on disk')
    ap.add_argument('-p', '--patch-size', type=int, default=PATCH_SIZE)
    ap.add_argument('-c', '--checkpoint', required=True, help='Path to checkpoint')
    ap.add_argument('--device', default=None, help='Device to use')
    ap.add_argument('--batch', type=int, default=None, help='patches per pass (default: 4, with --pixel 2)')
    ap.add_argument('--post-threshold', type=int, default=None,
                    help='remove regions and fill holes smaller than this many pixels (the reference never does)')
    ap.add_argument('--skip-background', nargs='?', type=float, const=SKIP_MIN_FRACTION, default=None, metavar='FRAC',
                    help='predict only patches of which at least FRAC of the pixels are tissue, the others are background '
                         f'(default FRAC {SKIP_MIN_FRACTION}: an interface default, not a measured optimum)')
    ap.add_argument('--tissue-channel', choices=TISSUE_CHANNELS, default='luma', help='the pixel value of the tissue decision')
    ap.add_argument('--tissue-threshold', default='otsu', metavar='otsu|INT',
                    help="the tissue threshold: Otsu's over the slide (default) or a value in 0 .. 254")
    ap.add_argument('--tissue-masks', default=None, metavar='DIR', help='write the tissue mask PNGs here (with --skip-background)')
    ap.add_argument('--geojson', default=None, metavar='DIR', help='write the outlines of every combined map here as <stem>.geojson')
    ap.add_argument('--measure', default=None, metavar='DIR', help='write the measurements of the objects of every combined map here as <stem>.csv')
    ap.add_argument('--simplify', type=float, default=None, metavar='PX', help='simplify the outlines of --geojson within this many pixels')
    from .stain import add_argument
    add_argument(ap)
    return ap.parse_args(argv)


def cli(argv=None):
    a = parse_args(argv)
    extra = {}
    if a.skip_background is not None:
        extra['skip_background'] = {'min_fraction': a.skip_background, 'channel': a.tissue_channel,
                                    'threshold': a.tissue_threshold if a.tissue_threshold == 'otsu' else int(a.tissue_threshold)}
    if a.tissue_masks is not None:
        extra['tissue_masks'] = a.tissue_masks
    if a.geojson is not None:
        extra['geojson'] = a.geojson
    if a.measure is not None:
        extra['measure'] = a.measure
    if a.simplify is not None:
        extra['simplify'] = a.simplify
    return main(a.data_root, a.checkpoint, model_type=a.model, pixel=a.pixel, patch_size=a.patch_size, skip_infer=a.skip_infer,
                device=a.device, batch=a.batch, post_threshold=a.post_threshold, **extra,
                **({} if a.stain_normalize is None else {'stain_normalize': a.stain_normalize}))


if __name__ == '__main__':
    cli()
