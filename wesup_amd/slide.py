"""Whole-slide evaluation: the DP2019 patch pipeline (mirror of the reference's ``test_dp2019_pipeline.py``).

A slide of ``DATA_ROOT/images/*.jpg`` is cut into a lattice of zero-padded ``patch_size`` x ``patch_size`` patches, every patch
is predicted at ``input_size`` = (400, 400) by the superpixel model (``infer.py``) or, with ``--pixel``, at scale 0.4 by the
pixel-wise model (``pixel_infer.py``), the predictions are pasted into a slide-size map, cropped, written as PNG and scored
against ``DATA_ROOT/masks/*.png``: overall accuracy and Dice for the ``positive-*`` slides and, with both maps inverted, for
the others (``negative-*``).

    python -m wesup_amd.slide DATA_ROOT -c CKPT [--pixel] [-p 1000] [--skip-infer] [--batch N] [--post-threshold T] [--device D]

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

The reference defines ``postprocess`` but never calls it; it is opt-in here (``--post-threshold``)."""
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


# ------------------------------------------------------------------------------------------------ device-resident path
def _resident(img_u8, device, stain=None):
    """``stain`` (wesup_amd.stain.StainNormalizer): one strided fit of the whole slide and one pass over it, in place on the
    uploaded tensor (a tensor the caller owns is normalised into a copy); an invalid fit -- empty glass, the near-white
    ``negative-*`` slides -- leaves the slide as it is."""
    if isinstance(img_u8, torch.Tensor) and img_u8.is_cuda:
        return img_u8 if stain is None else stain(img_u8)
    return _upload(img_u8, device, stain)


def _patch_walk(img_d, p, size, batch, keep_on_device, align_corners, forward, paste):
    """The walk over the patches of a resident slide: the lattice, per pass of ``batch`` patches ``ops.patch_gather_resize`` to
    ``size`` into one reused input -> ``forward(x)`` -> ``paste(the predictions of the pass's valid patches, out, first)`` into the
    (H, W) uint8 map; nothing in it waits for the device.  Returns the map on the host, or the device tensor with
    ``keep_on_device``."""
    h, w = size
    H, W = img_d.shape[:2]
    n_h, n_w = patch_grid(H, W, p)
    passes, batch = window_batches(n_h * n_w, batch)
    out = torch.empty(H, W, dtype=torch.uint8, device=img_d.device)            # (the lattice covers every pixel)
    x = torch.empty(batch, 3, h, w, dtype=torch.float32, device=img_d.device)
    with torch.no_grad():
        for first, valid in passes:
            ops.patch_gather_resize(img_d, p, h, w, first, batch, align_corners=align_corners, out=x)
            paste(forward(x)[:valid], out, first)
    return out if keep_on_device else out.cpu().numpy()


def slide_predict(trainer, img_u8, patch_size=PATCH_SIZE, input_size=INPUT_SIZE, batch=4, device='cuda', keep_on_device=False,
                  stain=None):
    """Superpixel prediction of a whole (H, W, 3) uint8 slide -> (H, W) uint8 map in {0, 255}: what the reference gets from
    ``split_patches`` -> ``infer(input_size=...)`` -> ``combine_single``, with the slide resident on the device.  One upload;
    per pass of ``batch`` patches ``ops.patch_gather_resize`` -> ``trainer.preprocess`` (batched GPU SLIC) -> ``trainer.model``
    -> ``ops.patch_scatter_u8`` (round, nearest resize to the patch, paste, crop); one copy back, or the device tensor with
    ``keep_on_device``.  At ``batch=1`` equal to the per-patch path bit for bit; at another batch size the convolutions tile
    differently and a pixel whose probability sits at 0.5 can turn (tests/test_slide_gpu.py).  A model of more than two classes
    gives the (H, W) uint8 map of class indices (``ops.patch_scatter_classes_u8``)."""
    p = int(patch_size)
    size = tuple(int(s) for s in input_size)
    img_d = _resident(img_u8, device, stain)
    C = _n_classes(trainer.model)

    def forward(x):
        input_, _ = trainer.preprocess(x)
        return trainer.model(input_)
    if C > 2:                                        # the painted class indices, pasted as they are
        status = torch.zeros(1, dtype=torch.int32, device=img_d.device)

        def paste(pred, out, first):
            ops.patch_scatter_classes_u8(pred, out, p, first, n_classes=C, mode=0, status=status)
    else:
        def paste(pred, out, first):
            ops.patch_scatter_u8(pred, out, p, first, mode=0)
    result = _patch_walk(img_d, p, size, batch, keep_on_device, False, forward, paste)
    if C > 2:                                        # one word over all passes, read once, behind the map
        _check_status(status, C, 'slide_predict')
    return result


def slide_pixel_predict(model, img_u8, patch_size=PATCH_SIZE, scale=PIXEL_SCALE, batch=2, device='cuda', keep_on_device=False,
                        stain=None):
    """Pixel-wise prediction of a whole slide -> (H, W) uint8 map in {0, 255}: ``pixel_infer`` with ``scales=(scale,)`` on every
    zero-padded patch, pasted and cropped.  Per pass ``ops.patch_gather_resize(align_corners=True)`` to
    ``pixel_infer.target_size`` -> ``model.forward_per_resolution`` -> ``ops.patch_scatter_u8`` reading class 1 in place
    (bilinear back to the patch, round, paste).  A model of more than two classes gives the map of class indices: all C
    planes bilinear back to the patch, the first maximum pasted (``ops.patch_scatter_classes_u8``)."""
    p = int(patch_size)
    size = target_size(p, p, scale)
    if min(size) < 1:
        raise ValueError(f'scale {scale} leaves nothing of a {p} x {p} patch')
    img_d = _resident(img_u8, device, stain)
    if _n_classes(model) > 2:                        # all C planes resized back, the first maximum pasted
        # (mode 1 takes probabilities: nothing comes in as an index and the word is never set -- one for all passes, not read)
        status = torch.zeros(1, dtype=torch.int32, device=img_d.device)

        def paste(probs, out, first):                # probs (valid, h, w, C)
            ops.patch_scatter_classes_u8(probs, out, p, first, mode=1, status=status)
    else:
        def paste(probs, out, first):
            ops.patch_scatter_u8(probs[:, :, :, 1], out, p, first, mode=1)
    return _patch_walk(img_d, p, size, batch, keep_on_device, True, model.forward_per_resolution, paste)


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
         post_threshold=None, log=print, stain_normalize=None):
    """test_dp2019_pipeline.py:114-219 without its patch files: predict every slide of ``data_root/images/*.jpg`` (unless
    ``skip_infer``), write the combined PNGs, score them against ``data_root/masks``.  Returns ``score_directory``'s result.

    The class count is the checkpoint's.  For more than two classes the PNGs hold class indices, the masks are read as class
    indices and ``post_threshold`` (a clean-up of binary maps) is refused.  Under ``skip_infer`` the checkpoint only names the
    output directory and need not exist: without the file the PNGs on disk are scored as two-class maps."""
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
        for path in sorted((data_root / 'images').glob('*.jpg')):
            img = np.asarray(Image.open(path).convert('RGB'))
            if pixel:
                combined = slide_pixel_predict(model, img, patch_size, PIXEL_SCALE, batch=batch or 2, device=device, **kw)
            else:
                combined = slide_predict(trainer, img, patch_size, INPUT_SIZE, batch=batch or 4, device=device, **kw)
            if post_threshold is not None:
                combined = postprocess(combined, post_threshold, device)
            Image.fromarray(combined).save(output_dir / f'{path.stem}.png', format='PNG')
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
    from .stain import add_argument
    add_argument(ap)
    return ap.parse_args(argv)


def cli(argv=None):
    a = parse_args(argv)
    return main(a.data_root, a.checkpoint, model_type=a.model, pixel=a.pixel, patch_size=a.patch_size, skip_infer=a.skip_infer,
                device=a.device, batch=a.batch, post_threshold=a.post_threshold,
                **({} if a.stain_normalize is None else {'stain_normalize': a.stain_normalize}))


if __name__ == '__main__':
    cli()
