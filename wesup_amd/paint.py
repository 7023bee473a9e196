"""Painted comparisons of predicted and ground-truth objects, and mask visualisation (reference scripts/paint_masks.py and
scripts/visualize_masks.py).

  python -m wesup_amd.paint PRED GT [-m MODEL] [-o OUT] [--gpu] [-d DEVICE]     # <stem>.<MODEL or "pred">.png + <stem>.gt.png
  python -m wesup_amd.paint --masks MASK_ROOT [-o OUT]                          # every mask times 255, under the same name

Prediction and ground truth are labelled (8-connected components of the non-zero pixels); every predicted object that covers more
than half of a ground-truth object takes that object's id -- the largest such object, the lowest id among equal areas -- and
every other one a fresh id above both counts; both maps are then painted through one palette, so that matching objects carry the
same colour.  The reference decides the match with one boolean mask per (predicted, ground-truth) pair, O(nP * nG * H * W); here
it is read off the contingency table of the two label maps (``match_objects_from_table``), in integers: ``2 * C[p, g] >
area[g]`` is the reference's ``C / area > 0.5`` exactly for every area below 2^31.

On the host by default (numpy / scipy).  With ``device=`` / ``--gpu`` the labelling, the table, the match and the paint run on the
GPU (csrc/regions.hip, csrc/paint.hip); only the match vector and the two painted maps come back, and they are the same arrays."""
import argparse
import logging
from itertools import product
from pathlib import Path

import numpy as np

from .utils import metrics as M

_log = logging.getLogger(__name__)
_said = set()
EXTENSIONS = ('jpg', 'jpeg', 'png', 'bmp')


def _shuffled_palette():
    """The palette and the state of numpy's legacy generator right after the shuffle that orders it
    (scripts/paint_masks.py:14-22 runs ``np.random.seed(42); np.random.shuffle(colors)`` on the global generator at import; a
    ``RandomState(42)`` of its own is the same stream)."""
    colors = [c for c in product([0, 64, 128, 192, 255], repeat=3) if 192 < sum(c) < 765]      # not close to black or white
    rs = np.random.RandomState(42)
    rs.shuffle(colors)
    return np.array(colors, dtype=np.uint8), rs


def palette():
    """(104, 3) uint8: the reference's colours in its order."""
    return _shuffled_palette()[0]


def reference_rng():
    """A ``RandomState`` in the state the reference's global generator has after its import: what ``paint`` draws the colours of
    the labels beyond the palette from."""
    return _shuffled_palette()[1]


def match_objects_from_table(C):
    """C (nP+1, nG+1): pixels per (predicted object, ground-truth object), row / column 0 the background -> (nP+1,) int64: the
    id every predicted object is repainted with (scripts/paint_masks.py:50-70).  Entry 0 is 0."""
    C = np.asarray(C).astype(np.int64)
    nP, nG = C.shape[0] - 1, C.shape[1] - 1
    out = np.zeros(nP + 1, dtype=np.int64)
    area = C.sum(0)
    for p in range(1, nP + 1):
        cand = np.flatnonzero(2 * C[p, 1:] > area[1:]) + 1
        # the largest matched ground-truth object; argmax keeps the first of equal areas, as Python's max does
        out[p] = cand[np.argmax(area[cand])] if cand.size else max(nP, nG) + p
    return out


def _draw(rs):
    return rs.randint(0, 256, size=(3,), dtype='uint8')


def _colour_table(ids, n, colors, rs):
    """(n, 3) uint8: row 0 black, palette colours for the ids inside the palette, one draw from ``rs`` per id beyond it in
    ascending order of the ids (scripts/paint_masks.py:38-47: ``np.unique`` sorts)."""
    lut = np.zeros((n, 3), dtype=np.uint8)
    for i in np.unique(np.asarray(ids, dtype=np.int64)):
        if i >= len(colors):
            lut[i] = _draw(rs)
        elif i > 0:
            lut[i] = colors[i]
    return lut


def paint(mask, rs=None):
    """A label map (H,W) of non-negative ids -> (H,W,3) uint8: 0 black, 1..103 the palette, every id from 104 on a colour drawn
    from ``rs`` (default: a fresh ``reference_rng()``), ids in ascending order."""
    mask = np.asarray(mask)
    rs = reference_rng() if rs is None else rs
    ids = np.unique(mask)
    return _colour_table(ids, int(ids.max()) + 1, palette(), rs)[mask]


def _say_once(key, msg):
    if key not in _said:
        _said.add(key)
        _log.warning(msg)


def _paint_on_device(pred, gt, rs, device):
    """The device sequence; None when the contingency table is too large to build there."""
    import torch
    from . import ops
    with torch.cuda.device(device):
        both = torch.from_numpy(np.stack([np.asarray(pred) != 0, np.asarray(gt) != 0])).to(device).to(torch.uint8)
        labels, n = ops.cc_label(both, 8, 1)
        nP, nG = (int(v) for v in n.cpu())
        if (nP + 1) * (nG + 1) > ops.CONTINGENCY_MAX_CELLS:
            return None
        table, _ = ops.contingency(labels[0], labels[1], nP, nG)
        match = ops.object_match(table, n[0:1].contiguous(), n[1:2].contiguous()).cpu().numpy().astype(np.int64)
        # the relabelled prediction is never built: its colour table, indexed by the ORIGINAL predicted ids, is the new ids' one
        colors = palette()
        n_new = int(match.max()) + 1
        lut_pred = _colour_table(match[1:], n_new, colors, rs)[match]
        lut_pred[0] = 0
        lut_gt = _colour_table(np.arange(1, nG + 1), nG + 1, colors, rs)
        n_lut = max(nP, nG) + 1
        luts = np.zeros((2, n_lut), dtype=np.int32)
        for row, lut in zip(luts, (lut_pred, lut_gt)):
            row[:len(lut)] = pack_colours(lut)
        out = ops.label_paint(labels, torch.from_numpy(luts).to(device))[0].cpu().numpy()
    return out[0], out[1]


def pack_colours(rgb):
    """(n, 3) uint8 -> (n,) int32, R | G << 8 | B << 16: the colour-table words of ``ops.label_paint``."""
    rgb = np.asarray(rgb, dtype=np.int32)
    return rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16)


def paint_pred_and_gt(pred, gt, rs=None, device=None):
    """(painted prediction, painted ground truth), two (H,W,3) uint8 arrays (scripts/paint_masks.py:50-72): the prediction
    relabelled by ``match_objects_from_table`` is painted first, the labelled ground truth second, both from the same ``rs``
    (default: a fresh ``reference_rng()``)."""
    rs = reference_rng() if rs is None else rs
    if device is not None:
        out = _paint_on_device(pred, gt, rs, device)
        if out is not None:
            return out
        _say_once('table', 'the contingency table of this pair is too large to build on the device: such pairs are painted on '
                           'the host')
    P, G = M.label(pred), M.label(gt)
    C = M._contingency(P, G)[0]
    return paint(match_objects_from_table(C)[P], rs), paint(G, rs)


def list_images(path):
    """The images of a directory in sorted order (scripts/paint_masks.py:25-31)."""
    return sorted(p for ext in EXTENSIONS for p in Path(path).glob(f'*.{ext}'))


def _read(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _read_mask(path):
    a = _read(path)
    return a[..., 0] if a.ndim == 3 else a


def paint_dir(pred_path, gt_path, model=None, output=None, device=None, log=print):
    """scripts/paint_masks.py:75-112: every prediction of ``pred_path`` with the ground truth of the same rank in ``gt_path``
    -> ``<stem>.<model or "pred">.png`` and ``<stem>.gt.png`` in ``output`` (default: ``paintings`` next to ``pred_path``).  One
    generator serves the whole directory in file order, as in a single-process run of the reference.  Returns the paths written."""
    from PIL import Image
    pred_path, gt_path = Path(pred_path), Path(gt_path)
    preds, gts = list_images(pred_path), list_images(gt_path)
    if len(preds) != len(gts):
        raise ValueError(f'{len(preds)} predictions in {pred_path} but {len(gts)} masks in {gt_path}')
    output = pred_path.parent / 'paintings' if output is None else Path(output)
    output.mkdir(parents=True, exist_ok=True)
    rs = reference_rng()
    written = []
    log('Painting beautiful illustrations ...')
    for p, g in zip(preds, gts):
        pair = paint_pred_and_gt(_read_mask(p), _read_mask(g), rs, device)
        for image, name in zip(pair, (f'{p.stem}.{model or "pred"}.png', f'{p.stem}.gt.png')):
            Image.fromarray(image).save(output / name)
            written.append(output / name)
    log(f'Saved paintings to {output}')
    return written


def visualize_masks(mask_root, output=None):
    """scripts/visualize_masks.py: every mask of ``mask_root`` times 255 (uint8 arithmetic, as read), under the same name in
    ``output`` (default: ``viz`` next to ``mask_root``).  Returns the paths written."""
    from PIL import Image
    mask_root = Path(mask_root)
    output = mask_root.parent / 'viz' if output is None else Path(output)
    output.mkdir(parents=True, exist_ok=True)
    written = []
    for path in list_images(mask_root):
        Image.fromarray(_read(path) * 255).save(output / path.name)
        written.append(output / path.name)
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('pred_path', nargs='?', help='model predictions')
    ap.add_argument('gt_path', nargs='?', help='ground-truth masks')
    ap.add_argument('-m', '--model', help='model name in the file names of the painted predictions')
    ap.add_argument('-o', '--output', help='output directory')
    ap.add_argument('--masks', metavar='MASK_ROOT', help='write every mask of this directory times 255 instead of painting')
    ap.add_argument('-d', '--device', default='cuda')
    ap.add_argument('--gpu', action='store_true', help='label, match and paint on --device instead of the CPU')
    a = ap.parse_args(argv)
    if a.masks:
        visualize_masks(a.masks, a.output)
    elif a.pred_path and a.gt_path:
        paint_dir(a.pred_path, a.gt_path, a.model, a.output, a.device if a.gpu else None)
    else:
        ap.error('give PRED and GT, or --masks MASK_ROOT')


if __name__ == '__main__':
    main()
