"""Surface-distance metrics of segmentation masks: HD, HD95, ASSD and surface Dice at a tolerance (NSD).

  python -m wesup_amd.surface PRED_DIR GT_DIR [--gpu] [--tolerance TAU] [--classes C] [--csv OUT]

The region scores of ``evaluate.py`` (accuracy, Dice, the object-level challenge metrics) say nothing about where a boundary lies.
These four do: with S_P and S_G the border pixels of the prediction and of the ground truth, and d(p, S) the Euclidean distance
from a pixel to the nearest pixel of S,

  hd    the largest of all d(p, S_G), p in S_P, and d(g, S_P), g in S_G
  hd95  the 95th percentile (numpy's linear rule) of those distances, both directions in one array: MedPy's ``hd95``
  assd  the mean of the two directed mean distances: MedPy's ``assd``
  nsd   the share of the border pixels of both masks that lie within ``tolerance`` of the other border

The functions ending in ``_host`` are the definition, in numpy; every value that is compared is an integer (squared distances),
and the device path (csrc/surface.hip, ``ops.surface_stats``) is held to them bit for bit, the two float64 sums of square roots to
their rounding."""
import argparse
import csv
import math
from pathlib import Path

import numpy as np

EDT_NONE = 2 ** 31 - 1           # the distance map of an image without a zero pixel (WESUP_EDT_NONE)
STAT_KEYS = ('n_p', 'n_g', 'max_pg', 'max_gp', 'within_p', 'within_g', 'lo', 'hi', 'sum_pg', 'sum_gp')
SCORE_KEYS = ('hd', 'hd95', 'assd', 'nsd')


def _check_shape(H, W):
    if H < 1 or W < 1:
        raise ValueError(f'mask: empty shape ({H}, {W})')
    if (H - 1) ** 2 + (W - 1) ** 2 >= EDT_NONE:
        raise ValueError(f'mask ({H}, {W}): squared distances reach {EDT_NONE}')


def edt_sq_full_host(mask):
    """Exact squared Euclidean distance map, int32: 0 where ``mask`` is 0, elsewhere |p - z|^2 to the nearest zero pixel z of the
    same image; ``EDT_NONE`` everywhere in an image without a zero pixel.  Pixels outside the image are not zero pixels
    (scipy.ndimage.distance_transform_edt's convention, and split.edt_sq_host's); (H,W) or (B,H,W).  Two integer passes: the
    distance to the nearest zero pixel of the column by a running count down and up, then the minimum over the row of
    dx^2 + that distance^2."""
    F = np.asarray(mask) != 0
    if F.ndim == 3:
        if len(F):
            _check_shape(*F.shape[1:])
        return np.stack([edt_sq_full_host(f) for f in F]) if len(F) else np.zeros(F.shape, np.int32)
    if F.ndim != 2:
        raise ValueError(f'mask: expected (H,W) or (B,H,W), got {F.shape}')
    H, W = F.shape
    _check_shape(H, W)
    far = H + W                                    # above every column distance
    g = np.empty((H, W), np.int64)
    run = np.full(W, far, np.int64)
    for y in range(H):                             # the nearest zero at or above
        run = np.where(F[y], np.minimum(run + 1, far), 0)
        g[y] = run
    run = np.full(W, far, np.int64)
    for y in range(H - 1, -1, -1):                 # ... or below
        run = np.where(F[y], np.minimum(run + 1, far), 0)
        g[y] = np.minimum(g[y], run)
    g2 = np.where(g >= far, EDT_NONE, g * g)
    best = g2.copy()
    for dx in range(1, W):
        sq = dx * dx
        if sq >= best.max():                       # no offset from here on can improve any pixel
            break
        best[:, dx:] = np.minimum(best[:, dx:], g2[:, :-dx] + sq)
        best[:, :-dx] = np.minimum(best[:, :-dx], g2[:, dx:] + sq)
    return np.minimum(best, EDT_NONE).astype(np.int32)


def border_host(mask):
    """bool: the foreground pixels with at least one of their four neighbours on the background or outside the image --
    ``mask & ~binary_erosion(mask, generate_binary_structure(2, 1), border_value=0)``, the border of MedPy and of
    surface-distance.  (H,W) or (B,H,W)."""
    F = np.asarray(mask) != 0
    if F.ndim == 3:
        return np.stack([border_host(f) for f in F]) if len(F) else np.zeros(F.shape, bool)
    if F.ndim != 2:
        raise ValueError(f'mask: expected (H,W) or (B,H,W), got {F.shape}')
    P = np.pad(F, 1)
    inner = P[:-2, 1:-1] & P[2:, 1:-1] & P[1:-1, :-2] & P[1:-1, 2:]
    return F & ~inner


def _tolerance_sq(tolerance):
    tolerance = float(tolerance)
    if not tolerance >= 0 or math.isinf(tolerance):
        raise ValueError(f'tolerance {tolerance}: expected a finite value >= 0')
    return int(math.floor(tolerance * tolerance))


def _q_frac(q):
    q = float(q)
    if not 0.0 <= q <= 100.0:
        raise ValueError(f'q {q}: expected 0 .. 100')
    return q / 100.0


def _mask_pair(pred, gt):
    P, G = np.asarray(pred) != 0, np.asarray(gt) != 0
    if P.shape != G.shape or P.ndim != 2:
        raise ValueError(f'pred {P.shape} and gt {G.shape}: expected two (H,W) masks of one shape')
    return P, G


def surface_stats_host(pred, gt, tolerance, q=95.0):
    """The raw quantities of the surface metrics of one image pair, a dict of ``STAT_KEYS``: the sizes of the two borders, the
    largest squared distance per direction, the counts of squared distances <= floor(tolerance^2), the order statistics
    k = floor((n - 1) q / 100) and min(k + 1, n - 1) of all n = n_p + n_g squared distances together (integers), and the float64
    sums of the distances per direction.  An empty border contributes 0 to its count, maximum and sum; the distances TO an empty
    border are sqrt(EDT_NONE); with both empty lo = hi = 0."""
    P, G = _mask_pair(pred, gt)
    t2, qf = _tolerance_sq(tolerance), _q_frac(q)
    SP, SG = border_host(P), border_host(G)
    d2_pg = edt_sq_full_host(~SG)[SP].astype(np.int64)
    d2_gp = edt_sq_full_host(~SP)[SG].astype(np.int64)
    n_p, n_g = int(d2_pg.size), int(d2_gp.size)
    n = n_p + n_g
    lo = hi = 0
    if n:
        both = np.sort(np.concatenate((d2_pg, d2_gp)))
        k = min(max(int(math.floor((n - 1) * qf)), 0), n - 1)
        lo, hi = int(both[k]), int(both[min(k + 1, n - 1)])
    return {'n_p': n_p, 'n_g': n_g,
            'max_pg': int(d2_pg.max()) if n_p else 0, 'max_gp': int(d2_gp.max()) if n_g else 0,
            'within_p': int((d2_pg <= t2).sum()), 'within_g': int((d2_gp <= t2).sum()),
            'lo': lo, 'hi': hi,
            'sum_pg': float(np.sqrt(d2_pg.astype(np.float64)).sum()), 'sum_gp': float(np.sqrt(d2_gp.astype(np.float64)).sum())}


def scores_from_stats(st, q=95.0):
    """``{'hd', 'hd95', 'assd', 'nsd'}`` from the raw quantities, in float64 on the host.  Both borders empty: 0, 0, 0, 1; exactly
    one empty: inf, inf, inf, 0 (the conventions of ``metrics.hausdorff``).  The percentile is numpy's linear rule on the two
    order statistics: with t = (n - 1) q / 100 - k and d = b - a it is a + d t below t = 0.5 and b - d (1 - t) from there on."""
    n_p, n_g = int(st['n_p']), int(st['n_g'])
    if n_p == 0 and n_g == 0:
        return {'hd': 0.0, 'hd95': 0.0, 'assd': 0.0, 'nsd': 1.0}
    if n_p == 0 or n_g == 0:
        return {'hd': math.inf, 'hd95': math.inf, 'assd': math.inf, 'nsd': 0.0}
    n = n_p + n_g
    qf = _q_frac(q)
    k = min(max(int(math.floor((n - 1) * qf)), 0), n - 1)
    a, b = math.sqrt(int(st['lo'])), math.sqrt(int(st['hi']))
    t, d = (n - 1) * qf - k, b - a
    return {'hd': math.sqrt(max(int(st['max_pg']), int(st['max_gp']))),
            'hd95': a + d * t if t < 0.5 else b - d * (1 - t),
            'assd': (float(st['sum_pg']) / n_p + float(st['sum_gp']) / n_g) / 2,
            'nsd': (int(st['within_p']) + int(st['within_g'])) / n}


DEFAULT_TOLERANCE = 2.0


def surface_scores_host(pred, gt, tolerance=DEFAULT_TOLERANCE):
    """HD, HD95, ASSD and NSD of one pair of binary masks (non-zero = foreground) on the host.  ``tolerance`` is NSD's, in pixels;
    the default of 2 is an interface default, not a measured optimum -- a study names its own."""
    return scores_from_stats(surface_stats_host(pred, gt, tolerance))


def surface_scores_classes_host(pred_map, gt_map, n_classes, tolerance=DEFAULT_TOLERANCE):
    """Class-index maps -> a list of the four scores per class c = 0 .. n_classes - 1, each on ``map == c``."""
    P, G = np.asarray(pred_map), np.asarray(gt_map)
    n_classes = _check_classes(n_classes)
    return [surface_scores_host(P == c, G == c, tolerance) for c in range(n_classes)]


def hausdorff_full_host(S, G):
    """The symmetric Hausdorff distance over ALL pixels of two masks (``utils.metrics.hausdorff``) by way of two distance maps:
    sqrt(max(edt(~G)[S].max(), edt(~S)[G].max()))."""
    S, G = _mask_pair(S, G)
    if not S.any() and not G.any():
        return 0
    if not S.any() or not G.any():
        return np.inf
    return math.sqrt(max(int(edt_sq_full_host(~G)[S].max()), int(edt_sq_full_host(~S)[G].max())))


def _check_classes(n_classes):
    n_classes = int(n_classes)
    if not 1 <= n_classes <= 256:
        raise ValueError(f'n_classes {n_classes}: expected 1 .. 256')
    return n_classes


def _device_masks(masks, device):
    import torch
    return torch.tensor(np.ascontiguousarray(masks)).to(device).to(torch.uint8).contiguous()


def _device_scores(P, G, tolerance, device):
    """(B,H,W) bool stacks -> a list of B score dicts; one launch chain and one read-back for the stack."""
    import torch
    from . import ops
    p, g = _device_masks(P, device), _device_masks(G, device)
    with torch.cuda.device(p.device):
        stats = ops.surface_stats(p, g, tolerance)
    return [scores_from_stats(st) for st in stats]


def surface_scores(pred, gt, tolerance=DEFAULT_TOLERANCE, device=None):
    """``surface_scores_host``, or with ``device`` the same on the GPU (ops.surface_stats; the float64 formulas stay on the host).
    The default tolerance of 2 pixels is an interface default, not a measured optimum."""
    if device is None:
        return surface_scores_host(pred, gt, tolerance)
    P, G = _mask_pair(pred, gt)
    _tolerance_sq(tolerance)
    return _device_scores(P[None], G[None], tolerance, device)[0]


def surface_scores_classes(pred_map, gt_map, n_classes, tolerance=DEFAULT_TOLERANCE, device=None):
    """``surface_scores_classes_host``, or with ``device`` on the GPU: the classes ride on the batch axis of the kernels."""
    if device is None:
        return surface_scores_classes_host(pred_map, gt_map, n_classes, tolerance)
    P, G = np.asarray(pred_map), np.asarray(gt_map)
    n_classes = _check_classes(n_classes)
    if P.shape != G.shape or P.ndim != 2:
        raise ValueError(f'pred {P.shape} and gt {G.shape}: expected two (H,W) class maps of one shape')
    _tolerance_sq(tolerance)
    cls = np.arange(n_classes).reshape(-1, 1, 1)
    return _device_scores(P[None] == cls, G[None] == cls, tolerance, device)


def hausdorff_full(S, G, device=None):
    """``hausdorff_full_host``, or with ``device`` from two device distance maps (ops.edt_sq_full with ``invert``)."""
    if device is None:
        return hausdorff_full_host(S, G)
    import torch
    from . import ops
    S, G = _mask_pair(S, G)
    if not S.any() and not G.any():
        return 0
    if not S.any() or not G.any():
        return np.inf
    m = _device_masks(np.stack([G, S]), device)
    with torch.cuda.device(m.device):
        d2 = ops.edt_sq_full(m, invert=True)                 # the distances to G, then to S
        other = torch.flip(m, (0,)) != 0
        worst = int(torch.where(other, d2, torch.zeros_like(d2)).max())
    return math.sqrt(worst)


def score_directory(pred_dir, gt_dir, tolerance=DEFAULT_TOLERANCE, n_classes=None, device=None, csv_path=None, log=print):
    """Score the ``*.png`` / ``*.bmp`` of ``pred_dir`` against those of ``gt_dir``, both sorted.  Without ``n_classes`` the files are
    masks (non-zero = foreground: 0/255 predictions, object-id ground truth); with it they are class-index maps and every class
    is scored on its own.  Logs the means (``nanmean``, an infinite value counted as missing) and optionally writes the rows
    -> (rows, means); a row is ``{'name', 'class', 'hd', 'hd95', 'assd', 'nsd'}``."""
    from PIL import Image
    exts = ('*.bmp', '*.png')
    pred_dir, gt_dir = Path(pred_dir).expanduser(), Path(gt_dir).expanduser()
    pred_paths = sorted(p for e in exts for p in pred_dir.glob(e))
    gt_paths = sorted(p for e in exts for p in gt_dir.glob(e))
    if len(pred_paths) != len(gt_paths):
        raise ValueError(f'{len(pred_paths)} predictions in {pred_dir} but {len(gt_paths)} masks in {gt_dir}')

    def read(path):
        a = np.asarray(Image.open(path))
        return a[..., 0] if a.ndim == 3 else a

    rows = []
    for pp, gp in zip(pred_paths, gt_paths):
        pred, gt = read(pp), read(gp)
        if n_classes is None:
            per_class = [surface_scores(pred, gt, tolerance, device)]
        else:
            per_class = surface_scores_classes(pred, gt, n_classes, tolerance, device)
        for c, s in enumerate(per_class):
            rows.append({'name': pp.name, 'class': c if n_classes is not None else '', **s})
    means = {}
    for k in SCORE_KEYS:
        vals = [r[k] for r in rows if math.isfinite(r[k])]
        means[k] = float(np.mean(vals)) if vals else float('nan')
    for name, k in (('Hausdorff', 'hd'), ('HD95', 'hd95'), ('ASSD', 'assd'), (f'NSD@{tolerance:g}', 'nsd')):
        log(f'{name}: {means[k]}')
    if csv_path is not None:
        with open(csv_path, 'w', newline='') as fp:
            out = csv.writer(fp)
            out.writerow(['', 'class'] + list(SCORE_KEYS))
            for r in rows:
                out.writerow([r['name'], r['class']] + [r[k] for k in SCORE_KEYS])
    return rows, means


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('pred_dir', help='directory of predicted masks (0/255) or class-index maps (*.png, *.bmp)')
    ap.add_argument('gt_dir', help='the ground truth under the same sorted order')
    ap.add_argument('--gpu', action='store_true', help='score on the device (ops.surface_stats)')
    ap.add_argument('-d', '--device', default='cuda')
    ap.add_argument('--tolerance', type=float, default=DEFAULT_TOLERANCE, metavar='TAU',
                    help='NSD tolerance in pixels (default 2: an interface default, not a measured optimum)')
    ap.add_argument('--classes', type=int, metavar='C', help='the files are class-index maps: score classes 0 .. C-1 each')
    ap.add_argument('--csv', metavar='OUT', help='write the per-image rows there')
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    score_directory(a.pred_dir, a.gt_dir, a.tolerance, a.classes, a.device if a.gpu else None, a.csv)


if __name__ == '__main__':
    main()
