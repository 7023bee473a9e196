"""GlaS, CRAG and LUSC evaluation: small-region post-processing of predicted masks, the challenge metrics over a directory
of predictions, and the test-set driver (reference scripts/evaluate_glas.py:29-98, scripts/evaluate_crag.py,
scripts/evaluate_pdl1.py and test_glas.py:13-61).

  python -m wesup_amd.evaluate PRED_ROOT --gt-root ~/data/GLAS_all        # post-process + score testA / testB
  python -m wesup_amd.evaluate PRED_ROOT --dataset crag [--gt-dir DIR]    # a flat directory, 5000-pixel rule (also: lusc)
  python -m wesup_amd.evaluate PRED_ROOT --surface-metrics [TAU]          # ... plus HD95, ASSD and NSD at TAU pixels (default 2)
  python -m wesup_amd.evaluate --test -c CKPT --scales 0.6,0.55,0.5,0.45,0.4 --data-root ~/data/GLAS_all

Evaluation-time code on the CPU by default, as in the reference (numpy / scipy; the training step does not touch it).
With ``device=`` / ``--gpu-scoring`` the post-processing and the scoring run on the GPU (csrc/regions.hip,
utils/metrics_gpu.py): integer kernels and the same float64 formulas on the host, so the numbers are the same."""
import argparse
import csv
from pathlib import Path

import numpy as np

from .utils import metrics as M

MIN_REGION = 2000        # pixels (scripts/evaluate_glas.py:33,39)
MIN_REGION_FLAT = 5000   # CRAG and LUSC (scripts/evaluate_crag.py:33,39, scripts/evaluate_pdl1.py:30,36)
FLAT_GT_DIRS = {'crag': '~/data/CRAG/test/masks', 'lusc': 'LUSC/test/masks'}   # evaluate_crag.py:65 (its author's home), evaluate_pdl1.py:73


def remove_small_regions(pred, min_size=MIN_REGION, device=None):
    """Post-processing of a binary prediction (scripts/evaluate_glas.py:29-43): connected foreground regions smaller
    than ``min_size`` pixels are erased, then connected background regions (holes) smaller than ``min_size`` are
    filled -- the second pass sees the result of the first.  8-connected components (skimage.measure.label's default
    for 2-D input).  The reference walks the regions one boolean mask at a time; here one ``bincount`` of the label map
    gives every region's area and one table lookup rewrites the mask.  With ``device`` both passes run there
    (ops.remove_small_regions); the result comes back as the same float64 array."""
    if device is not None:
        import torch
        from . import ops
        m = torch.tensor(np.asarray(pred) != 0).to(device).to(torch.uint8)
        return ops.remove_small_regions(m, min_size).cpu().numpy().astype(np.float64)
    out = (np.asarray(pred) != 0).astype(np.float64)
    for value in (1.0, 0.0):                       # erase small foreground regions, then fill small holes
        regions = M.label(out == value)
        area = np.bincount(regions.ravel())
        small = area < min_size
        small[0] = False                           # label 0 is "everything else", not a region of this pass
        out[small[regions]] = 1.0 - value
    return out


def _read_mask(path):
    from PIL import Image
    a = np.asarray(Image.open(path))
    return a[..., 0] if a.ndim == 3 else a


def score(predictions, gts, binarize_gt=False, device=None, surface=None):
    """Per-image rows and means of accuracy, Dice and the three object-level challenge metrics
    (scripts/evaluate_glas.py:46-69).  The reference hands the ground-truth OBJECT maps (ids 0..n) to ``accuracy`` and
    ``dice`` as they are -- for GlaS that compares a {0, 1} prediction with instance ids; kept by default so that the
    numbers are the reference's, ``binarize_gt=True`` scores against ``gt > 0`` instead.  With ``device`` the three
    object-level metrics of an image come from one pass on the GPU (metrics_gpu.challenge_scores).

    ``surface=tau`` adds the boundary columns ``hd95``, ``assd`` and ``nsd`` at tolerance ``tau`` pixels (surface.py, DESIGN.md
    3.20) to every row and to the means.  They compare ``pred != 0`` with ``gt > 0``: the ground truth is binarised for these
    three whatever ``binarize_gt`` says.  An infinite value (one of the two masks empty) is written as ``nan``, like the Hausdorff
    column.  With ``surface=None`` the rows are those of before."""
    rows = []
    for pred, gt in zip(predictions, gts):
        gt = np.asarray(gt)
        flat = (gt > 0).astype(pred.dtype) if binarize_gt else gt
        if device is not None:
            import torch
            from .utils import metrics_gpu
            with torch.cuda.device(device):
                obj = metrics_gpu.challenge_scores(torch.tensor(np.asarray(pred)).to(device),
                                                   torch.tensor(np.asarray(gt)).to(device))
            rows.append({'accuracy': float(M.accuracy(pred, flat)), 'dice': float(M.dice(pred, flat)),
                         'detection_f1': obj['detection_f1'], 'object_dice': obj['object_dice'],
                         'object_hausdorff': obj['object_hausdorff']})
            _add_surface(rows[-1], pred, gt, surface, device)
            continue
        rows.append({'accuracy': float(M.accuracy(pred, flat)),
                     'dice': float(M.dice(pred, flat)),
                     'detection_f1': float(M.detection_f1(pred, gt)),
                     'object_dice': float(M.object_dice(pred, gt)),
                     'object_hausdorff': float(M.object_hausdorff(pred, gt)) if pred.any() and gt.any() else float('nan')})
        _add_surface(rows[-1], pred, gt, surface, device)
    means = {k: float(np.nanmean([r[k] for r in rows])) for k in (rows[0] if rows else {})}
    return rows, means


SURFACE_COLUMNS = ('hd95', 'assd', 'nsd')


def _add_surface(row, pred, gt, tolerance, device):
    if tolerance is None:
        return
    from . import surface
    s = surface.surface_scores(np.asarray(pred) != 0, np.asarray(gt) > 0, tolerance, device)
    for k in SURFACE_COLUMNS:
        row[k] = float(s[k]) if np.isfinite(s[k]) else float('nan')


def split_objects(pred, radius, device=None):
    """Separate touching objects of a post-processed prediction (split.split_objects) -> the same float64 {0, 1}
    array as ``remove_small_regions`` returns."""
    from . import split
    return split.split_objects(np.asarray(pred) != 0, radius, device).astype(np.float64)


def _evaluate_paths(pred_paths, gt_paths, new_pred_dir, csv_path, min_size, log, device, split_radius=None,
                    surface_tolerance=None):
    """Post-process the predictions (0/255 images), optionally save them, score them against the ground truth as read, log the
    five means and optionally write the per-image csv -> (rows, means, post-processed predictions).  With ``split_radius``
    touching objects are separated after the small-region rule; the saved maps and the scores are those of the split maps.
    With ``surface_tolerance`` three more means are logged (HD95, ASSD, NSD) and the csv gains their columns."""
    from PIL import Image
    predictions = [remove_small_regions(_read_mask(p) / 255, min_size, device) for p in pred_paths]
    if split_radius is not None:
        predictions = [split_objects(p, split_radius, device) for p in predictions]
    gts = [_read_mask(p) for p in gt_paths]
    if new_pred_dir is not None:
        Path(new_pred_dir).mkdir(parents=True, exist_ok=True)
        for pred, path in zip(predictions, pred_paths):
            Image.fromarray((pred * 255).astype('uint8')).save(Path(new_pred_dir) / path.name)
    rows, means = score(predictions, gts, device=device, surface=surface_tolerance)
    for name, key in (('Accuracy', 'accuracy'), ('Dice', 'dice'), ('Detection F1', 'detection_f1'),
                      ('Object Dice', 'object_dice'), ('Object Hausdorff', 'object_hausdorff')):
        log(f'{name}: {means.get(key, float("nan"))}')
    extra = () if surface_tolerance is None else SURFACE_COLUMNS
    for name, key in (('HD95', 'hd95'), ('ASSD', 'assd'), (f'NSD@{surface_tolerance}', 'nsd')) if extra else ():
        log(f'{name}: {means.get(key, float("nan"))}')
    if csv_path is not None:
        with open(csv_path, 'w', newline='') as fp:
            out = csv.writer(fp)
            out.writerow(['', 'detection_f1', 'object_dice', 'object_hausdorff', *extra])
            for path, r in zip(pred_paths, rows):
                out.writerow([path.name, r['detection_f1'], r['object_dice'], r['object_hausdorff'], *(r[k] for k in extra)])
    return rows, means, predictions


def evaluate_split(pred_dir, gt_dir, new_pred_dir=None, csv_path=None, min_size=MIN_REGION, log=print, device=None,
                   split_radius=None, surface_tolerance=None):
    """One test split: read predictions (0/255 images) and ground-truth object maps in sorted order, post-process,
    optionally save the new predictions and the per-image csv (columns of scripts/evaluate_glas.py:62-66)."""
    exts = ('*.bmp', '*.png')
    pred_paths = sorted(p for e in exts for p in Path(pred_dir).glob(e))
    gt_paths = sorted(p for e in exts for p in Path(gt_dir).glob(e))
    if len(pred_paths) != len(gt_paths):
        raise ValueError(f'{len(pred_paths)} predictions in {pred_dir} but {len(gt_paths)} masks in {gt_dir}')
    return _evaluate_paths(pred_paths, gt_paths, new_pred_dir, csv_path, min_size, log, device, split_radius,
                           surface_tolerance)[:2]


def evaluate_flat(pred_root, gt_dir, min_size=MIN_REGION_FLAT, log=print, device=None, csv_path=None, split_radius=None,
                  surface_tolerance=None):
    """scripts/evaluate_crag.py and scripts/evaluate_pdl1.py (one script but for the ground-truth directory): the ``*.png``
    of ``pred_root`` against the ``*.png`` of ``gt_dir``, both sorted, the ground truth used as read; small regions and holes
    below ``min_size`` = 5000 pixels are removed, the post-processed maps go to ``<pred_root>-new/`` and the five means are
    logged in the reference's wording and order -> (rows, means, post-processed maps).

    The one deliberate difference: the scoring is ``score``'s, whose Hausdorff term is ``nan`` for an image with an empty map and
    whose means are ``nanmean`` -- the reference's ``np.mean`` of an ``inf`` there says nothing about the other images.  With every
    map non-empty the numbers are the reference's."""
    pred_root, gt_dir = Path(pred_root).expanduser(), Path(gt_dir).expanduser()
    pred_paths, gt_paths = sorted(pred_root.glob('*.png')), sorted(gt_dir.glob('*.png'))
    if len(pred_paths) != len(gt_paths):
        raise ValueError(f'{len(pred_paths)} predictions in {pred_root} but {len(gt_paths)} masks in {gt_dir}')
    new_root = pred_root.parent / (pred_root.name + '-new')
    return _evaluate_paths(pred_paths, gt_paths, new_root, csv_path, min_size, log, device, split_radius, surface_tolerance)


def evaluate_glas(pred_root, gt_root='~/data/GLAS_all', min_size=MIN_REGION, log=print, device=None, split_radius=None,
                  surface_tolerance=None):
    """scripts/evaluate_glas.py: testA and testB under ``pred_root`` against ``gt_root/<split>/masks``; post-processed
    predictions go to ``<pred_root>-new/<split>``, per-image metrics to ``pred_root/<split>.csv``."""
    pred_root, gt_root = Path(pred_root).expanduser(), Path(gt_root).expanduser()
    new_root = pred_root.parent / (pred_root.name + '-new')
    result = {}
    for split, title in (('testA', 'Test A'), ('testB', '\nTest B')):
        if not (pred_root / split).exists():
            continue
        log(title)
        result[split] = evaluate_split(pred_root / split, gt_root / split / 'masks', new_root / split,
                                       pred_root / f'{split}.csv', min_size, log, device, split_radius, surface_tolerance)[1]
    return result


def test(ckpt_path, model_type='wesup', input_size=None, scales=(0.5,), device='cuda', data_root='~/data/GLAS_all'):
    """test_glas.py:13-38: load a checkpoint, predict test sets A and B into ``<record_dir>/results`` (fixed input
    size) or ``<record_dir>/results-<n>scale`` (multi-scale)."""
    from .infer import infer
    from .models import initialize_trainer
    ckpt_path = Path(ckpt_path)
    trainer = initialize_trainer(model_type, device=device)
    from .models import require_two_class_checkpoint
    require_two_class_checkpoint(ckpt_path, 'GlaS evaluation')
    trainer.load_checkpoint(ckpt_path)
    record_dir = ckpt_path.parent.parent
    results_dir = record_dir / ('results' if input_size is not None else f'results-{len(scales)}scale')
    results_dir.mkdir(parents=True, exist_ok=True)
    data_root = Path(data_root).expanduser()
    for split in ('testA', 'testB'):
        if (data_root / split).exists():
            print(f'\nTesting on test set {split[-1]} ...')
            infer(trainer, data_root / split, results_dir / split, input_size, scales, device=device)
    return results_dir


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('pred_root', nargs='?')
    ap.add_argument('--gt-root', default='~/data/GLAS_all')
    ap.add_argument('--dataset', choices=('glas', 'crag', 'lusc'), default='glas',
                    help='glas: testA / testB under PRED_ROOT; crag, lusc: a flat directory of predictions')
    ap.add_argument('--gt-dir', help='ground-truth masks of --dataset crag / lusc (default: ' +
                                     ', '.join(f'{k}: {v}' for k, v in FLAT_GT_DIRS.items()) + ')')
    ap.add_argument('--min-size', type=int, help=f'default: {MIN_REGION} for glas, {MIN_REGION_FLAT} for crag and lusc')
    ap.add_argument('--test', action='store_true', help='run the test-set driver (test_glas.py) instead of scoring')
    ap.add_argument('-m', '--model', default='wesup')
    ap.add_argument('-c', '--checkpoint')
    ap.add_argument('--input-size')
    ap.add_argument('--scales', default='0.6,0.55,0.5,0.45,0.4')          # test_glas.py:48
    ap.add_argument('--data-root', default='~/data/GLAS_all')
    ap.add_argument('-d', '--device', default='cuda')
    ap.add_argument('--gpu-scoring', action='store_true', help='post-process and score on --device instead of the CPU')
    ap.add_argument('--split-objects', type=int, metavar='R', dest='split_objects',
                    help='separate touching objects after the small-region rule: seed radius in pixels, 1 .. 255 '
                         '(wesup_amd/split.py; glas, crag and lusc)')
    ap.add_argument('--surface-metrics', type=float, nargs='?', const=2.0, metavar='TAU', dest='surface_metrics',
                    help='also score boundaries: HD95, ASSD and NSD at TAU pixels (wesup_amd/surface.py; glas, crag and lusc).  '
                         'TAU defaults to 2, an interface default and not a measured optimum')
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.split_objects is not None and not 1 <= a.split_objects <= 255:
        raise SystemExit(f'--split-objects {a.split_objects}: expected 1 .. 255')
    if a.surface_metrics is not None and not 0 <= a.surface_metrics < float('inf'):
        raise SystemExit(f'--surface-metrics {a.surface_metrics}: expected a finite tolerance >= 0')
    extra = {} if a.split_objects is None else {'split_radius': a.split_objects}      # (without the flag: the calls of before)
    if a.surface_metrics is not None:
        extra['surface_tolerance'] = a.surface_metrics
    if a.test:
        size = [int(s) for s in a.input_size.split(',')] if a.input_size else None
        test(a.checkpoint, a.model, size, tuple(float(s) for s in a.scales.split(',')), a.device, a.data_root)
    elif a.dataset == 'glas':
        evaluate_glas(a.pred_root, a.gt_root, MIN_REGION if a.min_size is None else a.min_size,
                      device=a.device if a.gpu_scoring else None, **extra)
    else:
        evaluate_flat(a.pred_root, a.gt_dir or FLAT_GT_DIRS[a.dataset], MIN_REGION_FLAT if a.min_size is None else a.min_size,
                      device=a.device if a.gpu_scoring else None, **extra)


if __name__ == '__main__':
    main()
