"""Golden outputs of the reference's whole-slide pipeline (development machine only: it needs the reference checkout).

Runs the reference's ``test_dp2019_pipeline.py`` unmodified, by path, as ``__main__`` on a temporary data root with one random
150 x 131 slide at patch size 64, and records what its own functions produce -> ``tests/golden/dp2019.npz`` (a few KB).  Its
absent imports get stand-in modules, the method of ``oracle/make_golden.py``: ``cv2`` whose ``imwrite`` / ``imread`` capture and
return arrays (a file of the same name is touched, so that the script's globs find it), ``skimage.measure.label`` as
``scipy.ndimage.label`` with the full 3 x 3 structure, ``joblib`` / ``tqdm`` as plain loops, and ``infer`` / ``pixel_infer``
whose ``main`` writes one random {0, 255} prediction per patch through the same ``cv2.imwrite``.

    python tools/make_slide_golden.py [--reference DIR] [--out tests/golden/dp2019.npz]
"""
import argparse
import contextlib
import io
import os
import runpy
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

H, W, P = 150, 131, 64
ROOT = Path(__file__).resolve().parent.parent


def _install_standins(store, rs):
    from scipy import ndimage

    cv2 = types.ModuleType('cv2')
    cv2.IMREAD_GRAYSCALE = 0

    def imwrite(dest, array):
        store[str(dest)] = np.array(array, copy=True)
        Path(dest).touch()
        return True

    def imread(path, flag=None):
        return store[str(path)].copy()
    cv2.imwrite, cv2.imread = imwrite, imread

    skimage, measure = types.ModuleType('skimage'), types.ModuleType('skimage.measure')
    measure.label = lambda a: ndimage.label(np.asarray(a) != 0, structure=np.ones((3, 3), dtype=np.int32))[0]
    skimage.measure = measure

    joblib = types.ModuleType('joblib')
    joblib.Parallel = lambda *a, **k: (lambda jobs: [job() for job in jobs])
    joblib.delayed = lambda fn: (lambda *a, **k: (lambda: fn(*a, **k)))

    tqdm = types.ModuleType('tqdm')
    tqdm.tqdm = lambda it, **k: it

    def predictor(patch_dir, output_dir=None, **kwargs):
        for path in sorted((Path(patch_dir) / 'images').iterdir()):
            patch = store[str(path)]
            pred = (rs.rand(*patch.shape[:2]) < 0.5).astype(np.uint8) * 255
            imwrite(Path(output_dir) / path.name.replace('.jpg', '.png'), pred)
    infer, pixel_infer = types.ModuleType('infer'), types.ModuleType('pixel_infer')
    infer.main = pixel_infer.main = predictor

    for mod in (cv2, skimage, measure, joblib, tqdm, infer, pixel_infer):
        sys.modules[mod.__name__] = mod


def _blob_mask(rs):
    """A {0, 255} map with large blobs, islands smaller than 30 pixels and holes smaller than 30 pixels."""
    m = np.zeros((H, W), dtype=np.uint8)
    m[10:70, 8:60] = 255
    m[85:140, 50:125] = 255
    m[20:24, 20:25] = 0            # a hole of 20 pixels
    m[40:50, 30:40] = 0            # a hole of 100 pixels: stays
    m[100:103, 70:73] = 0          # 9
    m[5:8, 100:104] = 255          # an island of 12
    m[75:81, 5:10] = 255           # 30: stays (the test is <)
    m[76:78, 100:102] = 255        # 4
    m[144, 3] = 255
    for _ in range(12):            # diagonal contacts: connectivity 8 matters
        y, x = rs.randint(1, H - 1), rs.randint(1, W - 1)
        m[y, x] = 255
        m[y + 1, x + 1] = 255
    return m


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', default='/root/reference')
    ap.add_argument('--out', default=str(ROOT / 'tests' / 'golden' / 'dp2019.npz'))
    a = ap.parse_args(argv)
    script = Path(a.reference) / 'test_dp2019_pipeline.py'
    rs = np.random.RandomState(2019)
    store = {}
    _install_standins(store, rs)
    slide = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    mask = (rs.rand(H, W) < 0.4).astype(np.uint8) * 255

    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp) / 'slides'
        (root / 'images').mkdir(parents=True)
        (root / 'masks').mkdir()
        ckpt = Path(tmp) / 'record' / 'checkpoints' / 'ckpt.pth'
        ckpt.parent.mkdir(parents=True)
        import cv2
        cv2.imwrite(root / 'images' / 'positive-0.jpg', slide)
        cv2.imwrite(root / 'masks' / 'positive-0.png', mask)
        argv0, cwd = sys.argv, os.getcwd()
        sys.argv = [str(script), str(root), '-c', str(ckpt), '-p', str(P)]
        sys.path.insert(0, str(script.parent))
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                ref = runpy.run_path(str(script), run_name='__main__')
        finally:
            sys.argv = argv0
            sys.path.remove(str(script.parent))
            os.chdir(cwd)

        patch_dir = root.parent / 'slides-patches'
        results_dir = ckpt.parent.parent / 'results-for-ckpt.pth'
        corners, patches, mask_patches, preds = [], [], [], []
        for path in sorted((patch_dir / 'images').iterdir()):
            _, x, y = path.stem.split('-')
            corners.append((int(x), int(y)))
            patches.append(store[str(path)])
            mask_patches.append(store[str(patch_dir / 'masks' / path.name.replace('.jpg', '.png'))])
            preds.append(store[str(results_dir / path.name.replace('.jpg', '.png'))])
        # the reference's own stitch of exactly these prediction patches, through its combine_single
        combined = ref['combine_single'](sorted(results_dir.glob('0-*')), (H, W))
        assert np.array_equal(combined, store[str(ckpt.parent.parent / 'combined-results-for-ckpt.pth' / 'positive-0.png')])

    out = {'slide': slide, 'mask': mask, 'patch_size': np.int64(P), 'corners_xy': np.array(corners, dtype=np.int64),
           'patches': np.stack(patches), 'mask_patches': np.stack(mask_patches), 'pred_patches': np.stack(preds),
           'combined': combined}
    # accuracy / dice, both polarities, on three pairs (one all-background)
    pairs = [(combined.astype(np.uint8), mask),
             ((rs.rand(H, W) < 0.7).astype(np.uint8) * 255, (rs.rand(H, W) < 0.2).astype(np.uint8) * 255),
             (np.zeros((H, W), dtype=np.uint8), np.zeros((H, W), dtype=np.uint8))]
    scores = np.zeros((len(pairs), 2, 2))
    for i, (pred, gt) in enumerate(pairs):
        out[f'pair{i}_pred'], out[f'pair{i}_gt'] = pred, gt
        for neg in (0, 1):
            p_, g_ = (255 - pred, 255 - gt) if neg else (pred, gt)      # compute_metrics(negative=True)
            scores[i, neg] = ref['accuracy'](p_, g_), ref['dice'](p_, g_)
    out['scores'] = scores
    blob = _blob_mask(rs)
    out['blob'] = blob
    out['blob_post30'] = ref['postprocess'](blob.copy(), threshold=30)
    np.savez_compressed(a.out, **out)
    print(f'{a.out}: {os.path.getsize(a.out)} bytes; {len(corners)} patches, corners {corners}')


if __name__ == '__main__':
    main()
