"""Golden outputs of the reference's painted comparisons and of its CRAG / LUSC evaluation (development machine only: it needs
the reference checkout).

Loads the reference's ``scripts/paint_masks.py`` by path and runs ``scripts/evaluate_crag.py`` and ``scripts/evaluate_pdl1.py``
as ``__main__``, all unmodified, and records what their own functions produce -> ``tests/golden/paint.npz`` (a few tens of KB).
Their absent imports get stand-in modules, the method of ``tools/make_slide_golden.py``: ``skimage.measure.label`` as
``scipy.ndimage.label`` with the full 3 x 3 structure on the non-zero pixels, ``skimage.io`` whose ``imread`` / ``imsave`` return
and capture arrays (a file of the same name is touched, so that the scripts' globs find it), ``joblib`` / ``tqdm`` as plain loops.
The two evaluation scripts glob their ground truth from hard-coded places: ``glob.glob`` sends the absolute one to the temporary
directory, the relative one is met by running there.

    python tools/make_paint_golden.py [--reference DIR] [--out tests/golden/paint.npz]

Painting cases (each at most 96 x 120, so that the reference's loop over every pair of objects finishes):
  ellipses  overlapping random ellipses (wesup_amd.synth.gland_map), the prediction a shifted copy plus strangers;
  many      more than 104 isolated small blobs on each side: ids beyond the palette, colours drawn from the generator;
  no_pred / no_gt   an empty prediction / an empty ground truth;
  edges     hand-built: one predicted object over two ground-truth objects of equal area (the lower id wins), one over a small
            and a large one (the large one wins), one over exactly half of an object (no match), one over six tenths (a match),
            one over nothing, and a ground-truth object nobody covers.
Every case is painted by a freshly loaded module (the generator state right after the palette shuffle); ``seq_*`` are the files
one run of the script itself writes for the five cases plus 'many' swapped in one directory, one generator in file order.

Evaluation: three 160 x 200 pairs with regions and holes on both sides of 5000 and of 2000 pixels (the GlaS rule would give other
maps), every map non-empty after the post-processing."""
import argparse
import contextlib
import glob as glob_module
import io
import os
import runpy
import sys
import tempfile
import time
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
H, W = 96, 120
EH, EW = 160, 200
CRAG_GLOB = '/home/mrc/data/CRAG/test/masks'


def _install_standins(store):
    from scipy import ndimage

    skimage, measure, sio = types.ModuleType('skimage'), types.ModuleType('skimage.measure'), types.ModuleType('skimage.io')
    measure.label = lambda a: ndimage.label(np.asarray(a) != 0, structure=np.ones((3, 3), dtype=np.int32))[0]

    def imsave(dest, array, **kwargs):
        store[os.path.abspath(str(dest))] = np.array(array, copy=True)
        Path(dest).touch()

    def imread(path, **kwargs):
        return store[os.path.abspath(str(path))].copy()        # (evaluate_pdl1.py globs relative paths)
    sio.imread, sio.imsave = imread, imsave
    skimage.measure, skimage.io = measure, sio

    joblib = types.ModuleType('joblib')
    joblib.Parallel = lambda *a, **k: (lambda jobs: [job() for job in jobs])
    joblib.delayed = lambda fn: (lambda *a, **k: (lambda: fn(*a, **k)))

    tqdm = types.ModuleType('tqdm')
    tqdm.tqdm = lambda it, **k: it

    for mod in (skimage, measure, sio, joblib, tqdm):
        sys.modules[mod.__name__] = mod
    return imsave


def _blobs(rs, cells):
    """Isolated blobs of 1 .. 6 pixels, one per chosen cell of a 4 x 4 lattice (a free row and column between neighbours)."""
    m = np.zeros((H, W), dtype=np.uint8)
    for c in cells:
        y, x = 4 * (c // (W // 4)), 4 * (c % (W // 4))
        m[y:y + rs.randint(1, 4), x:x + rs.randint(1, 3)] = 1
    return m


def paint_cases():
    from wesup_amd import synth
    rs = np.random.RandomState(7)
    cases = {}
    G = synth.gland_map(3, H, W, 10, 5, 14)
    S = np.roll(G, 3, axis=(0, 1)) | synth.gland_map(4, H, W, 4, 5, 12)
    cases['ellipses'] = (S, G)
    n_cells = (H // 4) * (W // 4)
    shared = rs.choice(n_cells, 260, replace=False)
    # 130 cells carry a blob in both maps (independent sizes: some cover more than half, some do not), 70 + 60 in one only
    cases['many'] = (_blobs(rs, np.sort(shared[:200])), _blobs(rs, np.sort(np.r_[shared[:130], shared[200:]])))
    cases['no_pred'] = (np.zeros((H, W), np.uint8), G)
    cases['no_gt'] = (S, np.zeros((H, W), np.uint8))
    P, T = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    T[5:15, 5:15] = 1; T[5:15, 20:30] = 1; P[4:16, 4:31] = 1              # two objects of 100 pixels under one: the first wins
    T[5:13, 50:58] = 1; T[5:17, 62:74] = 1; P[3:18, 48:76] = 1            # 64 and 144 pixels under one: the larger, later one wins
    T[40:50, 5:15] = 1; P[40:50, 0:10] = 1                                # exactly 50 of 100 pixels: no match
    T[40:50, 30:40] = 1; P[40:50, 26:36] = 1                              # 60 of 100: a match
    P[70:80, 60:75] = 1                                                   # over nothing
    T[70:90, 90:110] = 1                                                  # covered by nobody
    T[60:64, 5:9] = 1; P[61:65, 6:10] = 1                                 # 9 of 16: a match by one pixel
    cases['edges'] = (P, T)
    return cases


def eval_pairs():
    """(prediction {0, 255}, ground truth as stored) x 3."""
    yy, xx = np.mgrid[0:EH, 0:EW]

    def disc(m, cy, cx, ry, rx, v=1):
        m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = v
    pairs = []
    # 1: a region of 13000 with holes of 1200 (filled by both rules) and 3500 (filled at 5000 only); blobs of 3000 (erased at
    #    5000 only) and 600
    p = np.zeros((EH, EW), np.uint8)
    p[10:110, 10:140] = 1; p[20:50, 20:60] = 0; p[55:105, 60:130] = 0
    p[115:155, 100:175] = 1; p[120:140, 20:50] = 1
    g = np.zeros((EH, EW), np.uint8)
    g[8:112, 12:138] = 1; g[118:152, 105:170] = 2
    pairs.append((p * 255, g))
    # 2: ellipses: 7900 and 5300 (kept), 2800 (erased at 5000 only), 1250 (erased); a hole of 2100 in the first
    p = np.zeros((EH, EW), np.uint8)
    disc(p, 55, 60, 45, 56); disc(p, 60, 60, 23, 29, 0); disc(p, 110, 150, 37, 46); disc(p, 30, 160, 26, 34); disc(p, 140, 40, 18, 22)
    g = np.zeros((EH, EW), np.uint8)
    disc(g, 57, 63, 44, 52, 1); disc(g, 108, 148, 38, 44, 1); disc(g, 30, 158, 25, 30, 1)
    pairs.append((p * 255, g))
    # 3: two squares joined by a diagonal contact (one object of 6160 under 8-connectivity, two below 5000 under 4), a frame
    #    with a hole of 4200 (filled at 5000 only), the ground truth an id map with 255 among the ids
    p = np.zeros((EH, EW), np.uint8)
    p[5:60, 5:60] = 1; p[60:117, 60:115] = 1; p[10:150, 125:195] = 1; p[30:100, 130:190] = 0
    g = np.zeros((EH, EW), np.uint8)
    g[5:60, 5:60] = 1; g[62:117, 62:115] = 3; g[10:150, 125:195] = 255
    pairs.append((p * 255, g))
    return pairs


def run_paint(script, cases, imsave):
    out = {}
    for name, (S, G) in cases.items():
        mod = runpy.run_path(str(script), run_name='paint_masks')          # re-seeds and re-shuffles: a fresh generator per case
        t0 = time.perf_counter()
        pred, gt = mod['paint_pred_and_gt'](S.copy(), G.copy())
        out[f'seconds_{name}'] = np.float64(time.perf_counter() - t0)
        out[f'pred_{name}'], out[f'gt_{name}'] = pred, gt
        out[f'S_{name}'], out[f'G_{name}'] = np.packbits(S != 0), np.packbits(G != 0)
    out['palette'] = np.array(mod['colors'], dtype=np.uint8)
    return out


def run_paint_script(script, cases, store, imsave):
    """The script itself on one directory with the five cases and, last in file order, 'many' again with the two maps swapped
    (its colours come from where the first 'many' left the generator); model name 'wesup', default output directory."""
    out = {}
    cases = dict(cases, zz_many_swapped=cases['many'][::-1])
    with tempfile.TemporaryDirectory() as tmp:
        pred_dir, gt_dir = Path(tmp) / 'run' / 'pred', Path(tmp) / 'run' / 'gt'
        pred_dir.mkdir(parents=True)
        gt_dir.mkdir()
        for i, (name, (S, G)) in enumerate(cases.items()):
            ext = ('png', 'bmp')[i % 2]
            imsave(pred_dir / f'{name}.{ext}', S * 255)
            imsave(gt_dir / f'{name}.{ext}', G)
        argv0 = sys.argv
        sys.argv = [str(script), str(pred_dir), str(gt_dir), '-m', 'wesup']
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                runpy.run_path(str(script), run_name='__main__')
        finally:
            sys.argv = argv0
        names = sorted(p.name for p in (pred_dir.parent / 'paintings').iterdir())
        out['seq_names'] = np.array(names)
        out['seq_inputs'] = np.array(sorted(p.name for p in pred_dir.iterdir()))
        for n in names:
            out[f'seq_{n}'] = store[str(pred_dir.parent / 'paintings' / n)]
    return out


def run_eval(script, pairs, store, imsave, where):
    """One evaluation script as __main__; ``where`` = 'absolute' (evaluate_crag.py) or 'relative' (evaluate_pdl1.py)."""
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        pred_root = tmp / 'results'
        pred_root.mkdir()
        gt_dir = tmp / 'LUSC' / 'test' / 'masks'
        gt_dir.mkdir(parents=True)
        for i, (p, g) in enumerate(pairs):
            imsave(pred_root / f'im{i}.png', p)
            imsave(gt_dir / f'im{i}.png', g)
        real_glob = glob_module.glob

        def redirected(pattern, *a, **k):
            return real_glob(pattern.replace(CRAG_GLOB, str(gt_dir)), *a, **k)
        argv0, cwd = sys.argv, os.getcwd()
        sys.argv = [str(script), str(pred_root)]
        sys.path.insert(0, str(script.parent.parent))
        glob_module.glob = redirected
        os.chdir(tmp)
        buf = io.StringIO()
        try:
            with contextlib.redirect_stdout(buf):
                runpy.run_path(str(script), run_name='__main__')
        finally:
            sys.argv = argv0
            glob_module.glob = real_glob
            sys.path.remove(str(script.parent.parent))
            os.chdir(cwd)
        lines = [l for l in buf.getvalue().splitlines() if ':' in l]
        names = [l.split(':')[0] for l in lines]
        assert names == ['Accuracy', 'Dice', 'Detection F1', 'Object Dice', 'Object Hausdorff'], names
        means = np.array([float(l.split(':')[1]) for l in lines])
        post = [store[str(tmp / 'results-new' / f'im{i}.png')] for i in range(len(pairs))]
    return names, means, post


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', default='/root/reference')
    ap.add_argument('--out', default=str(ROOT / 'tests' / 'golden' / 'paint.npz'))
    a = ap.parse_args(argv)
    scripts = Path(a.reference) / 'scripts'
    store = {}
    imsave = _install_standins(store)

    cases = paint_cases()
    out = run_paint(scripts / 'paint_masks.py', cases, imsave)
    out['cases'] = np.array(list(cases))
    out['shape'] = np.array([H, W], dtype=np.int64)
    out.update(run_paint_script(scripts / 'paint_masks.py', cases, store, imsave))

    pairs = eval_pairs()
    names, crag, post = run_eval(scripts / 'evaluate_crag.py', pairs, store, imsave, 'absolute')
    _, lusc, post2 = run_eval(scripts / 'evaluate_pdl1.py', pairs, store, imsave, 'relative')
    assert all(np.array_equal(x, y) for x, y in zip(post, post2))
    out['eval_names'], out['eval_means_crag'], out['eval_means_lusc'] = np.array(names), crag, lusc
    out['eval_shape'] = np.array([EH, EW], dtype=np.int64)
    out['eval_n'] = np.int64(len(pairs))
    for i, ((p, g), q) in enumerate(zip(pairs, post)):
        assert set(np.unique(q)) == {0, 255}, 'a post-processed map came out empty or full'
        out[f'eval_pred{i}'], out[f'eval_gt{i}'], out[f'eval_post{i}'] = np.packbits(p != 0), g, np.packbits(q != 0)
    np.savez_compressed(a.out, **out)
    print(f'{a.out}: {os.path.getsize(a.out)} bytes')
    for name in cases:
        print(f'  {name}: the reference painted it in {float(out["seconds_" + name]):.3f} s')
    print('  CRAG means', dict(zip(names, crag)))


if __name__ == '__main__':
    main()
