"""Golden outputs of the reference's data-preparation scripts (development machine only: it needs the reference checkout).

Runs ``scripts/generate_points.py``, ``scripts/generate_spl_masks.py`` and ``scripts/search_slic_params.py`` unmodified, by path,
and records what their own code produces -> ``tests/golden/prepare.npz`` (a few tens of KB).  Their absent imports get stand-in
modules, the method of ``tools/make_slide_golden.py``: ``skimage.segmentation.slic`` returns a label map made here and recorded
with the outputs, ``skimage.measure.label`` is ``scipy.ndimage.label`` with the full 3 x 3 structure, ``skimage.io.imread`` goes
through PIL, ``fire.Fire`` calls the function with the arguments set here, ``joblib`` runs its jobs one after the other and
``tqdm`` hands its items on in sorted order.

What the fixture holds, and what tests/test_prepare_*.py assert to be in it:
  * ``_generate_points`` on three masks under ``np.random.seed``: a ring whose six centre tries all miss, a 16 x 16 mask whose
    background has its centroid near a corner so that a wrapped NEGATIVE candidate is hit and returned as drawn (the seed is
    searched for), and a mask of many regions at a ratio that asks for several points per region.  The masks go in as int64:
    under numpy >= 2 the script's ``np.c_[x, y, class_label]`` with a uint8 class would come out as uint8 and lose a negative x;
  * both ``__main__`` blocks of generate_points.py and generate_spl_masks.py on one data root of two images: the csv texts and the
    spl-masks;
  * search_slic_params.py's ``__main__`` on a root of two images and 2 x 2 parameter pairs: the printed lines, every label map
    that ``slic`` returned, ``run_param_group`` per image and pair, ``read_image`` of the odd-sized files and ``_list_images``.
    Every label map holds a two-pixel superpixel over mask values (0, 1) -- a tie with an even quotient --, one over (1, 2) -- an
    odd quotient -- and skips one id.

    python tools/make_prepare_golden.py [--reference DIR] [--out tests/golden/prepare.npz]
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

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
AREAS, COMPACTNESSES = (50, 60), (10, 20)
POINT_RATIO_MAIN = 0.01


def _install_standins(state):
    from PIL import Image
    from scipy import ndimage

    skimage = types.ModuleType('skimage')
    segmentation, measure, sio = (types.ModuleType('skimage.' + n) for n in ('segmentation', 'measure', 'io'))
    segmentation.slic = lambda img, n_segments=100, compactness=10.0, **k: state['slic'](img, n_segments, compactness)
    measure.label = lambda a: ndimage.label(np.asarray(a) != 0, structure=np.ones((3, 3), dtype=np.int32))[0]
    sio.imread = lambda path: np.array(Image.open(path))
    skimage.segmentation, skimage.measure, skimage.io = segmentation, measure, sio

    fire = types.ModuleType('fire')
    fire.Fire = lambda fn: fn(*state['fire_args'])

    joblib = types.ModuleType('joblib')
    joblib.Parallel = lambda *a, **k: (lambda jobs: [job() for job in jobs])
    joblib.delayed = lambda fn: (lambda *a, **k: (lambda: fn(*a, **k)))

    tqdm = types.ModuleType('tqdm')
    tqdm.tqdm = lambda it, **k: sorted(it)

    for mod in (skimage, segmentation, measure, sio, fire, joblib, tqdm):
        sys.modules[mod.__name__] = mod


def _run_main(script, argv):
    argv0 = sys.argv
    sys.argv = [str(script)] + [str(a) for a in argv]
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            runpy.run_path(str(script), run_name='__main__')
    finally:
        sys.argv = argv0
    return out.getvalue()


def ring_mask():
    """Class 1: a square ring with a 16 x 16 hole (every centre candidate, centroid +-5, falls into the hole) and a 3 x 3 island;
    class 2: a blob that touches the border."""
    m = np.zeros((48, 56), dtype=np.uint8)
    m[6:28, 8:30] = 1
    m[9:25, 11:27] = 0
    m[40:43, 5:8] = 1
    m[30:48, 40:56] = 2
    return m


def wrap_mask():
    """Background = a 6 x 6 block in the top left corner and a 2 x 2 block in the bottom right one: its centroid is (4, 4), so the
    candidate (-1, -1) wraps to the far corner and is inside."""
    m = np.ones((16, 16), dtype=np.uint8)
    m[:6, :6] = 0
    m[14:, 14:] = 0
    return m


def many_mask(rs):
    """A few hundred regions of 1 to 50 pixels of two classes, some on the border, diagonal contacts included."""
    m = np.zeros((90, 110), dtype=np.uint8)
    for _ in range(260):
        h, w = rs.randint(1, 8), rs.randint(1, 8)
        y, x = rs.randint(0, 90 - h + 1), rs.randint(0, 110 - w + 1)
        m[y:y + h, x:x + w] = rs.randint(1, 3)
    return m


def band_mask(rs, H, W):
    """Vertical bands of the values 0..3 with some noise: neighbours (0, 1) and (1, 2) exist in every row."""
    m = np.repeat((np.arange(W) * 8 // W % 4).astype(np.uint8)[None], H, axis=0)
    noise = rs.rand(H, W) < 0.08
    m[noise] = rs.randint(0, 4, int(noise.sum()))
    return m


def _pair_at(mask, a, b, skip=0):
    ys, xs = np.where((mask[:, :-1] == a) & (mask[:, 1:] == b))
    return int(ys[skip]), int(xs[skip])


def search_map(mask, index, n_segments, compactness):
    """The label map the stand-in slic returns: a Voronoi map, then two two-pixel superpixels over (0, 1) and (1, 2), one id
    skipped and the last id on a single pixel."""
    from wesup_amd import synth
    H, W = mask.shape
    g = max(2, int(round(np.sqrt(n_segments))))
    lab = synth.voronoi_labels(1000 * index + 7 * n_segments + int(compactness), H, W, g).astype(np.int64)
    n = int(lab.max()) + 1
    y, x = _pair_at(mask, 0, 1, skip=3)
    lab[y, x:x + 2] = n                                      # sum 1, count 2: 0.5 -> 0
    y, x = _pair_at(mask, 1, 2, skip=5)
    lab[y, x:x + 2] = n + 1                                  # sum 3, count 2: 1.5 -> 2
    lab[H - 1, W - 1] = n + 3                                # n + 2 has no pixel
    return lab


def main(argv=None):
    from PIL import Image
    from wesup_amd import synth
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', default='/root/reference')
    ap.add_argument('--out', default=str(ROOT / 'tests' / 'golden' / 'prepare.npz'))
    a = ap.parse_args(argv)
    scripts = Path(a.reference) / 'scripts'
    state = {}
    _install_standins(state)
    out = {}

    # ---- _generate_points, called directly
    gp = runpy.run_path(str(scripts / 'generate_points.py'), run_name='reference_generate_points')
    rs = np.random.RandomState(2024)
    cases = {'ring': (ring_mask(), 1e-4, 3), 'wrap': (wrap_mask(), 0.03, None), 'many': (many_mask(rs), 0.1, 11)}
    for name, (mask, ratio, seed) in cases.items():
        if seed is None:                                     # the first seed under which a negative candidate is the hit
            for seed in range(100000):
                np.random.seed(seed)
                if (gp['_generate_points'](mask.astype(np.int64), point_ratio=ratio)[:, :2] < 0).any():
                    break
            else:
                raise SystemExit('no seed gives a wrapped negative candidate')
        np.random.seed(seed)
        pts = gp['_generate_points'](mask.astype(np.int64), point_ratio=ratio)
        out[f'points_{name}_mask'], out[f'points_{name}_ratio'] = mask, np.float64(ratio)
        out[f'points_{name}_seed'], out[f'points_{name}'] = np.int64(seed), pts.astype(np.int64)
        print(f'points/{name}: seed {seed}, {len(pts)} points')

    with tempfile.TemporaryDirectory() as tmp:
        # ---- the two __main__ blocks on one data root
        root = Path(tmp) / 'data'
        (root / 'images').mkdir(parents=True)
        (root / 'masks').mkdir()
        sizes = {'a': (40, 52), 'b': (45, 37)}
        spl_maps = {}
        for i, (stem, (H, W)) in enumerate(sizes.items()):
            img = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
            mask = np.zeros((H, W), dtype=np.uint8)
            mask[8:30, 6:25] = 1
            mask[12:18, 10:16] = 0
            mask[33:38, 20:34] = 1
            if i:
                mask[2:6, 28:35] = 2
            Image.fromarray(img).save(root / 'images' / f'{stem}.png')
            Image.fromarray(mask).save(root / 'masks' / f'{stem}.png')
            out[f'root_{stem}_image'], out[f'root_{stem}_mask'] = img, mask
            spl_maps[(H, W)] = synth.voronoi_labels(50 + i, H, W, 6).astype(np.int64) + 1       # (skimage's ids start at 1)
            out[f'root_{stem}_segments'] = spl_maps[(H, W)]
        seed = 7
        np.random.seed(seed)
        _run_main(scripts / 'generate_points.py', [root, '-p', POINT_RATIO_MAIN])
        out['root_seed'], out['root_ratio'] = np.int64(seed), np.float64(POINT_RATIO_MAIN)
        out['root_points_dir'] = np.array(f'points-{POINT_RATIO_MAIN}')
        for stem, (H, W) in sizes.items():
            text = (root / f'points-{POINT_RATIO_MAIN}' / f'{stem}.csv').read_bytes()
            rows = np.array([[int(v) for v in line.split(',')] for line in text.decode().split()], dtype=np.int64)
            assert (rows >= 0).all() and (rows[:, 0] < W).all() and (rows[:, 1] < H).all(), 'a uint8 row would have wrapped'
            out[f'root_{stem}_csv'] = np.frombuffer(text, dtype=np.uint8)
        state['slic'] = lambda img, n_segments, compactness: spl_maps[img.shape[:2]]
        state['fire_args'] = (str(root), 3)                  # n_classes = 3
        _run_main(scripts / 'generate_spl_masks.py', [])
        for stem in sizes:
            out[f'root_{stem}_spl'] = np.load(root / f'spl-masks-{POINT_RATIO_MAIN}' / f'{stem}.npy')

        # ---- search_slic_params.py
        root2 = Path(tmp) / 'search'
        (root2 / 'images').mkdir(parents=True)
        (root2 / 'masks').mkdir()
        full = {'a': (51, 67), 'b': (46, 59)}                # odd sizes: int() of the halves
        for stem, (H, W) in full.items():
            img = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
            mask = band_mask(rs, H, W)
            Image.fromarray(img).save(root2 / 'images' / f'{stem}.png')
            Image.fromarray(mask).save(root2 / 'masks' / f'{stem}.png')
            out[f'search_{stem}_image'], out[f'search_{stem}_mask'] = img, mask
        ss = runpy.run_path(str(scripts / 'search_slic_params.py'), run_name='reference_search_slic_params')
        halves, index_of = {}, {}
        for i, stem in enumerate(full):
            img = ss['read_image'](str(root2 / 'images' / f'{stem}.png'))
            mask = ss['read_image'](str(root2 / 'masks' / f'{stem}.png'), mode=Image.NEAREST)
            out[f'search_{stem}_image_half'], out[f'search_{stem}_mask_half'] = img, mask
            halves[stem], index_of[img.shape[:2]] = (img, mask), i
        recorded = {}

        def slic(img, n_segments, compactness):
            i = index_of[img.shape[:2]]
            lab = search_map(halves[list(full)[i]][1], i, n_segments, compactness)
            recorded[(i, n_segments, compactness)] = lab
            return lab
        state['slic'] = slic
        text = _run_main(scripts / 'search_slic_params.py', [root2, '-a', ','.join(map(str, AREAS)), '-c',
                                                             ','.join(map(str, COMPACTNESSES))])
        out['search_lines'] = np.array(text.splitlines())
        out['search_areas'], out['search_compactnesses'] = np.array(AREAS), np.array(COMPACTNESSES)
        accs = np.zeros((len(full), len(AREAS), len(COMPACTNESSES)))
        for i, stem in enumerate(full):
            img, mask = halves[stem]
            for j, area in enumerate(AREAS):
                for k, comp in enumerate(COMPACTNESSES):
                    accs[i, j, k] = ss['run_param_group'](img, mask, area, comp)
                    lab = recorded[(i, int(img.shape[0] * img.shape[1] / area), comp)]
                    out[f'search_{stem}_segments_{area}_{comp}'] = lab.astype(np.int32)
        out['search_accs'] = accs
        # the listing: extensions and order
        listing = Path(tmp) / 'listing'
        listing.mkdir()
        for name in ('b.png', 'a.jpg', 'c.bmp', 'd.jpeg', 'e.txt', 'A.png', 'f.PNG', 'a.png'):
            (listing / name).touch()
        out['listing_files'] = np.array(sorted(os.listdir(listing)))
        out['listing'] = np.array([os.path.basename(p) for p in ss['_list_images'](str(listing))])

    np.savez_compressed(a.out, **out)
    print(f'{a.out}: {os.path.getsize(a.out)} bytes, {len(out)} arrays')
    print('\n'.join(out['search_lines']))


if __name__ == '__main__':
    main()
