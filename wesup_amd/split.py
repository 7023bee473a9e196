"""Splitting touching objects of a predicted mask: distance seeds, label growth, cuts.

  python -m wesup_amd.split PRED_DIR OUT_DIR --radius R [--gpu] [--labels] [--geojson DIR [--simplify PX]] [--measure CSV]

Every object-level metric takes an object to be an 8-connected component of the mask, so two glands whose predictions touch
count as one.  ``split_objects`` separates them: the pixels whose whole open disc of radius ``radius`` is foreground are the
seeds, the seeds' labels grow over the rest of the mask in synchronous rounds, and a one-pixel cut is taken where two labels meet.

The functions here are the definition, in numpy and in integers only; the device path (csrc/split.hip, ``ops.split_objects``) is
held to them bit for bit."""
import argparse
from pathlib import Path

import numpy as np

from .utils import metrics as M

MAX_CAP = 255 * 255
_FAR = 255                       # a column distance of "none within reach"


def _check_radius(radius):
    radius = int(radius)
    if not 1 <= radius <= 255:
        raise ValueError(f'radius {radius}: expected 1 .. 255')
    return radius


def edt_sq_host(mask, cap):
    """Capped squared distance map, int32: 0 where ``mask`` is 0, elsewhere min(cap, |p - z|^2 over the background pixels z of the
    same image).  Pixels outside the image are not background (scipy.ndimage.distance_transform_edt's convention); (H,W) or
    (B,H,W); 1 <= cap <= 65025.  Two passes: the distance to the nearest background pixel of the column, then the minimum over
    the offsets dx with dx^2 < cap of dx^2 + that distance^2."""
    cap = int(cap)
    if not 1 <= cap <= MAX_CAP:
        raise ValueError(f'cap {cap}: expected 1 .. {MAX_CAP}')
    F = np.asarray(mask) != 0
    if F.ndim == 3:
        return np.stack([edt_sq_host(f, cap) for f in F]) if len(F) else np.zeros(F.shape, np.int32)
    if F.ndim != 2:
        raise ValueError(f'mask: expected (H,W) or (B,H,W), got {F.shape}')
    H, W = F.shape
    dmax = 0
    while (dmax + 1) ** 2 < cap:
        dmax += 1
    g = np.where(F, _FAR, 0).astype(np.int64)
    for d in range(1, dmax + 1):                   # nearest zero of the column at distance d, above or below
        hit = np.zeros((H, W), bool)
        hit[d:] |= ~F[:-d]
        hit[:-d or None] |= ~F[d:]
        g[(g == _FAR) & hit] = d
    best = np.minimum(g * g, cap)
    for dx in range(1, dmax + 1):
        sq = np.full((H, W), _FAR * _FAR, np.int64)
        sq[:, dx:] = g[:, :-dx] ** 2
        sq[:, :-dx or None] = np.minimum(sq[:, :-dx or None], g[:, dx:] ** 2)
        best = np.minimum(best, dx * dx + sq)
    return best.astype(np.int32)


def _shifted(L, dy, dx):
    """L[y + dy, x + dx], 0 outside."""
    H, W = L.shape
    out = np.zeros_like(L)
    ys, yd = (slice(dy, None), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, None))
    xs, xd = (slice(dx, None), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, None))
    out[yd, xd] = L[ys, xs]
    return out


_N4 = ((-1, 0), (1, 0), (0, -1), (0, 1))
_N8 = _N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def label_grow_host(mask, seeds, return_rounds=False):
    """Grow the positive labels of ``seeds`` over the foreground of ``mask`` in synchronous rounds k = 1, 2, ...: round k looks at
    the 4-neighbourhood when k is odd and at the 8-neighbourhood when k is even; every foreground pixel of label 0 takes the
    smallest positive label among that round's neighbours as they stood before the round.  Labelled pixels keep their label, the
    background stays 0 (seeds there and seeds <= 0 count as no label).  Rounds run in pairs and growth stops after the first pair
    that changes nothing -> int32 labels (and the number of rounds run)."""
    F = np.asarray(mask) != 0
    S = np.asarray(seeds)
    if F.shape != S.shape:
        raise ValueError(f'mask {F.shape} and seeds {S.shape} differ')
    if F.ndim == 3:
        res = [label_grow_host(f, s, True) for f, s in zip(F, S)]
        L = np.stack([r[0] for r in res]) if res else np.zeros(F.shape, np.int32)
        return (L, max([r[1] for r in res], default=0)) if return_rounds else L
    L = np.where(F & (S > 0), S, 0).astype(np.int64)
    big = np.iinfo(np.int64).max
    k = 0
    while True:
        changed = False
        for nbrs in (_N4, _N8):
            k += 1
            m = np.full(L.shape, big)
            for dy, dx in nbrs:
                n = _shifted(L, dy, dx)
                m = np.where(n > 0, np.minimum(m, n), m)
            take = F & (L == 0) & (m != big)
            if take.any():
                L = np.where(take, m, L)
                changed = True
        if not changed:
            break
    L = L.astype(np.int32)
    return (L, k) if return_rounds else L


def label_cut_host(mask, labels):
    """uint8 {0, 1}: 0 on the background and where a pixel's label a > 0 has an 8-neighbour with a label 0 < b < a."""
    F = np.asarray(mask) != 0
    L = np.asarray(labels).astype(np.int64)
    if F.ndim == 3:
        return np.stack([label_cut_host(f, l) for f, l in zip(F, L)]) if len(F) else np.zeros(F.shape, np.uint8)
    cut = np.zeros(F.shape, bool)
    for dy, dx in _N8:
        n = _shifted(L, dy, dx)
        cut |= (n > 0) & (n < L)
    return (F & ~((L > 0) & cut)).astype(np.uint8)


def split_objects(mask, radius, device=None, return_labels=False):
    """Binary mask (H,W) or (B,H,W) -> uint8 {0, 1} mask of the same shape whose 8-connected components are the separated
    objects: seeds = the components of {capped squared distance >= radius^2}, grown over the mask, cut where two labels meet.
    ``radius`` 1 .. 255; radius 1 is the identity.  With ``device`` the same on the GPU (ops.split_objects).

    The result lies inside the mask, no component of it carries two labels and components without a seed come back unchanged.
    No seed pixel is cut as long as different seeds lie more than 3 pixels (Chebyshev) apart; two cores closer than that -- a
    neck a pixel or two narrower than the cores -- lose a pixel of the larger label, and are separated all the same."""
    radius = _check_radius(radius)
    if device is not None:
        import torch
        from . import ops
        m = torch.tensor(np.asarray(mask) != 0).to(device).to(torch.uint8).contiguous()
        with torch.cuda.device(m.device):
            res = ops.split_objects(m, radius, return_labels=return_labels)
        return tuple(r.cpu().numpy() for r in res) if return_labels else res.cpu().numpy()
    F = np.asarray(mask) != 0
    r2 = radius * radius
    core = edt_sq_host(F, r2) >= r2
    seeds = np.stack([M.label(c) for c in core]) if F.ndim == 3 else M.label(core)
    L = label_grow_host(F, seeds.astype(np.int32))
    out = label_cut_host(F, L)
    return (out, L) if return_labels else out


def split_directory(pred_dir, out_dir, radius, device=None, labels=False, log=print, geojson=None, measure=None, simplify=None):
    """Split every 0/255 mask (``*.png``, ``*.bmp``) of ``pred_dir`` into ``out_dir`` (masks x 255; with ``labels`` also the
    instance map -- the 8-connected components of the result in raster order -- as ``<stem>_labels.png``, 16 bit; with
    ``geojson`` the outlines of the split instances as ``<stem>.geojson`` in that directory; with
    ``measure`` the measurements of the split instances of all masks as that csv file; with ``simplify`` the
    outlines are simplified within that many pixels, DESIGN.md 3.24, and what that changed is logged)."""
    if simplify is not None and geojson is None:
        raise ValueError('simplify: the tolerance of the outlines that geojson writes')
    from PIL import Image
    pred_dir, out_dir = Path(pred_dir).expanduser(), Path(out_dir).expanduser()
    out_dir.mkdir(parents=True, exist_ok=True)
    paths = sorted(p for e in ('*.bmp', '*.png') for p in pred_dir.glob(e))
    rows = []
    if measure is not None:
        from . import measure as measure_mod
    for path in paths:
        a = np.asarray(Image.open(path))
        a = a[..., 0] if a.ndim == 3 else a
        out = split_objects(a, radius, device)
        Image.fromarray((out * 255).astype(np.uint8)).save(out_dir / path.name)
        n_before, inst = int(M.label(a).max()), M.label(out)
        if labels:
            if inst.max() > 65535:
                raise ValueError(f'{path.name}: {int(inst.max())} objects do not fit a 16-bit instance map')
            Image.fromarray(inst.astype(np.uint16)).save(out_dir / (path.stem + '_labels.png'))
        if geojson is not None:
            from . import contour
            if simplify is None:
                polys = contour.polygons(*contour.trace(inst.astype(np.int32), device)[:2])
            else:
                stats = {}
                polys = contour.label_polygons(inst.astype(np.int32), device, simplify=simplify, stats=stats)
                log(f'{path.name}: ' + contour.simplify_log(stats, simplify))
            contour.write_geojson(Path(geojson).expanduser() / (path.stem + '.geojson'), polys)
        if measure is not None:
            rows += measure_mod.object_rows(inst.astype(np.int32), path.name, device)[0]
        log(f'{path.name}: {n_before} -> {int(inst.max())} objects')
    if measure is not None:
        measure_mod.write_csv(measure, rows)
    return paths


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('pred_dir', help='directory of 0/255 masks (*.png, *.bmp)')
    ap.add_argument('out_dir', help='receives the split masks x 255 under the same names')
    ap.add_argument('--radius', type=int, required=True, help='seed radius in pixels, 1 .. 255')
    ap.add_argument('--gpu', action='store_true', help='split on the device (ops.split_objects)')
    ap.add_argument('-d', '--device', default='cuda')
    ap.add_argument('--labels', action='store_true', help='also write the instance maps as 16-bit <stem>_labels.png')
    ap.add_argument('--geojson', default=None, metavar='DIR', help='write the outlines of the split instances here as <stem>.geojson')
    ap.add_argument('--measure', default=None, metavar='CSV', help='write the measurements of the split instances, one row per object')
    ap.add_argument('--simplify', type=float, default=None, metavar='PX', help='simplify the outlines of --geojson within this many pixels')
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    _check_radius(a.radius)
    split_directory(a.pred_dir, a.out_dir, a.radius, a.device if a.gpu else None, a.labels, geojson=a.geojson, measure=a.measure,
                    **({} if a.simplify is None else {'simplify': a.simplify}))


if __name__ == '__main__':
    main()
