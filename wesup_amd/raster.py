"""Vector annotations in: exact polygon fill and a GeoJSON reader, the inverse of contour.py.

  python -m wesup_amd.raster ANN_DIR OUT_DIR (--images DIR | --shape H W) [--gpu] [--labels | --classes NAME,NAME,...]
                             [--scale S] [--offset X Y] [--points DIR]

Coordinates are fixed point with 8 fractional bits: one pixel is 256 units.  Pixel (r, c) covers [c, c+1] x [r, r+1] as in
contour.py; its centre is (Xc, Yc) = (256 c + 128, 256 r + 128).  A real coordinate is converted once, on the host and in float64:
fx = floor(((x - offset) / scale) * 256 + 0.5), refused when |fx| > 2^28.  A *feature* is one annotation: a list of rings (outer
rings, holes and the parts of a MultiPolygon alike), an image index and a class; a ring is a cyclic list of n >= 1 vertices.

An edge, its ends ordered so that y0 < y1 (horizontal edges never count), *counts* for a pixel iff

    y0 <= Yc < y1   and   (x1 - x0)(Yc - y0) <= (Xc - x0)(y1 - y0)

and a feature covers a pixel iff an odd number of its edges counts: tops and left sides are inclusive, bottoms and right sides
exclusive.  A pixel's label is 1 + the largest index among the features of its image that cover it, 0 if none does; a class map is
values[label - 1].  In scanline form an edge toggles, in every centre row r with y0 <= Yc < y1, the columns from

    c* = ceil((N - 128 D) / (256 D)),   N = x0 D + (x1 - x0)(Yc - y0),   D = y1 - y0

on (floor-semantics division; clamped to 0 from below, dropped at W).  ``fill_host`` is this scanline form in numpy; the device
path (csrc/raster.hip, ``ops.polygon_fill``) is held to it bit for bit, and tests/_rasterref.py restates the crossing count."""
import argparse
import collections
import csv
import json
import re
from pathlib import Path

import numpy as np

FRAC_BITS = 8
ONE = 1 << FRAC_BITS
HALF = ONE >> 1
COORD_MAX = 2 ** 28

Packed = collections.namedtuple('Packed', 'verts ring_first feature_first_ring feature_image values')


def to_fixed(xy, scale=1.0, offset=(0, 0)):
    """Real (x, y) coordinates (n, 2) -> int32 fixed point: floor(((x - offset) / scale) * 256 + 0.5) in float64; ValueError for a
    coordinate that is not finite or lands outside +-2^28."""
    a = np.asarray(xy, np.float64).reshape(-1, 2)
    fx = np.floor(((a - np.asarray(offset, np.float64)) / float(scale)) * ONE + 0.5)
    if not np.isfinite(fx).all() or (np.abs(fx) > COORD_MAX).any():
        raise ValueError(f'coordinates outside the fixed-point range (|x| <= {COORD_MAX // ONE} pixels after scale and offset)')
    return fx.astype(np.int32)


def _rings_of(feat):
    """The fixed-point rings of a feature dict: ``rings_fixed`` (int fixed point, as read_geojson gives), ``rings`` (real pixel
    coordinates) or ``outer`` + ``holes`` (the integer corners of contour.polygons, multiplied by 256)."""
    if 'rings_fixed' in feat:
        out = [np.asarray(r, np.int64).reshape(-1, 2) for r in feat['rings_fixed']]
        if any((np.abs(r) > COORD_MAX).any() for r in out):
            raise ValueError('rings_fixed: coordinates outside +-2^28')
        return [r.astype(np.int32) for r in out]
    if 'rings' in feat:
        return [to_fixed(r) for r in feat['rings']]
    if 'outer' in feat:
        return [to_fixed(np.asarray(r, np.int64)) for r in [feat['outer']] + list(feat.get('holes', ()))]
    raise ValueError(f'a feature needs rings, rings_fixed or outer / holes: {sorted(feat)}')


def pack(features):
    """Feature dicts {image?, rings | rings_fixed | outer + holes, class?} -> Packed(verts (V, 2) int32, ring_first (R + 1,),
    feature_first_ring (F + 1,), feature_image (F,) int32, values (F,) uint8: the classes, 1 where none is given), in the order
    of the list.  The dicts of contour.polygons / mask_polygons / classmap_polygons are accepted as they are."""
    verts, ring_first, ffr, img, val = [np.zeros((0, 2), np.int32)], [0], [0], [], []
    for feat in features:
        for r in _rings_of(feat):
            verts.append(r)
            ring_first.append(ring_first[-1] + len(r))
        ffr.append(len(ring_first) - 1)
        img.append(int(feat.get('image', 0)))
        k = int(feat.get('class', 1))
        if not 0 <= k <= 255:
            raise ValueError(f'class {k}: class maps are uint8')
        val.append(k)
    if ring_first[-1] >= 2 ** 31:
        raise ValueError('more than 2^31 vertices')
    return Packed(np.concatenate(verts).astype(np.int32), np.array(ring_first, np.int32), np.array(ffr, np.int32),
                  np.array(img, np.int32).reshape(-1), np.array(val, np.uint8).reshape(-1))


def _shape3(shape):
    s = tuple(int(v) for v in shape)
    if len(s) not in (2, 3) or min(s) < 1:
        raise ValueError(f'shape: expected (H, W) or (B, H, W), got {shape}')
    return ((1,) + s if len(s) == 2 else s), len(s) == 2


def _ranges(first, n):
    """The indices first[i] .. first[i] + n[i] - 1 of every i, one after the other, and the i of each."""
    owner = np.repeat(np.arange(len(n)), n)
    return first[owner] + (np.arange(int(n.sum())) - (np.cumsum(n) - n)[owner]), owner


def _refused(verts, ring_first, ffr, fimg, B):
    """bool (F,): the features the device refuses (status bit 0): an image index outside [0, B), ring offsets that leave [0, R] or
    decrease, a ring whose vertex offsets leave [0, V] or decrease, a vertex outside +-2^28."""
    R, V = len(ring_first) - 1, len(verts)
    k0, k1 = ffr[:-1].astype(np.int64), ffr[1:].astype(np.int64)
    bad = (k0 < 0) | (k1 < k0) | (k1 > R) | (fimg < 0) | (fimg >= B)
    k0, k1 = np.where(bad, 0, k0), np.where(bad, 0, k1)
    rf = ring_first.astype(np.int64)
    ring_bad = np.concatenate([[0], np.cumsum((rf[:-1] < 0) | (rf[1:] < rf[:-1]) | (rf[1:] > V))])
    bad |= ring_bad[k1] > ring_bad[k0]
    far = np.concatenate([[0], np.cumsum((np.abs(verts.astype(np.int64)) > COORD_MAX).any(1))])
    v0, v1 = np.where(bad, 0, rf[k0]), np.where(bad | (k1 == k0), 0, rf[k1])
    v0 = np.where(k1 == k0, 0, v0)
    return bad | (far[v1] > far[v0])


def fill_host(verts, ring_first, feature_first_ring, feature_image, shape, values=None):
    """The definition in scanline form -> (labels int32, out8 uint8 or None, status): maps of ``shape`` (H, W) or (B, H, W).
    Every edge's toggles (feature, row, c*) are computed at once; sorted, the toggles of a row pair up into the spans the feature
    covers there, and the spans are painted feature by feature, later ones over earlier ones.  Bit 0 of status: a feature with a
    vertex outside +-2^28, an image index outside [0, B) or offsets that decrease or leave their tables was met; it paints
    nothing."""
    (B, H, W), squeeze = _shape3(shape)
    verts = np.asarray(verts, np.int32).reshape(-1, 2)
    ring_first = np.asarray(ring_first, np.int32).reshape(-1)
    ffr = np.asarray(feature_first_ring, np.int32).reshape(-1)
    fimg = np.asarray(feature_image, np.int32).reshape(-1)
    F = len(fimg)
    if len(ffr) != F + 1 or len(ring_first) < 1:
        raise ValueError('feature_first_ring holds F + 1 offsets, ring_first R + 1')
    labels = np.zeros((B, H, W), np.int32)
    refused = _refused(verts, ring_first, ffr, fimg, B)
    status = int(refused.any())
    good = np.flatnonzero(~refused)
    # the rings of the features that paint, their vertices, and every vertex's successor in its ring
    ring, ring_feat = _ranges(ffr[:-1].astype(np.int64)[good], (ffr[1:].astype(np.int64) - ffr[:-1])[good])
    n_ring = ring_first[ring + 1].astype(np.int64) - ring_first[ring]
    vi, owner = _ranges(ring_first[ring].astype(np.int64), n_ring)
    nxt = np.where(vi + 1 == (ring_first[ring + 1].astype(np.int64))[owner], ring_first[ring].astype(np.int64)[owner], vi + 1)
    feat = good[ring_feat][owner]
    p, q = verts[vi].astype(np.int64), verts[nxt].astype(np.int64)
    up = p[:, 1] > q[:, 1]
    x0, x1 = np.where(up, q[:, 0], p[:, 0]), np.where(up, p[:, 0], q[:, 0])
    y0, y1 = np.where(up, q[:, 1], p[:, 1]), np.where(up, p[:, 1], q[:, 1])
    ra = np.maximum((y0 + HALF - 1) >> FRAC_BITS, 0)                     # the first centre row with y0 <= Yc
    rb = np.minimum((y1 + HALF - 1) >> FRAC_BITS, H)                     # ... with y1 <= Yc: the end (horizontal edges: empty)
    row, e = _ranges(ra, np.maximum(rb - ra, 0))
    D = (y1 - y0)[e]
    N = x0[e] * D + (x1 - x0)[e] * (ONE * row + HALF - y0[e])
    cs = np.maximum(-((HALF * D - N) // (ONE * D)), 0)                   # ceil((N - 128 D) / (256 D)), clamped to the left edge
    keep = cs < W                                                        # dropped at W
    feat, row, cs = feat[e][keep], row[keep], cs[keep]
    order = np.lexsort((cs, row, feat))
    feat, row, cs = feat[order], row[order], cs[order]
    # the toggles of one (feature, row), in order, open and close spans in turn; a span left open ends at W
    new = np.ones(len(cs), bool)
    new[1:] = (feat[1:] != feat[:-1]) | (row[1:] != row[:-1])
    start = np.flatnonzero(new)
    pos = np.arange(len(cs)) - np.repeat(start, np.diff(np.append(start, len(cs))))
    last = np.append(new[1:], True)
    opens = pos % 2 == 0
    end = np.where(last, W, np.append(cs[1:], W))
    for f, r, a, b in zip(feat[opens].tolist(), row[opens].tolist(), cs[opens].tolist(), end[opens].tolist()):
        labels[fimg[f], r, a:b] = f + 1
    out8 = None
    if values is not None:
        values = np.asarray(values, np.uint8).reshape(-1)
        if len(values) != F:
            raise ValueError(f'values: {len(values)} entries for {F} features')
        out8 = np.concatenate([np.zeros(1, np.uint8), values])[labels]
    if squeeze:
        labels, out8 = labels[0], (None if out8 is None else out8[0])
    return labels, out8, status


def fill(features, shape, device=None, values=None):
    """Label map int32 of ``shape`` (H, W) / (B, H, W) from feature dicts (``pack``): 1 + the index of the last feature covering a
    pixel.  ``values`` True adds the class map from the features' classes, an array (F,) one from that table: (labels, out8).
    With ``device`` the fill runs on the GPU (ops.polygon_fill); numpy arrays either way."""
    p = pack(features)
    v = None if values is None else (p.values if values is True else np.asarray(values, np.uint8).reshape(-1))
    if device is None:
        labels, out8, status = fill_host(p.verts, p.ring_first, p.feature_first_ring, p.feature_image, shape, v)
    else:
        import torch
        from . import ops
        dev = torch.device(device)
        with torch.cuda.device(dev):
            t = [torch.from_numpy(a).to(dev) for a in p[:4]]
            tv = None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(dev)
            l, o, s = ops.polygon_fill(*t, shape, tv)
            labels, out8, status = l.cpu().numpy(), (None if o is None else o.cpu().numpy()), int(s.item())
    if status:
        raise ValueError('a feature names an image outside the batch')
    return labels if values is None else (labels, out8)


def rings_to_csr(rings, verts):
    """Ring records (R, 12) and vertices (V, 2) as ops.contour_trace leaves them on the device -> (verts * 256, ring_first,
    feature_first_ring, feature_image, feature_label) int32 device tensors for ops.polygon_fill: one feature per (image, label),
    in that order, its rings gathered behind each other.  The vertices never visit the host (one read-back: the feature count)."""
    import torch
    r = rings.long()
    key = (r[:, 0] << 32) | (r[:, 1] & 0xffffffff)
    order = torch.argsort(key, stable=True)
    n = r[order, 3]
    first = torch.cumsum(n, 0) - n
    ring_first = torch.cat([first, n.sum().reshape(1)]).int()
    src = torch.repeat_interleave(r[order, 2] - first, n) + torch.arange(int(verts.shape[0]), device=verts.device)
    k, counts = torch.unique_consecutive(key[order], return_counts=True)
    ffr = torch.cat([torch.zeros(1, dtype=torch.long, device=verts.device), torch.cumsum(counts, 0)]).int()
    return (verts[src] * ONE).int().contiguous(), ring_first, ffr, (k >> 32).int(), (k & 0xffffffff).int()


# ---------------------------------------------------------------- GeoJSON in
_OWN_CLASS = re.compile(r'class (\d+)$')


def _class_of(props, class_names):
    c = (props or {}).get('classification')
    name = c.get('name') if isinstance(c, dict) else c
    if name is None:
        return 1
    name = str(name)
    if class_names is not None:
        names = [str(n) for n in class_names]
        if name not in names:
            raise ValueError(f'unknown class name {name!r} (known: {names})')
        return names.index(name)
    m = _OWN_CLASS.match(name)
    if not m:
        raise ValueError(f'unknown class name {name!r}: give class_names')
    return int(m.group(1))


def _features_of(doc):
    if isinstance(doc, (str, Path)):
        with open(doc) as f:
            doc = json.load(f)
    if isinstance(doc, dict) and doc.get('type') == 'FeatureCollection':
        return list(doc.get('features', ()))
    if isinstance(doc, dict):
        return [doc]
    return list(doc)


def read_geojson(doc_or_path, scale=1.0, offset=(0, 0), class_names=None):
    """A FeatureCollection, a list of Features or one Feature (parsed, or a path) -> (features, points, skipped).  Polygon and
    MultiPolygon geometries become features in file order: {image 0, rings_fixed, class}, every ring of every part in one list,
    the closing vertex dropped, coordinates (x - offset) / scale in fixed point.  Point and MultiPoint geometries become point
    rows (x, y, class) in pixels (float).  Every other geometry type is counted in ``skipped``.  The class is
    properties.classification.name looked up in ``class_names`` (its index; ValueError for an unknown name), without
    ``class_names`` our own export's 'class k' gives k, and an unclassified feature is class 1."""
    return _read(doc_or_path, scale, offset, class_names, True)


def _read(doc_or_path, scale, offset, class_names, classed):
    feats, points, skipped = [], [], 0
    off = np.asarray(offset, np.float64)
    for ft in _features_of(doc_or_path):
        g = (ft.get('geometry') if ft.get('type') == 'Feature' else ft) or {}
        kind = g.get('type')
        if kind in ('Polygon', 'MultiPolygon'):
            parts = [g['coordinates']] if kind == 'Polygon' else g['coordinates']
            rings = []
            for part in parts:
                for r in part:
                    p = np.asarray(r, np.float64).reshape(-1, np.shape(r)[-1] if len(r) else 2)[:, :2]
                    if len(p) > 1 and (p[0] == p[-1]).all():
                        p = p[:-1]
                    if len(p):
                        rings.append(to_fixed(p, scale, offset))
            feats.append({'image': 0, 'rings_fixed': rings, 'class': _class_of(ft.get('properties'), class_names) if classed else 1})
        elif kind in ('Point', 'MultiPoint'):
            k = _class_of(ft.get('properties'), class_names) if classed else 1
            for xy in ([g['coordinates']] if kind == 'Point' else g['coordinates']):
                x, y = (np.asarray(xy[:2], np.float64) - off) / float(scale)
                points.append((float(x), float(y), k))
        else:
            skipped += 1
    return feats, points, skipped


def geojson_to_labels(doc, shape, scale=1.0, offset=(0, 0), device=None):
    """Instance map int32 (H, W): 1 + the index, among the polygon features in file order, of the last one covering the pixel
    (the classes are not looked at)."""
    return fill(_read(doc, scale, offset, None, False)[0], shape, device)


def geojson_to_classes(doc, shape, scale=1.0, offset=(0, 0), class_names=None, device=None):
    """Class-index map uint8 (H, W): the class of the last polygon feature covering the pixel, 0 where none does."""
    return fill(read_geojson(doc, scale, offset, class_names)[0], shape, device, values=True)[1]


def geojson_to_mask(doc, shape, scale=1.0, offset=(0, 0), device=None):
    """bool (H, W): the pixels some polygon feature covers."""
    return geojson_to_labels(doc, shape, scale, offset, device) > 0


def point_rows(points):
    """Point rows (x, y, class) -> (n, 3) int64, the coordinates floored: the rows of a ``points/<stem>.csv``."""
    if not len(points):
        return np.zeros((0, 3), np.int64)
    a = np.asarray(points, np.float64).reshape(-1, 3)
    return np.floor(a).astype(np.int64)


def write_points(path, points):
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, 'w', newline='') as f:
        csv.writer(f).writerows(point_rows(points).tolist())
    return path


def convert_directory(ann_dir, out_dir, images=None, shape=None, device=None, labels=False, classes=None, scale=1.0,
                      offset=(0, 0), points=None, log=print):
    """``<stem>.png`` in ``out_dir`` for every ``<stem>.geojson`` of ``ann_dir``: a class-index uint8 map by default (0 / 1 when
    nothing is classified: what ``masks/`` holds), a 16-bit instance map with ``labels``; ``points`` receives ``<stem>.csv``.  The
    size is that of the image of the same stem in ``images``, or ``shape``."""
    from PIL import Image
    ann_dir, out_dir = Path(ann_dir).expanduser(), Path(out_dir).expanduser()
    out_dir.mkdir(parents=True, exist_ok=True)
    paths = sorted(ann_dir.glob('*.geojson'))
    for path in paths:
        if images is not None:
            hits = sorted(q for q in Path(images).expanduser().glob(path.stem + '.*') if q.suffix.lower() in
                          ('.png', '.jpg', '.jpeg', '.bmp', '.tif', '.tiff'))
            if not hits:
                raise FileNotFoundError(f'{path.name}: no image {path.stem}.* in {images}')
            with Image.open(hits[0]) as im:
                hw = (im.height, im.width)
        else:
            hw = (int(shape[0]), int(shape[1]))
        feats, pts, skipped = _read(path, scale, offset, classes, not labels or points is not None)
        if labels:
            inst = fill(feats, hw, device)
            if inst.max(initial=0) > 65535:
                raise ValueError(f'{path.name}: more than 65535 objects do not fit a 16-bit instance map')
            Image.fromarray(inst.astype(np.uint16)).save(out_dir / (path.stem + '.png'))
        else:
            Image.fromarray(fill(feats, hw, device, values=True)[1]).save(out_dir / (path.stem + '.png'))
        if points is not None:
            write_points(Path(points).expanduser() / (path.stem + '.csv'), pts)
        log(f'{path.name}: {len(feats)} polygons, {len(pts)} points, {skipped} skipped -> {hw[0]} x {hw[1]}')
    return paths


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('ann_dir', help='directory of <stem>.geojson annotations')
    ap.add_argument('out_dir', help='receives <stem>.png')
    ap.add_argument('--images', help='directory of the images: <stem>.* gives the size')
    ap.add_argument('--shape', type=int, nargs=2, metavar=('H', 'W'), help='the size of every map, without images')
    ap.add_argument('--gpu', action='store_true', help='fill on the device (ops.polygon_fill)')
    ap.add_argument('-d', '--device', default='cuda')
    ap.add_argument('--labels', action='store_true', help='write 16-bit instance maps (as split.py --labels does)')
    ap.add_argument('--classes', help='comma-separated class names: the index in the list is the class')
    ap.add_argument('--scale', type=float, default=1.0, help='slide pixels per mask pixel')
    ap.add_argument('--offset', type=float, nargs=2, default=(0.0, 0.0), metavar=('X', 'Y'), help='slide coordinates of the corner of pixel (0, 0)')
    ap.add_argument('--points', help='directory that receives <stem>.csv point files')
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    if (a.images is None) == (a.shape is None):
        raise SystemExit('give one of --images DIR and --shape H W')
    if a.labels and a.classes:
        raise SystemExit('--labels and --classes exclude each other')
    convert_directory(a.ann_dir, a.out_dir, a.images, a.shape, a.device if a.gpu else None, a.labels,
                      a.classes.split(',') if a.classes else None, a.scale, tuple(a.offset), a.points)


if __name__ == '__main__':
    main()
