"""Object measurements: moments, shape counts and the exact convex hull of every label of a label map.

  python -m wesup_amd.measure PRED_DIR OUT.csv [--gpu] [--labels] [--classes C] [--min-area A] [--scale S] [--geojson DIR [--simplify PX]]

Coordinates are ``contour.py``'s: pixel (r, c) covers [c, c+1] x [r, r+1], vertices are integer pixel corners (x, y), y downwards.
The input is an int32 label map (H, W) / (B, H, W) with labels 0 .. L; label 0 is background and its row of the table is zero; a
label need not be connected.  ``measure_host`` is the definition: a table (B, L+1, MEASURE_WORDS) int64 whose row of label l holds

    word   content
    0      pixels
    1-5    sum r, sum c, sum r^2, sum r c, sum c^2 over the label's pixels
    6-9    rmin, cmin, rmax, cmax (inclusive); (H, W, -1, -1) for an absent label, whose other words are 0
    10-12  border pixels in the weight classes A, B, C of the 4-neighbourhood perimeter estimator (below)
    13-15  bit-quad counts Q1, Q3, QD over the (H+1)(W+1) pixel corners
    16     hull area x 2 by contour.py's area2 formula: positive, the hull runs counter-clockwise on screen
    17     hull vertices
    18     maximum Feret diameter squared
    19,20  lattice indices y (W+1) + x of the two hull vertices that realise it: among the pairs at the maximum distance the
           smallest (p, q) with p < q
    21     inscribed radius squared: the maximum of ``d2`` over the label's pixels (0 without ``d2``)
    22     pixel index r W + c of the first pixel in raster order that attains it (0 without ``d2``)
    23     index of the label's first hull vertex in ``hull_verts``

``hull_verts`` (V, 2) int32 holds the hulls (x, y) image by image and label by label.  A hull is the convex hull of the corners of
the label's pixels, strict vertices only, from the vertex with the smallest (y, x) down the left side first: counter-clockwise on
screen, as outer rings are.  ``status`` (B,) int32: bit 0 is set by a label outside [0, L], which is skipped and never used as an
index.  H, W <= 32768, so every sum stays below 2^62; L + 1 <= 2^20.

Border classes (words 10-12): ``border`` = the pixels of the label with a 4-neighbour of another label or outside the image;
v = 1 border[p] + 2 (border 4-neighbours) + 10 (border diagonal neighbours); class A: v in {5, 7, 15, 17, 25, 27}, weight 1;
class B: v in {21, 33}, weight sqrt 2; class C: v in {13, 23}, weight (1 + sqrt 2) / 2.  Bit quads (words 13-15): every 2 x 2
window of ``labels == l`` around a pixel corner with exactly one pixel set counts as Q1, with three as Q3, the two diagonal
patterns as QD; the 8-connected Euler number is (Q1 - Q3 - 2 QD) / 4.

``d2`` is an int32 map of squared distances, ``ops.edt_sq_full(labels > 0)`` in ``measure``: the distance to the *background*, not
to a neighbouring label, so two touching labels share one distance map and the inscribed radius of either may reach into the
other.

The device path (csrc/measure.hip, ``ops.object_measure``) is held to ``measure_host`` word for word and vertex for vertex; it finds
the hull from row profiles, ``hull_host`` by Andrew's monotone chain over all pixel corners."""
import argparse
import csv
import math
from pathlib import Path

import numpy as np

MEASURE_WORDS = 24                           # int64 words of a label's row (WESUP_MEASURE_WORDS)
FIELDS = ('pixels', 'sum_r', 'sum_c', 'sum_rr', 'sum_rc', 'sum_cc', 'rmin', 'cmin', 'rmax', 'cmax', 'border_a', 'border_b',
          'border_c', 'q1', 'q3', 'qd', 'hull_area2', 'hull_vertices', 'feret2', 'feret_p', 'feret_q', 'inradius2', 'inradius_pixel',
          'hull_first')
MAX_SIDE = 32768
MAX_LABELS = 1 << 20                         # L + 1 at most
_CLASS_A, _CLASS_B, _CLASS_C = (5, 7, 15, 17, 25, 27), (21, 33), (13, 23)


def _labels3(labels):
    a = np.asarray(labels)
    if a.ndim not in (2, 3) or a.dtype.kind not in 'iub' or a.size == 0:
        raise ValueError(f'labels: expected a non-empty integer (H,W) or (B,H,W) array, got {a.dtype} {a.shape}')
    a = a.astype(np.int64)
    a = a[None] if a.ndim == 2 else a
    if a.shape[1] > MAX_SIDE or a.shape[2] > MAX_SIDE:
        raise ValueError(f'labels: {a.shape[1]} x {a.shape[2]} (sides up to {MAX_SIDE})')
    return a


def hull_host(mask):
    """The convex hull of the corners of the set pixels of ``mask`` (H, W) -> (n, 2) int64 vertices (x, y): Andrew's monotone chain
    over all pixel corners sorted by (y, x), popping while cross <= 0, so only strict vertices stay; the lower chain in (y, x)
    is the left side from the top down, the upper chain the right side back up.  An empty mask has no vertex."""
    r, c = np.nonzero(np.asarray(mask))
    if len(r) == 0:
        return np.zeros((0, 2), np.int64)
    pts = np.unique(np.concatenate([np.stack([r + dy, c + dx], 1) for dy in (0, 1) for dx in (0, 1)]), axis=0)
    pts = [(int(y), int(x)) for y, x in pts]                        # sorted by (y, x)

    def chain(seq):
        out = []
        for p in seq:
            while len(out) >= 2:
                (ou, ov), (au, av) = out[-2], out[-1]
                if (au - ou) * (p[1] - ov) - (av - ov) * (p[0] - ou) <= 0:
                    out.pop()
                else:
                    break
            out.append(p)
        return out

    left, right = chain(pts), chain(pts[::-1])
    ring = left[:-1] + right[:-1]
    return np.array([(x, y) for y, x in ring], np.int64)


def hull_area2(verts):
    """contour.py's area2 of a vertex list (x, y): positive counter-clockwise on screen."""
    v = np.asarray(verts, np.int64).reshape(-1, 2)
    x, y = v[:, 0], v[:, 1]
    return -int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())


def feret_host(verts, W):
    """(d2, p, q): the largest squared distance between two hull vertices and the lattice indices y (W+1) + x of the pair that
    realises it, the smallest (p, q) with p < q among the pairs at that distance."""
    v = np.asarray(verts, np.int64).reshape(-1, 2)
    d = ((v[:, None, :] - v[None, :, :]) ** 2).sum(-1)
    best = int(d.max())
    i, j = np.nonzero(d == best)
    lat = v[:, 1] * (W + 1) + v[:, 0]
    p, q = np.minimum(lat[i], lat[j]), np.maximum(lat[i], lat[j])
    k = np.lexsort((q, p))[0]
    return best, int(p[k]), int(q[k])


def _shape_counts(m):
    """m: a label's mask cut to its box -> (A, B, C, Q1, Q3, QD).  The perimeter classes restate scikit-image's
    ``measure.perimeter(neighborhood=4)`` (border = mask minus its 4-erosion, the 3 x 3 weights [[10, 2, 10], [2, 1, 2],
    [10, 2, 10]], the three groups of sums with weights 1, sqrt 2, (1 + sqrt 2) / 2) FROM MEMORY: scikit-image is not available
    to this project's tests, so the agreement with it is unpinned."""
    p = np.pad(m.astype(bool), 2)
    inner = p[1:-1, 1:-1]
    border = inner & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])           # (h+2, w+2)
    bp = np.pad(border, 1).astype(np.int64)
    v = (bp[1:-1, 1:-1] + 2 * (bp[:-2, 1:-1] + bp[2:, 1:-1] + bp[1:-1, :-2] + bp[1:-1, 2:])
         + 10 * (bp[:-2, :-2] + bp[:-2, 2:] + bp[2:, :-2] + bp[2:, 2:]))
    v = v[border]
    cls = [int(np.isin(v, k).sum()) for k in (_CLASS_A, _CLASS_B, _CLASS_C)]
    q = np.pad(m.astype(np.int64), 1)
    nw, ne, sw, se = q[:-1, :-1], q[:-1, 1:], q[1:, :-1], q[1:, 1:]
    n = nw + ne + sw + se
    qd = (n == 2) & (nw == se) & (nw != ne)
    return cls + [int((n == 1).sum()), int((n == 3).sum()), int(qd.sum())]


def measure_host(labels, L, d2=None):
    """The definition (module docstring): labels (H,W) / (B,H,W) integers, L the largest label of the table, d2 None or an integer
    map of the same shape with values >= 0 -> (table (B, L+1, 24) int64, hull_verts (V, 2) int32, status (B,) int32)."""
    lab3 = _labels3(labels)
    B, H, W = lab3.shape
    L = int(L)
    if L < 0 or L + 1 > MAX_LABELS:
        raise ValueError(f'L = {L}: L + 1 in [1, {MAX_LABELS}]')
    if d2 is not None:
        d3 = np.asarray(d2).astype(np.int64).reshape(lab3.shape)
    table = np.zeros((B, L + 1, MEASURE_WORDS), np.int64)
    table[:, 1:, 6], table[:, 1:, 7], table[:, 1:, 8:10] = H, W, -1
    status = np.zeros(B, np.int32)
    verts, nv = [np.zeros((0, 2), np.int64)], 0
    for b in range(B):
        lab = lab3[b]
        if ((lab < 0) | (lab > L)).any():
            status[b] |= 1
        rr, cc = np.nonzero((lab >= 1) & (lab <= L))
        ll = lab[rr, cc]
        order = np.argsort(ll, kind='stable')
        rr, cc, ll = rr[order], cc[order], ll[order]
        present, start = np.unique(ll, return_index=True)
        for l, s, e in zip(present.tolist(), start.tolist(), start.tolist()[1:] + [len(ll)]):
            r, c = rr[s:e], cc[s:e]
            row = table[b, l]
            row[0] = len(r)
            row[1:6] = r.sum(), c.sum(), (r * r).sum(), (r * c).sum(), (c * c).sum()
            r0, c0, r1, c1 = r.min(), c.min(), r.max(), c.max()
            row[6:10] = r0, c0, r1, c1
            m = lab[r0:r1 + 1, c0:c1 + 1] == l
            row[10:16] = _shape_counts(m)
            hv = hull_host(m) + (c0, r0)
            row[16], row[17] = hull_area2(hv), len(hv)
            row[18:21] = feret_host(hv, W)
            if d2 is not None:
                d = d3[b, r, c]
                k = int(np.argmax(d))                           # the first maximum: the pixels are in raster order
                row[21], row[22] = d[k], r[k] * W + c[k]
            row[23] = nv
            verts.append(hv)
            nv += len(hv)
    return table, np.concatenate(verts).astype(np.int32), status


def measure(labels, L=None, device=None):
    """``measure_host`` with d2 the exact squared distance to the background, or with ``device`` the same from the GPU
    (ops.edt_sq_full, ops.object_measure); numpy arrays either way.  ``labels`` is an array, or on the device path also an int32
    tensor that already lives there.  ``L=None`` takes the largest label of the map (at least 0): from the host array, and for a
    device tensor by one 4-byte read-back in front of the call's own."""
    if device is None:
        from . import surface
        lab3 = _labels3(labels)
        L = max(int(lab3.max()), 0) if L is None else int(L)
        d2 = np.stack([surface.edt_sq_full_host(m) for m in (lab3 > 0)])
        return measure_host(lab3, L, d2)
    import torch
    from . import ops
    if isinstance(labels, torch.Tensor):
        t = labels.to(device)
    else:
        a = np.asarray(labels)
        if a.size and (a.max() > 2 ** 31 - 1 or a.min() < -2 ** 31):
            raise ValueError('labels outside int32')
        if L is None:
            L = max(int(a.max()), 0)
        t = torch.as_tensor(np.ascontiguousarray(a.astype(np.int32))).to(device)
    with torch.cuda.device(t.device):
        if L is None:
            L = max(int(t.max()), 0)
        d2 = ops.edt_sq_full((t > 0).to(torch.uint8))
        return tuple(x.cpu().numpy() for x in ops.object_measure(t, int(L), d2))


def features(table_row, scale=1.0, width=None):
    """The float quantities of one table row, from Python integers (area x sum r^2 - (sum r)^2 does not fit 64 bits).  Lengths
    are multiplied by ``scale``, areas by ``scale``^2.  ``width`` (the image's W) turns the Feret end points and the inradius point
    into coordinates; without it they are None.  None for an absent label.

    area; centroid (x, y) of the pixel centres (+ 0.5); bbox [xmin, ymin, xmax, ymax] in corners and extent = area / box area;
    equivalent_diameter; perimeter = A + sqrt 2 B + (1 + sqrt 2) / 2 C and circularity 4 pi area / perimeter^2 (None for
    perimeter 0); major / minor axis 4 sqrt(lambda) of the covariance of the pixel centres, eccentricity, orientation
    1/2 atan2(2 mu_xy, mu_xx - mu_yy) in image coordinates (x to the right, y downwards); convex_area and solidity; feret_max
    with its end points; euler = (Q1 - Q3 - 2 QD) / 4 and holes = 1 - euler, which count holes only for an 8-connected label;
    inradius with its point (the pixel's centre)."""
    w = [int(v) for v in np.asarray(table_row).reshape(-1)]
    n = w[0]
    if n == 0:
        return None
    s = float(scale)
    sr, sc, srr, src, scc = w[1:6]
    # n^2 x central moments, exact
    myy, mxy, mxx = n * srr - sr * sr, n * src - sr * sc, n * scc - sc * sc
    n2 = float(n) * float(n)
    a, b, c = mxx / n2, mxy / n2, myy / n2
    root = math.sqrt(max(((a - c) / 2) ** 2 + b * b, 0.0))
    l1, l2 = (a + c) / 2 + root, max((a + c) / 2 - root, 0.0)
    perimeter = w[10] + math.sqrt(2.0) * w[11] + (1.0 + math.sqrt(2.0)) / 2.0 * w[12]
    box_area = (w[8] - w[6] + 1) * (w[9] - w[7] + 1)
    euler = (w[13] - w[14] - 2 * w[15]) // 4
    pt = (lambda p: [(p % (width + 1)) * s, (p // (width + 1)) * s]) if width is not None else (lambda p: None)
    out = {
        'area': n * s * s,
        'centroid_x': (sc / n + 0.5) * s, 'centroid_y': (sr / n + 0.5) * s,
        'bbox': [w[7] * s, w[6] * s, (w[9] + 1) * s, (w[8] + 1) * s],
        'extent': n / box_area,
        'equivalent_diameter': math.sqrt(4.0 * n / math.pi) * s,
        'perimeter': perimeter * s,
        'circularity': 4.0 * math.pi * n / (perimeter * perimeter) if perimeter > 0 else None,
        'major_axis': 4.0 * math.sqrt(l1) * s, 'minor_axis': 4.0 * math.sqrt(l2) * s,
        'eccentricity': math.sqrt(max(1.0 - l2 / l1, 0.0)) if l1 > 0 else 0.0,
        'orientation': 0.5 * math.atan2(2.0 * b, a - c),
        'convex_area': w[16] / 2.0 * s * s,
        'solidity': 2.0 * n / w[16],
        'feret_max': math.sqrt(w[18]) * s, 'feret_p': pt(w[19]), 'feret_q': pt(w[20]),
        'euler': euler, 'holes': 1 - euler,
        'inradius': math.sqrt(w[21]) * s,
        'inradius_point': [(w[22] % width + 0.5) * s, (w[22] // width + 0.5) * s] if width is not None else None,
    }
    return out


CSV_FIELDS = ('area', 'centroid_x', 'centroid_y', 'bbox_xmin', 'bbox_ymin', 'bbox_xmax', 'bbox_ymax', 'extent',
              'equivalent_diameter', 'perimeter', 'circularity', 'major_axis', 'minor_axis', 'eccentricity', 'orientation',
              'convex_area', 'solidity', 'feret_max', 'feret_px', 'feret_py', 'feret_qx', 'feret_qy', 'euler', 'holes', 'inradius',
              'inradius_x', 'inradius_y')


def _flat(f):
    """A feature dict as the csv's columns."""
    d = {k: v for k, v in f.items() if k not in ('bbox', 'feret_p', 'feret_q', 'inradius_point')}
    d.update(zip(('bbox_xmin', 'bbox_ymin', 'bbox_xmax', 'bbox_ymax'), f['bbox']))
    for k, name in (('feret_p', 'feret_p'), ('feret_q', 'feret_q'), ('inradius_point', 'inradius_')):
        x, y = f[k] if f[k] is not None else ('', '')
        d[name + 'x'], d[name + 'y'] = x, y
    return d


def object_rows(labels, image, device=None, cls=0, min_area=0, scale=1.0):
    """The csv rows (dicts) of the objects of one label map (H, W): image, object, class and the features; labels of fewer than
    ``min_area`` pixels are dropped.  Also returns {(0, label): features} for ``contour.to_geojson``."""
    table, _, status = measure(labels, None, device)
    if status.any():
        raise ValueError(f'{image}: a negative label')
    W = int(labels.shape[-1])
    rows, by_label = [], {}
    for l in range(1, table.shape[1]):
        if table[0, l, 0] == 0 or table[0, l, 0] < min_area:
            continue
        f = features(table[0, l], scale, W)
        by_label[(0, l)] = f
        row = {'image': image, 'object': l, 'class': cls}
        flat = _flat(f)
        row.update({k: ('' if flat[k] is None else repr(flat[k]) if isinstance(flat[k], float) else flat[k]) for k in CSV_FIELDS})
        rows.append(row)
    return rows, by_label


def write_csv(path, rows):
    path = Path(path).expanduser()
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, 'w', newline='') as f:
        wr = csv.DictWriter(f, fieldnames=('image', 'object', 'class') + CSV_FIELDS)
        wr.writeheader()
        wr.writerows(rows)
    return path


def _instances(mask, device):
    """8-connected components of a binary mask as an instance map: a numpy array, or a device tensor with ``device``."""
    from . import contour
    lab, _ = contour._components(mask, device)
    return lab


def measure_directory(pred_dir, out_csv, device=None, labels=False, classes=0, min_area=0, scale=1.0, geojson=None, log=print,
                      simplify=None):
    """One csv row per object of every ``*.png`` / ``*.bmp`` of ``pred_dir``: binary masks (any non-zero) are labelled 8-connected
    (``ops.cc_label`` on the device), 16-bit instance maps are read with ``labels``, class-index maps of ``classes`` = C per class.
    ``geojson``: a directory that gets ``<stem>.geojson`` with the features under ``properties.measurements``; ``simplify``: its
    outlines are simplified within that many pixels -- the measurements stay those of the traced objects."""
    from PIL import Image
    from . import contour
    if simplify is not None and geojson is None:
        raise ValueError('simplify: the tolerance of the outlines that geojson writes')
    pred_dir = Path(pred_dir).expanduser()
    paths = sorted(p for e in ('*.bmp', '*.png') for p in pred_dir.glob(e))
    rows = []
    for path in paths:
        a = np.asarray(Image.open(path))
        a = a[..., 0] if a.ndim == 3 else a
        n0, polys, meas, stats = len(rows), [], {}, {}
        for k in (range(1, int(classes)) if classes else (0,)):
            lab = a.astype(np.int32) if labels else _instances(a == k if classes else a, device)
            r, by_label = object_rows(lab, path.name, device, k, min_area, scale)
            rows += r
            if geojson is not None:
                lab_np = lab.cpu().numpy() if not isinstance(lab, np.ndarray) else lab
                if simplify is None:
                    ps = [p for p in contour.polygons(*contour.trace(lab_np, device)[:2]) if p['area_px'] >= min_area]
                else:
                    ps = contour.label_polygons(lab_np, device, min_area, simplify, stats)
                for p in ps:
                    if classes:
                        p['class'] = k
                    meas[(len(polys), p['label'])] = by_label[(0, p['label'])]
                    p['image'] = len(polys)
                    polys.append(p)
        if geojson is not None:
            contour.write_geojson(Path(geojson).expanduser() / (path.stem + '.geojson'), polys, scale, measurements=meas)
        log(f'{path.name}: {len(rows) - n0} objects' + ('' if simplify is None else '; ' + contour.simplify_log(stats, simplify)))
    write_csv(out_csv, rows)
    return rows


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('pred_dir', help='directory of masks (*.png, *.bmp): binary (any non-zero) unless --labels or --classes')
    ap.add_argument('out_csv', help='receives one row per object')
    ap.add_argument('--gpu', action='store_true', help='label and measure on the device (ops.cc_label, ops.object_measure)')
    ap.add_argument('-d', '--device', default='cuda')
    ap.add_argument('--labels', action='store_true', help='the inputs are 16-bit instance maps (split.py --labels)')
    ap.add_argument('--classes', type=int, default=0, help='the inputs are class-index maps of this many classes')
    ap.add_argument('--min-area', type=int, default=0, help='drop objects of fewer pixels')
    ap.add_argument('--scale', type=float, default=1.0, help='slide pixels per mask pixel')
    ap.add_argument('--geojson', default=None, metavar='DIR', help='also write <stem>.geojson with the measurements as properties')
    ap.add_argument('--simplify', type=float, default=None, metavar='PX', help='simplify the outlines of --geojson within this many pixels')
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.labels and a.classes:
        raise SystemExit('--labels and --classes exclude each other')
    measure_directory(a.pred_dir, a.out_csv, a.device if a.gpu else None, a.labels, a.classes, a.min_area, a.scale, a.geojson,
                      **({} if a.simplify is None else {'simplify': a.simplify}))


if __name__ == '__main__':
    main()
