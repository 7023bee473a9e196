"""Object outlines: exact boundary rings of a label map, polygons with holes, GeoJSON.

  python -m wesup_amd.contour PRED_DIR OUT_DIR [--gpu] [--labels] [--classes C] [--min-area A] [--scale S]

Pixel (r, c) covers [c, c+1] x [r, r+1]; vertices are integer pixel corners (x, y), y downwards.  A *crack* is a unit edge between
a pixel of label l > 0 and a 4-neighbour whose label differs or that lies outside the image, directed with its pixel on the left
hand (image shown with row 0 on top):

    side   index   from            to
    N      0       (c+1, r)        (c, r)
    W      1       (c, r)          (c, r+1)
    S      2       (c, r+1)        (c+1, r+1)
    E      3       (c+1, r+1)      (c+1, r)

and its *slot* is 4 (r W + c) + side.  At a crack's end point its successor is the first of the right turn, straight on and the
left turn that is a crack of the same label (right as travelled on screen: E -> S -> W -> N -> E), which follows objects as
8-connected; every crack has one successor and one predecessor, so the cracks fall into rings.  A ring's *leader* is its crack of
the smallest slot, rings are ordered by (image, leader slot), a ring's vertices are the start points of those of its cracks
whose direction differs from their predecessor's, from the leader on, and area2 = -sum(x_i y_i+1 - x_i+1 y_i) over its cracks is
positive for outer rings (counter-clockwise on screen) and negative for holes.

``trace_host`` is this definition, a sequential tracer in plain Python; the device path (csrc/contour.hip, ``ops.contour_trace``)
is held to it word for word."""
import argparse
import json
from pathlib import Path

import numpy as np

from .utils import metrics as M

RING = 12                                    # int32 words of a ring record (WESUP_CONTOUR_RING)
RING_FIELDS = ('image', 'label', 'first_vertex', 'n_vertices', 'n_cracks', 'xmin', 'ymin', 'xmax', 'ymax', 'leader_slot',
               'area2_lo', 'area2_hi')
_START = ((1, 0), (0, 0), (0, 1), (1, 1))    # (dx, dy) from the pixel's corner (c, r) to the crack's start, per side
_END = ((0, 0), (0, 1), (1, 1), (1, 0))      # ... to its end
_LEAVE = ((0, -1), (0, 0), (-1, 0), (-1, -1))  # (dr, dc) from a vertex (vy, vx) to the pixel whose side t leaves it: SW, SE, NE, NW


def _labels3(labels):
    a = np.asarray(labels)
    if a.ndim not in (2, 3) or a.dtype.kind not in 'iub':
        raise ValueError(f'labels: expected an integer (H,W) or (B,H,W) array, got {a.dtype} {a.shape}')
    a = a.astype(np.int64)
    return a[None] if a.ndim == 2 else a


def area2_of(rings):
    """The int64 area2 of ring records (R, 12) int32."""
    r = np.ascontiguousarray(np.asarray(rings, dtype=np.int32).reshape(-1, RING)[:, 10:12])
    return r.view('<i8').reshape(-1)


def _trace_image(lab, b, v0, rings, verts):
    H, W = lab.shape
    pad = np.zeros((H + 2, W + 2), np.int64)
    pad[1:-1, 1:-1] = lab
    fg = lab > 0
    crack = np.zeros((H, W, 4), bool)
    crack[..., 0] = fg & (pad[:-2, 1:-1] != lab)
    crack[..., 1] = fg & (pad[1:-1, :-2] != lab)
    crack[..., 2] = fg & (pad[2:, 1:-1] != lab)
    crack[..., 3] = fg & (pad[1:-1, 2:] != lab)
    flat, labf = crack.ravel(), lab.ravel()
    seen = bytearray(flat.size)
    nv = v0
    for s in np.flatnonzero(flat).tolist():
        if seen[s]:
            continue
        l = int(labf[s >> 2])
        xs, ys, ds = [], [], []
        cur = s
        while True:
            seen[cur] = 1
            p, d = divmod(cur, 4)
            r, c = divmod(p, W)
            xs.append(c + _START[d][0])
            ys.append(r + _START[d][1])
            ds.append(d)
            vx, vy = c + _END[d][0], r + _END[d][1]
            for t in ((d + 3) & 3, d, (d + 1) & 3):
                rr, cc = vy + _LEAVE[t][0], vx + _LEAVE[t][1]
                if 0 <= rr < H and 0 <= cc < W:
                    q = 4 * (rr * W + cc) + t
                    if labf[q >> 2] == l and flat[q]:
                        cur = q
                        break
            else:
                raise AssertionError('a crack without a successor')
            if cur == s:
                break
        x, y, d = np.array(xs, np.int64), np.array(ys, np.int64), np.array(ds)
        a2 = -int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())
        corner = d != np.roll(d, 1)
        pts = np.stack([x[corner], y[corner]], 1)
        lo, hi = np.array([a2], '<i8').view('<i4')
        rings.append((b, np.int64(l).astype(np.int32), nv, len(pts), len(ds), x.min(), y.min(),
                      x.max(), y.max(), s, lo, hi))
        verts.append(pts)
        nv += len(pts)


def trace_host(labels):
    """The rings of a label map, labels (H,W) or (B,H,W) integers (labels <= 0 own no cracks) -> (rings (R, 12) int32, verts
    (V, 2) int32, n_rings (B,) int32): records [image, label, first vertex, vertices, cracks, xmin, ymin, xmax, ymax, leader slot,
    area2 as one little-endian int64], rings and vertices of a batch concatenated image-major."""
    L = _labels3(labels)
    rings, verts, n_rings = [], [np.zeros((0, 2), np.int64)], []
    for b, lab in enumerate(L):
        before = len(rings)
        chunk = [np.zeros((0, 2), np.int64)]
        v0 = sum(len(v) for v in verts)
        _trace_image(lab, b, v0, rings, chunk)
        verts.extend(chunk[1:])
        n_rings.append(len(rings) - before)
    R = np.array(rings, np.int64).astype(np.int32).reshape(-1, RING)
    return R, np.concatenate(verts).astype(np.int32), np.array(n_rings, np.int32)


def count_host(labels):
    """(B, 2) int32: the cracks and the corners of every image, from the traced rings."""
    L = _labels3(labels)
    R, _, _ = trace_host(L)
    out = np.zeros((len(L), 2), np.int32)
    np.add.at(out, (R[:, 0], 0), R[:, 4])
    np.add.at(out, (R[:, 0], 1), R[:, 3])
    return out


def trace(labels, device=None):
    """``trace_host``, or with ``device`` the same from the GPU (ops.contour_trace); numpy arrays either way."""
    if device is None:
        return trace_host(labels)
    import torch
    from . import ops
    a = np.asarray(labels)
    if a.size and (a.max() > 2 ** 31 - 1 or a.min() < -2 ** 31):
        raise ValueError('labels outside int32')
    t = torch.as_tensor(np.ascontiguousarray(a.astype(np.int32))).to(device)
    with torch.cuda.device(t.device):
        return tuple(x.cpu().numpy() for x in ops.contour_trace(t))


def rings_to_mask_host(rings, verts, shape, image=0, label=None):
    """Even-odd fill of the rings of ``image`` (those of ``label``, or all) -> bool (H, W).  Every vertical polygon edge at x
    spanning rows y0..y1 toggles the cells [y0:y1, x:]: a difference array and a cumulative xor along the row."""
    H, W = int(shape[0]), int(shape[1])
    rings = np.asarray(rings).reshape(-1, RING)
    verts = np.asarray(verts).reshape(-1, 2)
    T = np.zeros((H + 1, W + 1), np.int64)
    for rec in rings:
        if rec[0] != image or (label is not None and rec[1] != label):
            continue
        p = verts[rec[2]:rec[2] + rec[3]].astype(np.int64)
        _toggle(T, p)
    return _fill(T, H, W)


def _toggle(T, p):
    q = np.roll(p, -1, axis=0)
    v = p[:, 0] == q[:, 0]
    np.add.at(T, (p[v, 1], p[v, 0]), 1)
    np.add.at(T, (q[v, 1], q[v, 0]), 1)


def _fill(T, H, W):
    return (np.cumsum(np.cumsum(T, axis=0) & 1, axis=1) & 1)[:H, :W].astype(bool)


def polygons(rings, verts):
    """Group rings per (image, label) -> a list of {image, label, outer (n, 2) int32, holes [(m, 2) ...], area_px, perimeter_px,
    bbox [xmin, ymin, xmax, ymax]} in the order of the outer rings.  A label with other than one outer ring is more than one
    object: ValueError."""
    rings = np.asarray(rings).reshape(-1, RING)
    verts = np.asarray(verts).reshape(-1, 2)
    a2 = area2_of(rings)
    groups = {}
    for i, rec in enumerate(rings):
        groups.setdefault((int(rec[0]), int(rec[1])), []).append(i)
    out = []
    for (b, l), idx in groups.items():
        outer = [i for i in idx if a2[i] > 0]
        if len(outer) != 1:
            raise ValueError(f'image {b}, label {l}: {len(outer)} outer rings -- a label must be one 8-connected object: label '
                             'the components first (cc_label / mask_polygons)')
        pts = lambda i: verts[rings[i, 2]:rings[i, 2] + rings[i, 3]].astype(np.int32)
        o = outer[0]
        out.append({'image': b, 'label': l, 'outer': pts(o), 'holes': [pts(i) for i in idx if a2[i] < 0],
                    'area_px': int(sum(int(a2[i]) for i in idx) // 2), 'perimeter_px': int(sum(int(rings[i, 4]) for i in idx)),
                    'bbox': [int(v) for v in rings[o, 5:9]]})
    return out


def _components(mask, device):
    m = np.asarray(mask) != 0
    if m.ndim != 2:
        raise ValueError(f'mask: expected (H,W), got {m.shape}')
    if device is None:
        return M.label(m).astype(np.int32), None
    import torch
    from . import ops
    t = torch.as_tensor(m).to(device).to(torch.uint8).contiguous()
    with torch.cuda.device(t.device):
        return ops.cc_label(t, 8)[0], t.device


def mask_polygons(mask, device=None, min_area=0):
    """The objects of a binary mask (H, W), 8-connected (``cc_label(..., 8)``), as polygons with holes; objects of fewer than
    ``min_area`` pixels are dropped.  With ``device`` labelling and tracing run on the GPU."""
    lab, dev = _components(mask, device)
    if dev is None:
        r, v, _ = trace_host(lab)
    else:
        import torch
        from . import ops
        with torch.cuda.device(dev):
            r, v = (x.cpu().numpy() for x in ops.contour_trace(lab)[:2])
    return [p for p in polygons(r, v) if p['area_px'] >= min_area]


def classmap_polygons(cmap, n_classes, device=None, min_area=0):
    """The objects of every class 1 .. n_classes - 1 of a class-index map (H, W), each polygon carrying its ``class``; labels
    number the objects of their class."""
    cmap = np.asarray(cmap)
    n_classes = int(n_classes)
    if n_classes < 2:
        raise ValueError(f'n_classes {n_classes}: at least 2')
    out = []
    for k in range(1, n_classes):
        for p in mask_polygons(cmap == k, device, min_area):
            p['class'] = k
            out.append(p)
    return out


def to_geojson(polys, scale=1.0, offset=(0, 0), class_names=None, measurements=None):
    """A GeoJSON FeatureCollection (a dict): one Polygon feature per object, the outer ring first and then the holes, rings closed
    and in the direction they were traced; coordinates x * scale + offset[0], y * scale + offset[1].  ``measurements`` maps
    (image, label) to a feature dict (measure.features), written to ``properties.measurements`` of that object."""
    ox, oy = offset

    def ring(p):
        pts = [[float(x) * scale + ox, float(y) * scale + oy] for x, y in np.asarray(p).tolist()]
        return pts + pts[:1]

    feats = []
    for p in polys:
        props = {'objectType': 'annotation', 'label': int(p['label']), 'area_px': int(p['area_px']),
                 'perimeter_px': int(p['perimeter_px']), 'bbox': [int(v) for v in p['bbox']]}
        if 'class' in p:
            k = int(p['class'])
            props['classification'] = {'name': str(class_names[k]) if class_names is not None else f'class {k}'}
        if measurements is not None and (int(p['image']), int(p['label'])) in measurements:
            props['measurements'] = measurements[(int(p['image']), int(p['label']))]
        feats.append({'type': 'Feature', 'geometry': {'type': 'Polygon', 'coordinates': [ring(p['outer'])] + [ring(h) for h in p['holes']]},
                      'properties': props})
    return {'type': 'FeatureCollection', 'features': feats}


def write_geojson(path, polys, scale=1.0, offset=(0, 0), class_names=None, measurements=None):
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, 'w') as f:
        json.dump(to_geojson(polys, scale, offset, class_names, measurements), f)
    return path


def geojson_to_mask_host(doc, shape, scale=1.0, offset=(0, 0)):
    """Even-odd fill of every polygon of a FeatureCollection whose coordinates are integer corners after undoing scale and offset
    -> bool (H, W).  The check of an export, not a general reader."""
    H, W = int(shape[0]), int(shape[1])
    T = np.zeros((H + 1, W + 1), np.int64)
    for f in doc['features']:
        for r in f['geometry']['coordinates']:
            p = np.asarray(r[:-1], np.float64)
            p = np.rint((p - np.asarray(offset, np.float64)) / scale).astype(np.int64)
            _toggle(T, p)
    return _fill(T, H, W)


def export_directory(pred_dir, out_dir, device=None, labels=False, classes=0, min_area=0, scale=1.0, log=print):
    """``<stem>.geojson`` in ``out_dir`` for every ``*.png`` / ``*.bmp`` of ``pred_dir``: binary masks (any non-zero) by default,
    16-bit instance maps with ``labels``, class-index maps with ``classes`` = C."""
    from PIL import Image
    pred_dir, out_dir = Path(pred_dir).expanduser(), Path(out_dir).expanduser()
    out_dir.mkdir(parents=True, exist_ok=True)
    paths = sorted(p for e in ('*.bmp', '*.png') for p in pred_dir.glob(e))
    for path in paths:
        a = np.asarray(Image.open(path))
        a = a[..., 0] if a.ndim == 3 else a
        if labels:
            polys = [p for p in polygons(*trace(a.astype(np.int32), device)[:2]) if p['area_px'] >= min_area]
        elif classes:
            polys = classmap_polygons(a, classes, device, min_area)
        else:
            polys = mask_polygons(a, device, min_area)
        write_geojson(out_dir / (path.stem + '.geojson'), polys, scale)
        log(f'{path.name}: {len(polys)} polygons')
    return paths


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('pred_dir', help='directory of masks (*.png, *.bmp): binary (any non-zero) unless --labels or --classes')
    ap.add_argument('out_dir', help='receives <stem>.geojson')
    ap.add_argument('--gpu', action='store_true', help='label and trace on the device (ops.cc_label, ops.contour_trace)')
    ap.add_argument('-d', '--device', default='cuda')
    ap.add_argument('--labels', action='store_true', help='the inputs are 16-bit instance maps (split.py --labels)')
    ap.add_argument('--classes', type=int, default=0, help='the inputs are class-index maps of this many classes')
    ap.add_argument('--min-area', type=int, default=0, help='drop objects of fewer pixels')
    ap.add_argument('--scale', type=float, default=1.0, help='slide pixels per mask pixel')
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.labels and a.classes:
        raise SystemExit('--labels and --classes exclude each other')
    export_directory(a.pred_dir, a.out_dir, a.device if a.gpu else None, a.labels, a.classes, a.min_area, a.scale)


if __name__ == '__main__':
    main()
