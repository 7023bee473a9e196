"""Object outlines: exact boundary rings of a label map, polygons with holes, GeoJSON.

  python -m wesup_amd.contour PRED_DIR OUT_DIR [--gpu] [--labels] [--classes C] [--min-area A] [--scale S] [--simplify PX]

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
is held to it word for word.

Simplification is opt-in: ``simplify_host`` is an exact integer Douglas-Peucker over the traced rings, the device
path (``ops.contour_simplify``) is held to it word for word, and ``simplify=PX`` / ``--simplify PX`` put it under the exports."""
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


# ---------------------------------------------------------------- simplification
SIMPLIFY_TOL_MAX = 4096                      # sixteenths of a pixel: 256 px
SIMPLIFY_SPAN = 32768                        # a ring whose bounding box spans this or more is emitted as traced (flag 2)
FLAG_ORIENTATION, FLAG_OVERSIZE = 1, 2
_M64 = (1 << 64) - 1


def _wrap64(v):
    v &= _M64
    return v - (1 << 64) if v >> 63 else v


def _area2_points(x, y):
    n = len(x)
    return _wrap64(-sum(x[i] * y[(i + 1) % n] - x[(i + 1) % n] * y[i] for i in range(n)))


def _kept_of_ring(x, y, tol2):
    """The kept indices of one ring of n > 4 vertices (Python integer lists), ascending: the anchors and every split point."""
    n = len(x)
    x0, y0 = x[0], y[0]
    a1, far = 0, 0
    for k in range(n):
        d = (x[k] - x0) ** 2 + (y[k] - y0) ** 2
        if d > far:
            a1, far = k, d
    keep = {0, a1}
    stack = [(0, a1), (a1, n)]                # positions along the ring, n standing for vertex 0 again
    while stack:
        lo, hi = stack.pop()
        if hi - lo < 2:
            continue
        ax, ay = x[lo], y[lo]
        bx, by = x[hi % n], y[hi % n]
        ux, uy = bx - ax, by - ay
        L = ux * ux + uy * uy
        best, bkey, m = -1, 0, -1
        for k in range(lo + 1, hi):
            px, py = x[k] - ax, y[k] - ay
            if L == 0:
                D = px * px + py * py
            else:
                t = px * ux + py * uy
                if t <= 0:
                    D = (px * px + py * py) * L
                elif t >= L:
                    D = ((x[k] - bx) ** 2 + (y[k] - by) ** 2) * L
                else:
                    c = px * uy - py * ux
                    D = c * c
            key = abs(2 * k - lo - hi)
            if D > best or (D == best and key < bkey):        # k ascends: among equal (D, key) the smallest k stays
                best, bkey, m = D, key, k
        if best > (tol2 * (L if L else 1)) >> 8:
            keep.add(m)
            stack.append((lo, m))
            stack.append((m, hi))
    return sorted(keep)


def simplify_host(rings, verts, tol_q4):
    """Exact Douglas-Peucker of traced rings: ring records (R, 12) and vertices (V, 2) as ``trace_host`` returns
    them, ``tol_q4`` the tolerance in sixteenths of a pixel (an integer, 0 .. 4096) -> (rings2 (R, 12) int32, verts2 (V2, 2)
    int32, flags (R,) int32).  Rings and vertices stay in order, the kept vertices are a subsequence of every ring's; image, label,
    cracks and leader slot stay as traced, first vertex, vertex count, bounding box and area2 are those of the kept vertices.

    A ring of n <= 4 vertices is emitted as it is; one whose record's bounding box spans 32768 or more as it is with flag 2.
    Otherwise the anchors are vertex 0 and the vertex farthest from it (the smallest index among equals), and a piece between kept
    positions lo < hi splits at the position m of the largest D (squared distance to the segment, times L = |b - a|^2; among
    equals the smallest |2k - lo - hi|, then the smallest k) iff 256 D(m) > tol_q4^2 L.  A ring left with fewer than 3 vertices or
    with an area2 that is zero or of the other sign is emitted as traced with flag 1.  Plain Python integers, an explicit stack."""
    if int(tol_q4) != tol_q4 or not 0 <= int(tol_q4) <= SIMPLIFY_TOL_MAX:
        raise ValueError(f'tol_q4 {tol_q4}: an integer in 0 .. {SIMPLIFY_TOL_MAX}')
    tol2 = int(tol_q4) ** 2
    rings = np.asarray(rings, np.int32).reshape(-1, RING)
    verts = np.asarray(verts, np.int32).reshape(-1, 2)
    V = len(verts)
    out = rings.copy()
    flags = np.zeros(len(rings), np.int32)
    a2 = area2_of(rings).tolist()
    chunks, nv, expect = [np.zeros((0, 2), np.int32)], 0, 0
    for i, rec in enumerate(rings.tolist()):
        fv, n = rec[2], rec[3]
        if fv != expect or n < 1 or fv + n > V:
            raise ValueError(f'ring {i}: vertices {fv} .. {fv + n} do not follow ring {i - 1} inside 0 .. {V}')
        expect = fv + n
        x, y = verts[fv:fv + n, 0].tolist(), verts[fv:fv + n, 1].tolist()
        kept = list(range(n))
        if n > 4:
            if rec[7] - rec[5] >= SIMPLIFY_SPAN or rec[8] - rec[6] >= SIMPLIFY_SPAN:
                flags[i] |= FLAG_OVERSIZE
            else:
                k2 = _kept_of_ring(x, y, tol2)
                s = _area2_points([x[k] for k in k2], [y[k] for k in k2]) if len(k2) >= 3 else 0
                if len(k2) < 3 or s == 0 or (s > 0) != (a2[i] > 0) or a2[i] == 0:
                    flags[i] |= FLAG_ORIENTATION
                else:
                    kept = k2
        kx, ky = [x[k] for k in kept], [y[k] for k in kept]
        lo, hi = np.array([_area2_points(kx, ky)], '<i8').view('<i4')
        out[i, 2], out[i, 3] = nv, len(kept)
        out[i, 5:9] = (min(kx), min(ky), max(kx), max(ky))
        out[i, 10], out[i, 11] = lo, hi
        chunks.append(verts[fv:fv + n][kept])
        nv += len(kept)
    if expect != V:
        raise ValueError(f'the rings hold {expect} vertices, verts {V}')
    return out, np.concatenate(chunks).astype(np.int32).reshape(-1, 2), flags


def _tol_q4(tolerance_px):
    t = float(tolerance_px)
    if not 0 <= t <= SIMPLIFY_TOL_MAX / 16:
        raise ValueError(f'simplify tolerance {tolerance_px}: 0 .. {SIMPLIFY_TOL_MAX // 16} pixels')
    return int(round(16 * t))


def simplify(rings, verts, tolerance_px, device=None):
    """``simplify_host`` at tol_q4 = round(16 tolerance_px), or with ``device`` the same from the GPU (ops.contour_simplify);
    numpy arrays either way: (rings2, verts2, flags)."""
    tol = _tol_q4(tolerance_px)
    if device is None:
        return simplify_host(rings, verts, tol)
    import torch
    from . import ops
    dev = torch.device(device)
    with torch.cuda.device(dev):
        r = torch.as_tensor(np.ascontiguousarray(np.asarray(rings, np.int32).reshape(-1, RING))).to(dev)
        v = torch.as_tensor(np.ascontiguousarray(np.asarray(verts, np.int32).reshape(-1, 2))).to(dev)
        return tuple(t.cpu().numpy() for t in ops.contour_simplify(r, v, tol)[:3])


def _per_label(before, after):
    per = {}
    for arr in (before, after):
        ls, cs = np.unique(arr[arr > 0], return_counts=True)
        for l, c in zip(ls.tolist(), cs.tolist()):
            per[l] = per.get(l, 0) + c
    return per


def _change_device(lab3, rings2, verts2):
    """``simplify_change`` on device tensors: lab3 (B, H, W) int32 with nothing below 0."""
    import torch
    from . import ops, raster
    if rings2.shape[0]:
        fv, rf, ffr, fimg, flab = raster.rings_to_csr(rings2, verts2)
        filled = ops.polygon_fill(fv, rf, ffr, fimg, tuple(lab3.shape))[0]
        after = torch.cat([torch.zeros(1, dtype=torch.int32, device=lab3.device), flab])[filled.long()]
    else:
        after = torch.zeros_like(lab3)
    diff = after != lab3
    return int(diff.sum().item()), _per_label(lab3[diff].cpu().numpy().astype(np.int64), after[diff].cpu().numpy().astype(np.int64))


def simplify_change(labels, rings2, verts2, device=None):
    """What a simplification changed: the simplified polygons filled back (one feature per (image, label), later features over
    earlier ones) against ``labels`` (H,W) / (B,H,W) -> (the number of pixels whose label differs, {label: pixels that the label
    lost or gained}).  ``raster.fill_host`` on the host, ``raster.rings_to_csr`` and ``ops.polygon_fill`` with ``device``."""
    from . import raster
    L = _labels3(labels)
    L = np.where(L > 0, L, 0)
    rings2 = np.asarray(rings2, np.int32).reshape(-1, RING)
    verts2 = np.asarray(verts2, np.int32).reshape(-1, 2)
    if device is not None:
        import torch
        dev = torch.device(device)
        with torch.cuda.device(dev):
            return _change_device(torch.as_tensor(L.astype(np.int32)).to(dev), torch.as_tensor(rings2).to(dev),
                                  torch.as_tensor(verts2).to(dev))
    key = (rings2[:, 0].astype(np.int64) << 32) | (rings2[:, 1].astype(np.int64) & 0xffffffff)
    order = np.argsort(key, kind='stable')
    n = rings2[order, 3].astype(np.int64)
    ring_first = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    src, _ = raster._ranges(rings2[order, 2].astype(np.int64), n)
    k, counts = np.unique(key[order], return_counts=True)
    ffr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    filled = raster.fill_host(verts2[src] * raster.ONE, ring_first, ffr, (k >> 32).astype(np.int32), L.shape)[0]
    after = np.concatenate([[0], (k & 0xffffffff).astype(np.int64)])[filled]
    diff = after != L
    return int(diff.sum()), _per_label(L[diff], after[diff])


def _traced_and_simplified(lab, device, tolerance_px, stats):
    """(rings, verts, rings2, verts2) of an instance map as numpy arrays; with ``device`` the map, the rings and the fill-back stay
    on the GPU (ops.contour_trace, ops.contour_simplify, ops.polygon_fill).  ``stats`` collects the counts of ``simplify_log``."""
    tol = _tol_q4(tolerance_px)
    if device is None:
        lab = np.asarray(lab)
        r, v = trace_host(lab)[:2]
        r2, v2, fl = simplify_host(r, v, tol)
        changed = simplify_change(lab, r2, v2)[0] if stats is not None else 0
    else:
        import torch
        from . import ops
        dev = torch.device(device)
        with torch.cuda.device(dev):
            t = lab if isinstance(lab, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(np.asarray(lab).astype(np.int32))).to(dev)
            rt, vt, _ = ops.contour_trace(t)
            r2t, v2t, flt, _ = ops.contour_simplify(rt, vt, tol)
            t3 = t.clamp(min=0).reshape((-1,) + tuple(t.shape[-2:]))
            changed = _change_device(t3, r2t, v2t)[0] if stats is not None else 0
            r, v, r2, v2, fl = (x.cpu().numpy() for x in (rt, vt, r2t, v2t, flt))
    if stats is not None:
        for k, n in (('vertices', len(v)), ('kept', len(v2)), ('flag1', int((fl & FLAG_ORIENTATION != 0).sum())),
                     ('flag2', int((fl & FLAG_OVERSIZE != 0).sum())), ('changed', changed)):
            stats[k] = stats.get(k, 0) + n
    return r, v, r2, v2


def label_polygons(lab, device=None, min_area=0, simplify=None, stats=None):
    """The polygons of an instance map (H, W) in which every label is one 8-connected object.  ``simplify``: a tolerance in pixels
    (DESIGN.md 3.24); area_px / perimeter_px / bbox stay those of the traced object, ``simplified_area2`` (the area2 of the
    simplified rings, holes counting negative) and ``simplify_px`` are added.  ``stats``: a dict that collects vertices, kept,
    flag1, flag2 and changed (``simplify_change``) for ``simplify_log``."""
    if simplify is None:
        return [p for p in polygons(*trace(np.asarray(lab).astype(np.int32), device)[:2]) if p['area_px'] >= min_area]
    r, v, r2, v2 = _traced_and_simplified(lab, device, simplify, stats)
    traced = {(p['image'], p['label']): p for p in polygons(r, v)}
    a2 = {}
    for rec, a in zip(r2.tolist(), area2_of(r2).tolist()):
        a2[(rec[0], rec[1])] = a2.get((rec[0], rec[1]), 0) + a
    out = []
    for p in polygons(r2, v2):
        t = traced[(p['image'], p['label'])]
        if t['area_px'] < min_area:
            continue
        p.update(area_px=t['area_px'], perimeter_px=t['perimeter_px'], bbox=t['bbox'],
                 simplified_area2=int(a2[(p['image'], p['label'])]), simplify_px=float(simplify))
        out.append(p)
    return out


def simplify_log(stats, simplify):
    return (f"simplify {simplify} px: {stats.get('vertices', 0)} -> {stats.get('kept', 0)} vertices, {stats.get('flag1', 0)} rings "
            f"kept for their orientation, {stats.get('flag2', 0)} oversize, {stats.get('changed', 0)} pixels change on fill-back")


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


def mask_polygons(mask, device=None, min_area=0, simplify=None, stats=None):
    """The objects of a binary mask (H, W), 8-connected (``cc_label(..., 8)``), as polygons with holes; objects of fewer than
    ``min_area`` pixels are dropped.  With ``device`` labelling and tracing run on the GPU.  ``simplify``: see ``label_polygons``."""
    lab, dev = _components(mask, device)
    if simplify is not None:
        return label_polygons(lab, device, min_area, simplify, stats)            # (with a device the labels stay there)
    if dev is None:
        r, v, _ = trace_host(lab)
    else:
        import torch
        from . import ops
        with torch.cuda.device(dev):
            r, v = (x.cpu().numpy() for x in ops.contour_trace(lab)[:2])
    return [p for p in polygons(r, v) if p['area_px'] >= min_area]


def classmap_polygons(cmap, n_classes, device=None, min_area=0, simplify=None, stats=None):
    """The objects of every class 1 .. n_classes - 1 of a class-index map (H, W), each polygon carrying its ``class``; labels
    number the objects of their class."""
    cmap = np.asarray(cmap)
    n_classes = int(n_classes)
    if n_classes < 2:
        raise ValueError(f'n_classes {n_classes}: at least 2')
    out = []
    for k in range(1, n_classes):
        for p in (mask_polygons(cmap == k, device, min_area) if simplify is None else
                  mask_polygons(cmap == k, device, min_area, simplify, stats)):
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
        if 'simplify_px' in p:
            props['simplified_area2'] = int(p['simplified_area2'])
            props['simplify_px'] = float(p['simplify_px'])
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


def export_directory(pred_dir, out_dir, device=None, labels=False, classes=0, min_area=0, scale=1.0, log=print, simplify=None):
    """``<stem>.geojson`` in ``out_dir`` for every ``*.png`` / ``*.bmp`` of ``pred_dir``: binary masks (any non-zero) by default,
    16-bit instance maps with ``labels``, class-index maps with ``classes`` = C.  ``simplify``: a tolerance in pixels (DESIGN.md
    3.24); the vertex counts, the flagged rings and the pixels that change on fill-back are logged per file."""
    from PIL import Image
    pred_dir, out_dir = Path(pred_dir).expanduser(), Path(out_dir).expanduser()
    out_dir.mkdir(parents=True, exist_ok=True)
    paths = sorted(p for e in ('*.bmp', '*.png') for p in pred_dir.glob(e))
    for path in paths:
        a = np.asarray(Image.open(path))
        a = a[..., 0] if a.ndim == 3 else a
        stats = {}
        if simplify is None:
            if labels:
                polys = [p for p in polygons(*trace(a.astype(np.int32), device)[:2]) if p['area_px'] >= min_area]
            elif classes:
                polys = classmap_polygons(a, classes, device, min_area)
            else:
                polys = mask_polygons(a, device, min_area)
        elif labels:
            polys = label_polygons(a, device, min_area, simplify, stats)
        elif classes:
            polys = classmap_polygons(a, classes, device, min_area, simplify, stats)
        else:
            polys = mask_polygons(a, device, min_area, simplify, stats)
        write_geojson(out_dir / (path.stem + '.geojson'), polys, scale)
        log(f'{path.name}: {len(polys)} polygons' + ('' if simplify is None else '; ' + simplify_log(stats, simplify)))
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
    ap.add_argument('--simplify', type=float, default=None, metavar='PX', help='simplify every ring within this many pixels (exact Douglas-Peucker, DESIGN.md 3.24)')
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.labels and a.classes:
        raise SystemExit('--labels and --classes exclude each other')
    export_directory(a.pred_dir, a.out_dir, a.device if a.gpu else None, a.labels, a.classes, a.min_area, a.scale, simplify=a.simplify)


if __name__ == '__main__':
    main()
