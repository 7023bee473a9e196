"""Label maps, hand-made rings and an independent restatement for the simplification tests (tests/test_simplify_cpu.py,
tests/test_simplify_gpu.py).  Nothing here depends on a GPU, and nothing here calls the definition's helpers:
``ref_kept`` decides every comparison in ``fractions.Fraction`` on true squared distances, by recursion."""
import functools
import sys
from fractions import Fraction

import numpy as np

from _contourcases import checkerboard, named_cases, random_map, serpentine

TOLS = (0, 8, 12, 16, 40)          # sixteenths of a pixel
RING = 12


def diamond():
    """40 x 40, |r - 19.5| + |c - 19.5| <= 17: one ring of 132 vertices, four 45-degree staircases."""
    r, c = np.indices((40, 40))
    return (np.abs(r - 19.5) + np.abs(c - 19.5) <= 17).astype(np.int32)


def diagonal():
    """A 20-pixel diagonal line, 8-connected: one ring of 80 vertices."""
    return np.eye(20, dtype=np.int32)


def comb(teeth=64):
    """Teeth two pixels wide and 1 .. teeth pixels high, one pixel apart, on a base row: 258 vertices for 64 teeth.  The farthest
    vertex from a chord is always beside one of its ends, so the pieces nest 127 deep."""
    a = np.zeros((teeth + 1, 3 * teeth), np.int32)
    a[teeth, :] = 1
    for i in range(teeth):
        a[teeth - 1 - i:teeth, 3 * i:3 * i + 2] = 1
    return a


def ellipses(H=160, W=200, seed=5):
    """Twelve gland-like ellipses, one label each, on a 3 x 4 grid of cells so that none touches another."""
    rs = np.random.RandomState(seed)
    lab = np.zeros((H, W), np.int32)
    r, c = np.indices((H, W))
    ch, cw = H // 3, W // 4
    for i in range(12):
        cy, cx = (i // 4) * ch + ch / 2 + rs.uniform(-3, 3), (i % 4) * cw + cw / 2 + rs.uniform(-3, 3)
        a, b, th = rs.uniform(12, 20), rs.uniform(8, 14), rs.uniform(0, np.pi)
        u = (c - cx) * np.cos(th) + (r - cy) * np.sin(th)
        v = -(c - cx) * np.sin(th) + (r - cy) * np.cos(th)
        inside = (u / a) ** 2 + (v / b) ** 2 <= 1
        if rs.rand() < 0.5:
            inside &= (u / (0.4 * a)) ** 2 + (v / (0.4 * b)) ** 2 > 1          # a lumen: a hole ring
        lab[inside] = i + 1
    return lab


def plus_lattice(n=34):
    """n x n plus signs, 12 vertices each, none touching another: more rings than the simplify kernel's grid has blocks."""
    a = np.zeros((4 * n, 4 * n), np.int32)
    for dr, dc in ((0, 1), (1, 0), (1, 1), (1, 2), (2, 1)):
        a[dr::4, dc::4] = 1
    return a


def four_and_five():
    """A rectangle (4 vertices: emitted as it is) beside an L (6 vertices): traced rings have even counts, the ring of exactly 5
    vertices is hand-made (FOUR_FIVE)."""
    a = np.zeros((8, 16), np.int32)
    a[1:4, 1:5] = 1                    # 4 vertices
    a[1:6, 7:9] = 2
    a[4:6, 9:12] = 2                   # an L: 6 vertices
    return a


def small_maps():
    """The maps small enough for the brute-force pixel test."""
    out = dict(named_cases())
    for seed in (3, 4, 5):
        out[f'random1_{seed}'] = random_map(seed, 13, 13)
        out[f'random3_{seed}'] = random_map(seed, 13, 13, n_labels=3)
    out['checker8'] = checkerboard(8, 8)
    out['four_and_five'] = four_and_five()
    return out


def label_cases():
    out = small_maps()
    out['serpentine32'] = serpentine(32)
    out['diamond'] = diamond()
    out['diagonal'] = diagonal()
    out['comb'] = comb()
    out['ellipses'] = ellipses()
    return out


# ---------------------------------------------------------------- hand-made rings
def make_rings(point_lists, spans=None):
    """Ring records and vertices from vertex lists: image 0, label i + 1, the bounding box and area2 of the vertices as given."""
    rings, verts, fv = [], [], 0
    for i, pts in enumerate(point_lists):
        p = np.asarray(pts, np.int64).reshape(-1, 2)
        x, y = p[:, 0], p[:, 1]
        a2 = -int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())
        lo, hi = np.array([a2], '<i8').view('<i4')
        rings.append((0, i + 1, fv, len(p), 2 * len(p), x.min(), y.min(), x.max(), y.max(), 4 * i, lo, hi))
        verts.append(p)
        fv += len(p)
    return np.array(rings, np.int64).astype(np.int32).reshape(-1, RING), np.concatenate(verts).astype(np.int32)


SLIVER = [(0, 0), (0, 1), (50, 1), (100, 1), (100, 0), (50, 0)]              # tol 32 keeps the two anchors only: flag 1
REVERSED = [(2, 0), (3, 2), (10, 0), (7, 5), (9, 0)]                        # area2 +11; tol 32 keeps 0 2 3 4 with area2 -5: flag 1
OVERSIZE = [(0, 0), (0, 1), (16384, 1), (32768, 1), (32768, 0), (16384, 0)]  # a span of 32768: flag 2
THREE_MAXIMA = [(0, 0), (2, 1), (4, 1), (6, 1), (8, 0), (4, -5)]             # vertices 1 2 3 equally far from the chord 0 -> 4
FOUR_FIVE = [[(0, 0), (0, 4), (6, 4), (6, 0)], [(10, 0), (10, 4), (13, 5), (16, 4), (16, 0)]]     # 4: as it is; 5: the first that is worked on
ONE_POINT = [(3, 3)] * 5                                                    # every piece has L = 0


# ---------------------------------------------------------------- the independent restatement
def seg_dist2(p, a, b):
    """The squared distance from p to the segment ab, a Fraction."""
    ux, uy = b[0] - a[0], b[1] - a[1]
    L = ux * ux + uy * uy
    if L == 0:
        return Fraction((p[0] - a[0]) ** 2 + (p[1] - a[1]) ** 2)
    t = Fraction((p[0] - a[0]) * ux + (p[1] - a[1]) * uy, L)
    t = min(max(t, Fraction(0)), Fraction(1))
    qx, qy = a[0] + t * ux, a[1] + t * uy
    return (p[0] - qx) ** 2 + (p[1] - qy) ** 2


def ref_kept(pts, tol_q4):
    """The anchors and split points of a ring of n > 4 vertices (ascending indices), rule 5 not applied."""
    n = len(pts)
    P = [tuple(int(v) for v in p) for p in pts] + [tuple(int(v) for v in pts[0])]
    far = max(range(n), key=lambda k: ((P[k][0] - P[0][0]) ** 2 + (P[k][1] - P[0][1]) ** 2, -k))
    if P[far] == P[0]:
        far = 0
    kept = {0, far}
    tol2 = Fraction(tol_q4 * tol_q4, 256)

    def split(lo, hi):
        if hi - lo < 2:
            return
        d = {k: seg_dist2(P[k], P[lo], P[hi]) for k in range(lo + 1, hi)}
        m = min(d, key=lambda k: (-d[k], abs(2 * k - lo - hi), k))
        if d[m] > tol2:
            kept.add(m)
            split(lo, m)
            split(m, hi)

    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * n + 1000))
    split(0, far)
    split(far, n)
    return sorted(kept)


def area2(pts):
    p = [(int(x), int(y)) for x, y in pts]
    return -sum(p[i][0] * p[(i + 1) % len(p)][1] - p[(i + 1) % len(p)][0] * p[i][1] for i in range(len(p)))


def ref_simplify(rings, verts, tol_q4):
    """(rings2, verts2, flags) by ``ref_kept`` and the rules of DESIGN.md 3.24, in Python integers and Fractions."""
    rings = np.asarray(rings, np.int32).reshape(-1, RING)
    out, flags, chunks, nv = rings.copy(), [], [], 0
    for i, rec in enumerate(rings.tolist()):
        pts = np.asarray(verts)[rec[2]:rec[2] + rec[3]].tolist()
        a_in = int(np.array(rec[10:12], '<i4').view('<i8')[0])
        kept, flag = list(range(len(pts))), 0
        if len(pts) > 4:
            if rec[7] - rec[5] >= 32768 or rec[8] - rec[6] >= 32768:
                flag = 2
            else:
                k2 = ref_kept(pts, tol_q4)
                s = area2([pts[k] for k in k2]) if len(k2) >= 3 else 0
                if s == 0 or a_in == 0 or (s > 0) != (a_in > 0):
                    flag = 1
                else:
                    kept = k2
        q = [pts[k] for k in kept]
        lo, hi = np.array([area2(q)], '<i8').view('<i4')
        out[i, 2], out[i, 3] = nv, len(q)
        out[i, 5:9] = (min(x for x, _ in q), min(y for _, y in q), max(x for x, _ in q), max(y for _, y in q))
        out[i, 10], out[i, 11] = lo, hi
        chunks.extend(q)
        nv += len(q)
        flags.append(flag)
    return out, np.array(chunks, np.int32).reshape(-1, 2), np.array(flags, np.int32)


@functools.lru_cache(maxsize=None)
def traced(name):
    """(labels, rings, verts) of a label case by the host tracer, read-only."""
    from wesup_amd import contour as C
    lab = label_cases()[name]
    r, v, _ = C.trace_host(lab)
    for a in (lab, r, v):
        a.setflags(write=False)
    return lab, r, v


@functools.lru_cache(maxsize=None)
def host(name, tol_q4):
    """``simplify_host`` of a traced label case, read-only."""
    from wesup_amd import contour as C
    _, r, v = traced(name)
    out = C.simplify_host(r, v, tol_q4)
    for a in out:
        a.setflags(write=False)
    return out


def big_diamond(size=700, radius=340):
    """One ring of 8 radius + 4 vertices (2724): every per-thread loop of the simplify kernel wraps, and the ring's state lives in
    the workspace, not in LDS."""
    r, c = np.indices((size, size))
    return (np.abs(r - size // 2) + np.abs(c - size // 2) <= radius).astype(np.int32)
