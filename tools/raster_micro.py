"""Polygon fill (csrc/raster.hip): the device path against the host's scanline fill, with one ops.contour_trace
and one ops.cc_label of the same map as yardsticks.  No time was fixed in advance: this is a report.

  python tools/raster_micro.py [--reps N] [--out profiles/raster_micro.txt]

The gland-like scenes of tools/contour_micro.py at 522 x 775 (GlaS) and 5000 x 5000, labelled by ops.cc_label, traced by
ops.contour_trace and turned into polygons (one feature per object, vertices x 256); one quadrilateral covering 4096 x 4096; one
jagged ring of 0.4 M edges inside 4096 x 4096 (every tile of its box walks all of them: the worst case of the per-tile walk).

  fill            ops.polygon_fill on the resident CSR arrays, the wall clock around a synchronised call
  fill + copies   the CSR arrays host -> device, the fill, the label map device -> host
  trace           ops.contour_trace of the map and the copy of rings and vertices to the host (as tools/contour_micro.py times it)
  cc_label        ops.cc_label of the mask
  host            raster.fill_host, the wall clock of one run

all min / median of `reps` after a warm-up.  The device result is compared with the host's, word for word."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from wesup_amd import ops, raster

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=9)
ap.add_argument('--out', default='')
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit('raster_micro.py measures the device path: it needs a GPU')
dev = torch.device('cuda:0')
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def scene(H, W, seed):
    """About 25 glands per 522 x 775 pixels: ellipses of half-axes 15 .. 60 with a lumen of 0.4 of the size in two of three
    (the scene of tools/contour_micro.py)."""
    rng = np.random.default_rng(seed)
    mask = np.zeros((H, W), np.uint8)
    for _ in range(max(1, round(25 * H * W / (522 * 775)))):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        ay, ax = rng.uniform(15, 60, 2)
        y0, y1, x0, x1 = int(max(cy - ay, 0)), int(min(cy + ay + 1, H)), int(max(cx - ax, 0)), int(min(cx + ax + 1, W))
        yy, xx = np.mgrid[y0:y1, x0:x1]
        d = ((yy - cy) / ay) ** 2 + ((xx - cx) / ax) ** 2
        mask[y0:y1, x0:x1][d <= 1.0] = 1
        if rng.random() < 2 / 3:
            mask[y0:y1, x0:x1][d <= 0.16] = 0
    return mask


def timed(fn, reps):
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t), float(np.median(t))


def measure(name, csr, shape, extra=None):
    host = [np.ascontiguousarray(x) for x in csr]
    res = [torch.from_numpy(x).to(dev) for x in host]

    def with_copies():
        t = [torch.from_numpy(x).to(dev) for x in host]
        return ops.polygon_fill(*t, shape)[0].cpu()

    got = with_copies()                                     # warm-up: the workspace grows here
    ops.polygon_fill(*res, shape)
    f_min, f_med = timed(lambda: ops.polygon_fill(*res, shape), a.reps)
    c_min, c_med = timed(with_copies, a.reps)
    t0 = time.perf_counter()
    want, _, status = raster.fill_host(*host, shape)
    h = (time.perf_counter() - t0) * 1e3
    same = status == 0 and np.array_equal(want, got.numpy())
    tiles = -(-shape[0] // 64) * -(-shape[1] // 64)
    say(f'{name}: {shape[0]} x {shape[1]}, {len(host[3])} features, {len(host[1]) - 1} rings, {len(host[0])} vertices, '
        f'{int((want > 0).sum())} pixels covered, {tiles} tiles in the image')
    say(f'  fill            ops.polygon_fill, resident        {f_min:9.3f} / {f_med:9.3f}')
    say(f'  fill + copies   CSR in, label map out             {c_min:9.3f} / {c_med:9.3f}')
    if extra is not None:
        (t_min, t_med), (l_min, l_med) = extra
        say(f'  trace           ops.contour_trace + copy          {t_min:9.3f} / {t_med:9.3f}   fill = {f_med / t_med:.2f} x, fill + copies = '
            f'{c_med / t_med:.2f} x the trace (medians)')
        say(f'  cc_label        ops.cc_label                      {l_min:9.3f} / {l_med:9.3f}   fill = {f_med / l_med:.2f} x, fill + copies = '
            f'{c_med / l_med:.2f} x cc_label (medians)')
    say(f'  host            raster.fill_host                  {h:9.1f}               = {h / f_med:.0f} x the fill, {h / c_med:.0f} x fill + copies; '
        f'equal: {same}')
    if not same:
        raise SystemExit('the device path differs from fill_host')


say(f'raster_micro: {torch.cuda.get_device_name(0)}, reps {a.reps}; times in ms (min / median)')
for H, W in ((522, 775), (5000, 5000)):
    m = torch.from_numpy(scene(H, W, 7)).to(dev)
    lab = ops.cc_label(m, 8)[0]

    def trace_path():
        r, v, _ = ops.contour_trace(lab)
        return r.cpu(), v.cpu()

    trace_path()
    ops.cc_label(m, 8)
    extra = (timed(trace_path, a.reps), timed(lambda: ops.cc_label(m, 8), a.reps))
    rings, verts, _ = ops.contour_trace(lab)
    csr = [t.cpu().numpy() for t in raster.rings_to_csr(rings, verts)[:4]]
    measure('scene', csr, (H, W), extra)
    del m, lab, rings, verts

quad = raster.pack([{'rings': [[(0.25, 0.5), (4095.75, 0.25), (4095.5, 4095.75), (0.5, 4095.5)]]}])
measure('one quadrilateral', quad[:4], (4096, 4096))
n = 400000
k = np.arange(n)
rad = 1900.0 + 1.5 * (k % 2)
ring = np.stack([2048 + rad * np.cos(2 * np.pi * k / n), 2048 + rad * np.sin(2 * np.pi * k / n)], 1)
measure('one jagged ring', raster.pack([{'rings': [ring]}])[:4], (4096, 4096))
if a.out:
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
