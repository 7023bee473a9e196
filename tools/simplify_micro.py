"""Ring simplification (csrc/contour.hip): ops.contour_simplify beside ops.contour_trace of the same map, the
yardstick, and beside the host definition contour.simplify_host.  No ratio was fixed in advance.

  python tools/simplify_micro.py [--reps N] [--host-max VERTICES] [--out profiles/simplify_micro.txt]

The seeded gland-like masks of tools/contour_micro.py at 522 x 775 (GlaS), 2048 x 2048 and 5000 x 5000, labelled by ops.cc_label
and traced by ops.contour_trace; the rings stay on the device.  Per tolerance (0.5, 1 and 2 pixels):

  simplify  ops.contour_simplify on the resident rings with its read-back of the counts; the wall clock around a synchronised
            call, min and median of `reps`, and the median as a multiple of the trace's
  trace     ops.contour_trace of the label map (its two read-backs included), the same way, in the same run
  host      contour.simplify_host, the wall clock of one run (above --host-max vertices: not run); the device result is compared
            with it word for word wherever it runs
  change    contour.simplify_change on the device: the pixels whose label differs after the simplified polygons are filled back

and the two worst cases: one hand-made ring of 0.4 M vertices (a noisy circle: the ring that a single block works through) and
the 45-degree staircases of a diamond at 0.5 px, below the tolerance at which a staircase collapses, beside the trace of the
diamond."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from wesup_amd import contour, ops

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--host-max', type=int, default=300000)
ap.add_argument('--out', default='')
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit('simplify_micro.py measures the device path: it needs a GPU')
dev = torch.device('cuda:0')
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def scene(H, W, seed):
    """tools/contour_micro.py's: about 25 glands per 522 x 775 pixels, ellipses of half-axes 15 .. 60, a lumen in two of three."""
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


def simplify_lines(r, v, tol_px, t_med, lab=None):
    """One tolerance on resident rings: times, counts, the host beside it."""
    tol = int(round(16 * tol_px))
    out = ops.contour_simplify(r, v, tol)                  # warm-up: the workspace grows here
    s_min, s_med = timed(lambda: ops.contour_simplify(r, v, tol), a.reps)
    c = out[3].tolist()
    line = (f'  simplify {tol_px:3.1f} px   {s_min:9.3f} / {s_med:9.3f}   {v.shape[0]} -> {c[0]} vertices, {c[1]} + {c[2]} rings flagged'
            + (f'   = {s_med / t_med:.2f} x the trace' if t_med else ''))
    if lab is not None:
        line += f'; {contour._change_device(lab.reshape((1,) + tuple(lab.shape)), out[0], out[1])[0]} pixels change on fill-back'
    say(line)
    if v.shape[0] <= a.host_max:
        rh, vh = r.cpu().numpy(), v.cpu().numpy()
        t0 = time.perf_counter()
        er, ev, ef = contour.simplify_host(rh, vh, tol)
        h = (time.perf_counter() - t0) * 1e3
        same = all(np.array_equal(x, y.cpu().numpy()) for x, y in zip((er, ev, ef), out[:3]))
        say(f'  host     {tol_px:3.1f} px   {h:9.1f}               = {h / s_med:.0f} x the device; equal: {same}')
        if not same:
            raise SystemExit('the device path differs from simplify_host')
    else:
        say(f'  host     {tol_px:3.1f} px   not run (--host-max)')


say(f'simplify_micro: {torch.cuda.get_device_name(0)}, reps {a.reps}; times in ms (min / median)')
for H, W in ((522, 775), (2048, 2048), (5000, 5000)):
    lab = ops.cc_label(torch.from_numpy(scene(H, W, 7)).to(dev), 8)[0]
    r, v, _ = ops.contour_trace(lab)                       # warm-up of the trace as well
    t_min, t_med = timed(lambda: ops.contour_trace(lab), a.reps)
    say(f'{H} x {W}: {int(lab.max())} objects, {r.shape[0]} rings, {v.shape[0]} vertices, the longest ring {int(r[:, 3].max())}')
    say(f'  trace    ops.contour_trace   {t_min:9.3f} / {t_med:9.3f}')
    for tol_px in (0.5, 1.0, 2.0):
        simplify_lines(r, v, tol_px, t_med, lab)

# one ring of 0.4 M vertices: a circle of radius 12000 whose radius wobbles by up to 40 pixels
n = 400000
rng = np.random.default_rng(3)
ang = np.sort(rng.uniform(0, 2 * np.pi, n))
rad = 12000 + 40 * np.sin(37 * ang) + rng.uniform(-3, 3, n)
pts = np.stack([np.rint(13000 + rad * np.cos(ang)), np.rint(13000 - rad * np.sin(ang))], 1).astype(np.int64)
x, y = pts[:, 0], pts[:, 1]
a2 = -int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())
lo, hi = np.array([a2], '<i8').view('<i4')
rec = np.array([[0, 1, 0, n, n, x.min(), y.min(), x.max(), y.max(), 0, lo, hi]], np.int64).astype(np.int32)
r, v = torch.from_numpy(rec).to(dev), torch.from_numpy(pts.astype(np.int32)).to(dev)
say(f'one ring of {n} vertices (a noisy circle, area2 {a2:+d}): the single-block case; the trace of 5000 x 5000 above is the yardstick')
for tol_px in (0.5, 2.0):
    simplify_lines(r, v, tol_px, t_med)

# 45-degree staircases below the collapse tolerance (1 / sqrt 2 px): a diamond of radius 2000 in 4096 x 4096
rr, cc = np.indices((4096, 4096))
lab = torch.from_numpy((np.abs(rr - 2047.5) + np.abs(cc - 2047.5) <= 2000).astype(np.int32)).to(dev)
r, v, _ = ops.contour_trace(lab)
t_min, t_med = timed(lambda: ops.contour_trace(lab), a.reps)
say(f'a diamond of radius 2000 in 4096 x 4096: {v.shape[0]} vertices in one ring, four 45-degree staircases')
say(f'  trace    ops.contour_trace   {t_min:9.3f} / {t_med:9.3f}')
for tol_px in (0.5, 1.0):
    simplify_lines(r, v, tol_px, t_med, lab)
if a.out:
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
