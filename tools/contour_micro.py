"""Object outlines (csrc/contour.hip): the device path against the sequential host tracer, with ops.cc_label of the
same maps as a yardstick.  No ratio was fixed in advance.

  python tools/contour_micro.py [--reps N] [--host-max PIXELS] [--out profiles/contour_micro.txt]

Seeded gland-like masks (ellipses with lumina) at 522 x 775 (GlaS), 2048 x 2048 and 5000 x 5000, labelled by ops.cc_label:

  device    ops.contour_trace on the resident label map -- the count, its read-back, the trace, the status read-back -- and the
            copy of rings and vertices to the host; the wall clock around a synchronised call, min and median of `reps`
  cc_label  ops.cc_label of the mask (synchronised), the same way; the device path's time is given as a multiple of it
  host      contour.trace_host, the wall clock of one run (maps above --host-max pixels: not run, the line says so)

The device result is compared with the host's, word for word, wherever the host runs."""
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
ap.add_argument('--host-max', type=int, default=5000 * 5000)
ap.add_argument('--out', default='')
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit('contour_micro.py measures the device path: it needs a GPU')
dev = torch.device('cuda:0')
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def scene(H, W, seed):
    """About 25 glands per 522 x 775 pixels: ellipses of half-axes 15 .. 60 with a lumen of 0.4 of the size in two of three."""
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


say(f'contour_micro: {torch.cuda.get_device_name(0)}, reps {a.reps}; times in ms (min / median)')
for H, W in ((522, 775), (2048, 2048), (5000, 5000)):
    mask = scene(H, W, 7)
    m = torch.from_numpy(mask).to(dev)
    lab = ops.cc_label(m, 8)[0]

    def device_path():
        r, v, _ = ops.contour_trace(lab)
        return r.cpu(), v.cpu()

    r, v = device_path()                                   # warm-up: the workspace grows here
    ops.cc_label(m, 8)
    counts = ops.contour_count(lab).cpu().numpy()[0]
    d_min, d_med = timed(device_path, a.reps)
    c_min, c_med = timed(lambda: ops.cc_label(m, 8), a.reps)
    say(f'{H} x {W}: {int(lab.max())} objects, {len(r)} rings, {int(counts[0])} cracks, {int(counts[1])} vertices')
    say(f'  device   count + read-back + trace + copy   {d_min:9.3f} / {d_med:9.3f}')
    say(f'  cc_label                                    {c_min:9.3f} / {c_med:9.3f}   device path = {d_med / c_med:.1f} x cc_label (medians)')
    if H * W <= a.host_max:
        lab_h = lab.cpu().numpy()
        t0 = time.perf_counter()
        hr, hv, _ = contour.trace_host(lab_h)
        h = (time.perf_counter() - t0) * 1e3
        same = np.array_equal(hr, r.numpy()) and np.array_equal(hv, v.numpy())
        say(f'  host     contour.trace_host                 {h:9.1f}               = {h / d_med:.0f} x the device path; equal: {same}')
        if not same:
            raise SystemExit('the device path differs from trace_host')
    else:
        say('  host     contour.trace_host                 not run (--host-max)')
if a.out:
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
