"""Object measurements (csrc/measure.hip): the device path against the host definition, with ops.cc_label of the
same maps as a yardstick, and the two worst cases of the hull construction.  No time was fixed in advance.

  python tools/measure_micro.py [--reps N] [--host-max PIXELS] [--out profiles/measure_micro.txt]

Seeded gland-like masks (ellipses with lumina) at 522 x 775 (GlaS) and 5000 x 5000, labelled by ops.cc_label:

  device    ops.object_measure on the resident label map and distance map -- the profile count, its read-back, the measurement, the
            status read-back -- and the copy of the table and the hulls to the host; the wall clock around a synchronised call,
            min and median of `reps`
  edt       ops.edt_sq_full of the mask, the distance map the inscribed radius is read from (not part of `device`)
  cc_label  ops.cc_label of the mask (synchronised), the same way; the device path's time is given as a multiple of it
  host      measure.measure_host with the same distance map, the wall clock of one run (maps above --host-max pixels: not run)

and, device path only, checked against closed forms: one label over 4096 x 4096 (every add meets on one entry), and a
one-pixel-wide object 32768 rows high (the O(h^2) hull test at its largest h)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from wesup_amd import measure, ops

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--host-max', type=int, default=5000 * 5000)
ap.add_argument('--out', default='')
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit('measure_micro.py measures the device path: it needs a GPU')
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


say(f'measure_micro: {torch.cuda.get_device_name(0)}, reps {a.reps}; times in ms (min / median)')
for H, W in ((522, 775), (5000, 5000)):
    mask = scene(H, W, 7)
    m = torch.from_numpy(mask).to(dev)
    lab = ops.cc_label(m, 8)[0]
    L = int(lab.max())
    d2 = ops.edt_sq_full(m)

    def device_path():
        t, v, s = ops.object_measure(lab, L, d2)
        return t.cpu(), v.cpu(), s.cpu()

    t, v, s = device_path()                                # warm-up: the workspace grows here
    ops.cc_label(m, 8)
    d_min, d_med = timed(device_path, a.reps)
    e_min, e_med = timed(lambda: ops.edt_sq_full(m), a.reps)
    c_min, c_med = timed(lambda: ops.cc_label(m, 8), a.reps)
    lines_h = int(ops.measure_profile_count(lab, L)[0].item())
    say(f'{H} x {W}: {L} objects, {lines_h} profile lines, {len(v)} hull vertices')
    say(f'  device   count + read-back + measure + copy  {d_min:9.3f} / {d_med:9.3f}')
    say(f'  edt      ops.edt_sq_full                     {e_min:9.3f} / {e_med:9.3f}')
    say(f'  cc_label                                     {c_min:9.3f} / {c_med:9.3f}   device path = {d_med / c_med:.1f} x cc_label (medians)')
    if H * W <= a.host_max:
        lab_h, d2_h = lab.cpu().numpy(), d2.cpu().numpy()
        t0 = time.perf_counter()
        ht, hv, hs = measure.measure_host(lab_h, L, d2_h)
        h = (time.perf_counter() - t0) * 1e3
        same = np.array_equal(ht, t.numpy()) and np.array_equal(hv, v.numpy()) and np.array_equal(hs, s.numpy())
        say(f'  host     measure.measure_host                {h:9.1f}               = {h / d_med:.0f} x the device path; equal: {same}')
        if not same:
            raise SystemExit('the device path differs from measure_host')
    else:
        say('  host     measure.measure_host                not run (--host-max)')

for name, lab in (('one label over 4096 x 4096', torch.ones(4096, 4096, dtype=torch.int32, device=dev)),
                  ('a 1-pixel-wide object of 32768 rows', torch.ones(32768, 1, dtype=torch.int32, device=dev))):
    H, W = lab.shape

    def worst():
        t, v, s = ops.object_measure(lab, 1)
        return t.cpu(), v.cpu()

    t, v = worst()
    row = t[0, 1].tolist()
    ok = (row[0] == H * W and row[3] == W * (H - 1) * H * (2 * H - 1) // 6 and row[16] == 2 * H * W and row[18] == H * H + W * W
          and v.tolist() == [[0, 0], [0, H], [W, H], [W, 0]])
    w_min, w_med = timed(worst, a.reps)
    say(f'{name}: {w_min:9.3f} / {w_med:9.3f}   closed forms hold: {ok}')
    if not ok:
        raise SystemExit(f'{name}: the device path misses the closed forms')
if a.out:
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
