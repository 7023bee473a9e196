"""The surface-distance metrics (csrc/surface.hip) per image, host against device, stage by stage.  No speed was
fixed in advance; what is required is that the device `whole` is below the host `whole` at both sizes.

  python tools/surface_micro.py [--reps N] [--launches N] [--out profiles/surface_micro.txt]

At 522 x 775 (GlaS) and 2048 x 2048, seeded blob scenes (a ground truth of ellipses, the prediction shifted and grown):

  borders   both 4-neighbour borders                     surface.border_host x 2         ops.mask_border on the two masks stacked
  EDT x 2   the distance maps to the two borders         surface.edt_sq_full_host x 2    ops.edt_sq_full(invert=True), 2 images
  stats     counts, maxima, sums, the two order stats    sort + reductions in numpy      wesup_surface_stats (no read-back)
  whole     masks in, the four scores out                surface.surface_scores_host     ops.surface_stats on resident masks with
                                                                                          its one read-back + the host formulas
  whole, from numpy arrays: surface.surface_scores(device=), the upload of both masks included.

The host definition is numpy and written for exactness, not speed, so a second host yardstick stands beside it: the same scores
with scipy.ndimage.distance_transform_edt and binary_erosion (what MedPy runs).  Then the row pass's worst case at 2048 x 2048:
all foreground with one zero pixel in a corner, where every pixel scans its whole row; the host figure there is scipy's transform
(the numpy definition takes W - 1 whole-image passes on that map).

Device: `launches` back-to-back runs between two device events, `reps` times, over a ring of four scenes (the inputs are small
beside the caches: these are per-image latencies, no bandwidth claim); min, median, max per run.  Host: the wall clock, three
runs (one at 2048 x 2048).  The device results are compared with the host's before anything is timed."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scipy import ndimage

from wesup_amd import ops, surface

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--launches', type=int, default=10)
ap.add_argument('--out', default='')
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit('surface_micro.py measures the device path: it needs a GPU')

dev = torch.device('cuda:0')
TOL = 2.0
RING = 4
CROSS = ndimage.generate_binary_structure(2, 1)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def scene(H, W, seed):
    """About 25 ellipses per 522 x 775 pixels, half-axes 15 .. 60; the prediction is the truth shifted by (2, -3) and dilated twice."""
    rng = np.random.default_rng(seed)
    n = max(1, round(25 * H * W / (522 * 775)))
    yy, xx = np.mgrid[:H, :W].astype(np.float32)
    gt = np.zeros((H, W), bool)
    for _ in range(n):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        ry, rx = rng.uniform(15, 60, 2)
        y0, y1, x0, x1 = max(int(cy - ry), 0), min(int(cy + ry) + 2, H), max(int(cx - rx), 0), min(int(cx + rx) + 2, W)
        if y0 < y1 and x0 < x1:
            gt[y0:y1, x0:x1] |= ((yy[y0:y1, x0:x1] - cy) / ry) ** 2 + ((xx[y0:y1, x0:x1] - cx) / rx) ** 2 <= 1.0
    pred = ndimage.binary_dilation(np.roll(gt, (2, -3), (0, 1)), iterations=2)
    return pred, gt


def device_us(name, run):
    for i in range(RING):
        run(i)
    torch.cuda.synchronize()
    t = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(a.launches):
            run(k % RING)
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1) * 1e-3 / a.launches)
    t = np.array(t)
    say(f'{name:86s} {t.min():12.6f} {np.median(t):12.6f} {t.max():12.6f}')
    return float(np.median(t))


def host_s(name, fn, runs):
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    t = np.array(t)
    say(f'{name:86s} {t.min():12.6f} {np.median(t):12.6f} {t.max():12.6f}')
    return float(np.median(t))


def scipy_scores(pred, gt, tol):
    SP = pred & ~ndimage.binary_erosion(pred, CROSS, border_value=0)
    SG = gt & ~ndimage.binary_erosion(gt, CROSS, border_value=0)
    d_pg, d_gp = ndimage.distance_transform_edt(~SG)[SP], ndimage.distance_transform_edt(~SP)[SG]
    both = np.hstack((d_pg, d_gp))
    return {'hd': both.max(), 'hd95': np.percentile(both, 95), 'assd': (d_pg.mean() + d_gp.mean()) / 2,
            'nsd': ((d_pg <= tol).sum() + (d_gp <= tol).sum()) / both.size}


say(f'# tools/surface_micro.py on {torch.cuda.get_device_name(0)}: tolerance {TOL}; device: {a.launches} runs per measurement, '
    f'{a.reps} measurements, a ring of {RING} scenes; host: wall clock')
say(f'{"seconds per image":86s} {"min":>12s} {"median":>12s} {"max":>12s}')
for H, W in ((522, 775), (2048, 2048)):
    say('')
    say(f'== {H} x {W}')
    runs = 3 if H * W < 1 << 20 else 1
    scenes = [scene(H, W, 200 + i) for i in range(RING)]
    P = [torch.from_numpy(p).to(dev).to(torch.uint8) for p, _ in scenes]
    G = [torch.from_numpy(g).to(dev).to(torch.uint8) for _, g in scenes]
    both = [torch.cat((p[None], g[None])) for p, g in zip(P, G)]
    borders = [ops.mask_border(b) for b in both]
    d2 = [ops.edt_sq_full(b, invert=True) for b in borders]
    pred0, gt0 = scenes[0]
    ref = surface.surface_stats_host(pred0, gt0, TOL)
    got = ops.surface_stats(P[0], G[0], TOL)
    assert all(got[k] == ref[k] for k in surface.STAT_KEYS[:8]), (got, ref)
    assert all(abs(got[k] - ref[k]) <= (ref['n_p'] + ref['n_g'] + 2) * 2.0 ** -52 * ref[k] for k in surface.STAT_KEYS[8:]), (got, ref)
    s_ref, s_sp = surface.scores_from_stats(ref), scipy_scores(pred0, gt0, TOL)
    assert all(s_ref[k] == s_sp[k] for k in ('hd', 'hd95', 'nsd')) and abs(s_ref['assd'] - s_sp['assd']) <= 1e-12 * s_sp['assd']
    say(f'   scene 0: n_p {ref["n_p"]}, n_g {ref["n_g"]}, hd {s_ref["hd"]:.3f}, hd95 {s_ref["hd95"]:.3f}, assd {s_ref["assd"]:.4f}, '
        f'nsd {s_ref["nsd"]:.4f}; device, numpy host and scipy agree')

    SP, SG = surface.border_host(pred0), surface.border_host(gt0)
    h_b = host_s('host   borders: surface.border_host x 2', lambda: (surface.border_host(pred0), surface.border_host(gt0)), runs)
    h_e = host_s('host   EDT x 2: surface.edt_sq_full_host x 2',
                 lambda: (surface.edt_sq_full_host(~SG), surface.edt_sq_full_host(~SP)), runs)
    e_pg, e_gp = surface.edt_sq_full_host(~SG)[SP].astype(np.int64), surface.edt_sq_full_host(~SP)[SG].astype(np.int64)
    h_s = host_s('host   stats: sort, counts, maxima, sums of roots',
                 lambda: (np.sort(np.concatenate((e_pg, e_gp))), (e_pg <= 4).sum(), (e_gp <= 4).sum(), e_pg.max(), e_gp.max(),
                          np.sqrt(e_pg.astype(np.float64)).sum(), np.sqrt(e_gp.astype(np.float64)).sum()), runs)
    h_w = host_s('host   whole: surface.surface_scores_host', lambda: surface.surface_scores_host(pred0, gt0, TOL), runs)
    h_sp = host_s('host   whole with scipy (binary_erosion, distance_transform_edt, np.percentile)',
                  lambda: scipy_scores(pred0, gt0, TOL), 3)
    d_b = device_us('device borders: ops.mask_border, both masks in one launch', lambda i: ops.mask_border(both[i]))
    d_e = device_us('device EDT x 2: ops.edt_sq_full(invert=True), both borders in one transform',
                    lambda i: ops.edt_sq_full(borders[i], invert=True))
    stats = torch.empty(1, 10, dtype=torch.int64, device=dev)
    nb = ops._lib.load().wesup_surface_stats_workspace_bytes(1, H, W)
    ws = ops.workspace(nb, dev, 'surface')
    q_bits = np.float64(0.95).view(np.int64).item()
    d_s = device_us('device stats: wesup_surface_stats (11 launches, no read-back)',
                    lambda i: ops._lib.call('wesup_surface_stats', ops._p(borders[i][:1]), ops._p(borders[i][1:]), ops._p(d2[i][1:]),
                                            ops._p(d2[i][:1]), ops._p(stats), 1, H, W, 4, q_bits, ops._p(ws), nb, ops._stream()))
    d_w = device_us('device whole: ops.surface_stats on resident masks, read-back and formulas included',
                    lambda i: surface.scores_from_stats(ops.surface_stats(P[i], G[i], TOL)))
    d_u = device_us('device whole from numpy arrays: surface.surface_scores(device=), uploads included',
                    lambda i: surface.surface_scores(scenes[i][0], scenes[i][1], TOL, device=dev))
    say(f'   host whole / device whole at the medians: {h_w / d_w:.0f} (numpy definition), {h_sp / d_w:.0f} (scipy); '
        f'from numpy arrays: {h_w / d_u:.0f}, {h_sp / d_u:.0f}')
    say(f'   device whole below host whole: {"yes" if d_w < min(h_w, h_sp) and d_u < min(h_w, h_sp) else "NO"}')
    del P, G, both, borders, d2
    torch.cuda.empty_cache()

say('')
say('== 2048 x 2048, all foreground, one zero pixel at (0, 0): the row pass scans every row to its end')
H = W = 2048
worst = np.ones((H, W), bool)
worst[0, 0] = False
wd = torch.from_numpy(worst).to(dev).to(torch.uint8)
yy, xx = np.mgrid[:H, :W].astype(np.int64)
assert np.array_equal(ops.edt_sq_full(wd).cpu().numpy(), yy * yy + xx * xx)
h_a = host_s('host   scipy.ndimage.distance_transform_edt', lambda: ndimage.distance_transform_edt(worst), 3)
d_a = device_us('device ops.edt_sq_full, one image', lambda i: ops.edt_sq_full(wd))
blob = torch.from_numpy(scene(H, W, 200)[1]).to(dev).to(torch.uint8)
d_n = device_us('device ops.edt_sq_full, one image, the blob scene beside it', lambda i: ops.edt_sq_full(blob))
say(f'   the worst case costs {d_a / d_n:.1f} x the blob scene on the device; host (scipy) / device: {h_a / d_a:.0f}')

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
