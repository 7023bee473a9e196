"""The kernels that split touching objects (csrc/split.hip) beside what a user could do without them.  No speed
was fixed in advance.  At 522 x 775 (GlaS) and 1500 x 1500 (CRAG), random overlapping discs, radius 20:

  (1) the whole ops.split_objects against the host split.split_objects (numpy + scipy.ndimage.label), at B = 1 and B = 8;
  (2) ops.edt_sq at cap 15^2 against the one composition that yields seeds today: ops.binary_morph erosion with the 31 x 31 disc
      footprint (709 cells, the largest disc its 1024-cell limit allows; its border rule differs, so only the times compare);
  (3) the phases of ops.split_objects at B = 1: distance map, seeds (compare + cc_label), growth, cut; the growth's launch count,
      and the growth alone at several read-back cadences (launches between two reads of the changed word).

  python tools/split_micro.py [--reps N] [--launches N] [--ring-mb MB] [--out profiles/split_micro.txt]

Per path: `launches` back-to-back runs between two device events, `reps` times, the paths of a group ALTERNATING inside every
repetition; min, median and max per run in us.  Each run of a series works on the next of a ring of input masks whose sum is well
past the 256 MiB Infinity Cache, so every input comes from HBM (the outputs and intermediates are torch allocations and the
library's workspace: the same blocks every run).  The growth reads one word
back per group of launches, so its figures include those host round trips: they are part of what a caller waits for.  The host
path is timed with the wall clock, three runs (one at B = 8)."""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from wesup_amd import ops, split

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--launches', type=int, default=10)
ap.add_argument('--ring-mb', type=float, default=768.0, help='the input masks of a case add up to at least this')
ap.add_argument('--out', default='')
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit('split_micro.py measures the device path: it needs a GPU')

dev = torch.device('cuda:0')
RADIUS = 20
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def scene(H, W, seed):
    """Random discs, about 25 per 522 x 775 pixels, radii 22 .. 59: many of them overlap."""
    rng = np.random.default_rng(seed)
    n = max(1, round(25 * H * W / (522 * 775)))
    yy, xx = np.mgrid[:H, :W].astype(np.int32)
    F = np.zeros((H, W), np.uint8)
    for _ in range(n):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(22, 60)
        F[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    return F


def measure(cfgs, ring, launches=None):
    """The alternating series of tta_micro.py; returns the medians in us."""
    launches = launches or a.launches
    for c in cfgs:                                   # warm-up: code objects, workspaces, every mask of the ring touched
        c['t'] = []
        for i in range(ring):
            c['run'](i)
    torch.cuda.synchronize()
    for rep in range(a.reps):
        for c in cfgs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(launches):
                c['run'](k % ring)
            e1.record()
            e1.synchronize()
            c['t'].append(e0.elapsed_time(e1) * 1e3 / launches)
    for c in cfgs:
        t = np.array(c['t'])
        say(f'{c["name"]:72s} {ring:4d} {t.min():10.1f} {np.median(t):10.1f} {t.max():10.1f}')
    return [float(np.median(c['t'])) for c in cfgs]


def host_seconds(F, runs):
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        split.split_objects(F, RADIUS)
        t.append(time.perf_counter() - t0)
    return np.array(t)


yy, xx = np.mgrid[-15:16, -15:16]
DISC31 = torch.from_numpy((yy * yy + xx * xx <= 15 * 15).astype(np.uint8)).to(dev)

say(f'# tools/split_micro.py on {torch.cuda.get_device_name(0)}: radius {RADIUS}; {a.launches} runs per measurement, {a.reps} '
    f'measurements per path, alternating; the input masks of a case add up to >= {a.ring_mb:.0f} MB; read-back cadence of the '
    f'growth {ops.GROW_CADENCE} launches of {ops.GROW_ROUNDS} rounds')
say(f'{"path":72s} {"ring":>4s} {"min us":>10s} {"median":>10s} {"max":>10s}')
for H, W in ((522, 775), (1500, 1500)):
    say('')
    say(f'== {H} x {W}')
    ring = max(3, math.ceil(a.ring_mb * 1e6 / (H * W)))
    base = [scene(H, W, 100 + i) for i in range(4)]                       # four scenes, turned over: a ring of different masks
    masks_np = [np.ascontiguousarray(base[i % 4][::-1] if (i // 4) % 2 else base[i % 4]) for i in range(ring)]
    masks = [torch.from_numpy(m).to(dev) for m in masks_np]
    assert np.array_equal(ops.split_objects(masks[0], RADIUS).cpu().numpy(), split.split_objects(masks_np[0], RADIUS))

    # (1) the whole split, B = 1
    (dev_us,) = measure([dict(name='(1) ops.split_objects, B = 1', run=lambda i: ops.split_objects(masks[i], RADIUS))], ring)
    ht = host_seconds(masks_np[0], 3)
    say(f'{"(1) split.split_objects on the host, B = 1 (wall clock, 3 runs)":72s} {"":4s} {ht.min() * 1e6:10.0f} '
        f'{np.median(ht) * 1e6:10.0f} {ht.max() * 1e6:10.0f}')
    say(f'    host / device at the medians: {np.median(ht) * 1e6 / dev_us:.0f}')

    # (2) the seeds' distance map against the footprint erosion, radius 15
    e_us, m_us = measure([dict(name='(2) ops.edt_sq, cap 15^2', run=lambda i: ops.edt_sq(masks[i], 225)),
                          dict(name='(2) ops.binary_morph erosion, 31 x 31 disc (709 cells)',
                               run=lambda i: ops.binary_morph(masks[i], DISC31, ops.MORPH_ERODE))], ring)
    say(f'    footprint erosion / distance map at the medians: {m_us / e_us:.2f}')

    # (3) the phases at B = 1
    r2 = RADIUS * RADIUS
    d2s = [ops.edt_sq(m, r2) for m in masks]
    seeds = [ops.cc_label((d >= r2).to(torch.uint8))[0] for d in d2s]
    grown = [ops.label_grow(m, s, return_launches=True) for m, s in zip(masks, seeds)]
    labels, n_launch = [g[0] for g in grown], [g[1] for g in grown]
    rounds = [split.label_grow_host(masks_np[i], seeds[i].cpu().numpy(), True)[1] for i in range(min(ring, 4))]
    say(f'    growth: {min(rounds)} .. {max(rounds)} rounds on the host over the first scenes; {min(n_launch)} .. {max(n_launch)} '
        f'launches of {ops.GROW_ROUNDS} rounds on the device at cadence {ops.GROW_CADENCE}')
    ph = measure([dict(name='(3) distance map: ops.edt_sq, cap 20^2', run=lambda i: ops.edt_sq(masks[i], r2)),
                  dict(name='(3) seeds: compare + ops.cc_label', run=lambda i: ops.cc_label((d2s[i] >= r2).to(torch.uint8))),
                  dict(name=f'(3) growth: ops.label_grow, cadence {ops.GROW_CADENCE}', run=lambda i: ops.label_grow(masks[i], seeds[i])),
                  dict(name='(3) cut: ops.label_cut', run=lambda i: ops.label_cut(masks[i], labels[i]))], ring)
    tot = sum(ph)
    say('    shares of the four phases: ' + ' / '.join(f'{100 * p / tot:.0f} %' for p in ph) + f' of {tot:.1f} us')
    measure([dict(name=f'(3) growth alone, cadence {c}', run=lambda i, c=c: ops.label_grow(masks[i], seeds[i], cadence=c))
             for c in (1, 2, 4, 8)], ring)
    del d2s, seeds, grown, labels

    # (1) the whole split, B = 8
    nb = max(3, ring // 8)
    batches = [torch.stack([masks[(8 * j + k) % ring] for k in range(8)]) for j in range(nb)]
    (dev8,) = measure([dict(name='(1) ops.split_objects, B = 8', run=lambda i: ops.split_objects(batches[i], RADIUS))], nb,
                      launches=max(2, a.launches // 2))
    ht8 = host_seconds(batches[0].cpu().numpy(), 1)
    say(f'{"(1) split.split_objects on the host, B = 8 (wall clock, 1 run)":72s} {"":4s} {"":10s} {ht8[0] * 1e6:10.0f}')
    say(f'    host / device: {ht8[0] * 1e6 / dev8:.0f}')
    del masks, batches
    torch.cuda.empty_cache()

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
