"""The class-map kernels of csrc/classmap.hip beside what the same run could do before them.  No speed was
fixed in advance; the yardstick is the composition of the one-plane entries and torch:

  (a) resize + argmax at 261 x 388 -> 522 x 775: C calls of ops.plane_resize_acc (one per class, into a (C, H, W) buffer) followed
      by torch.argmax, against ops.planes_resize_acc + ops.class_argmax_u8;
  (b) merge + argmax at 1000 x 1400, p = 464 (12 windows): ops.window_merge to the (H, W, C) fp64 tensor followed by torch.argmax,
      against ops.window_merge_classes;

each for C = 3 and C = 16.

  python tools/classmap_micro.py [--reps N] [--launches N] [--out profiles/classmap_micro.txt]

Per path: `launches` back-to-back runs of the whole path between two device events, `reps` times, the paths ALTERNATING inside
every repetition (whatever else the box does hits all of them alike); min, median and max per run in us.  Each run of a series
works on the next of a ring of buffer sets whose sum is well past the 256 MiB Infinity Cache: HBM figures.  MB: the bytes a path
cannot avoid -- every input read once, every output written once, every intermediate written once and read once."""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from wesup_amd import infer_tile, ops

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=15)
ap.add_argument('--launches', type=int, default=100)
ap.add_argument('--ring-mb', type=float, default=768.0, help='the buffer sets of a case add up to at least this')
ap.add_argument('--out', default='')
a = ap.parse_args()

dev = torch.device('cuda:0')
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def ring_of(set_bytes):
    return max(3, math.ceil(a.ring_mb * 1e6 / set_bytes))


def resize_case(C):
    h, w, H, W = 261, 388, 522, 775
    set_bytes = 4 * C * (h * w + 2 * H * W) + 9 * H * W           # (every buffer of a set)
    ring = ring_of(set_bytes)
    g = torch.Generator(device=dev).manual_seed(C)
    sets = [dict(src=torch.rand(h, w, C, device=dev, generator=g), planes=torch.empty(C, H, W, device=dev),
                 hwc=torch.empty(H, W, C, device=dev), u8=torch.empty(H, W, dtype=torch.uint8, device=dev),
                 idx=torch.empty(H, W, dtype=torch.int64, device=dev)) for _ in range(ring)]

    def old(i):
        s = sets[i]
        for c in range(C):
            ops.plane_resize_acc(s['src'][..., c], s['planes'][c])
        torch.argmax(s['planes'], dim=0, out=s['idx'])               # (into a buffer, as the new path writes into one)

    def new(i):
        s = sets[i]
        ops.planes_resize_acc(s['src'], s['hwc'])
        ops.class_argmax_u8(s['hwc'], out=s['u8'])

    def check():
        old(0); new(0)
        assert torch.equal(sets[0]['idx'].to(torch.uint8), sets[0]['u8'])
    inp, planes = 4.0 * C * h * w, 4.0 * C * H * W
    return [dict(name=f'(a) C={C:2d}  {C} x plane_resize_acc + torch.argmax', run=old, bytes=inp + 2 * planes + 8.0 * H * W),
            dict(name=f'(a) C={C:2d}  planes_resize_acc + class_argmax_u8', run=new, bytes=inp + 2 * planes + 1.0 * H * W)], ring, check


def merge_case(C):
    H, W, p = 1000, 1400, 464
    tops, lefts = infer_tile.window_grid(H, W, p)
    N = len(tops) * len(lefts)
    set_bytes = 4 * N * p * p * C + 8 * H * W * C + 9 * H * W
    ring = ring_of(set_bytes)
    g = torch.Generator(device=dev).manual_seed(100 + C)
    sets = [dict(pred=torch.rand(N, p, p, C, device=dev, generator=g), f64=torch.empty(H, W, C, dtype=torch.float64, device=dev),
                 u8=torch.empty(H, W, dtype=torch.uint8, device=dev), st=torch.zeros(1, dtype=torch.int32, device=dev),
                 idx=torch.empty(H, W, dtype=torch.int64, device=dev)) for _ in range(ring)]

    def old(i):
        s = sets[i]
        ops.window_merge(s['pred'], tops, lefts, H, W, out=s['f64'])
        torch.argmax(s['f64'], dim=-1, out=s['idx'])

    def new(i):
        s = sets[i]
        ops.window_merge_classes(s['pred'], tops, lefts, H, W, out=s['u8'], status=s['st'])

    def check():
        old(0); new(0)
        assert torch.equal(sets[0]['idx'].to(torch.uint8), sets[0]['u8'])
    inp, f64 = 4.0 * N * p * p * C, 8.0 * H * W * C
    return [dict(name=f'(b) C={C:2d}  window_merge (fp64) + torch.argmax', run=old, bytes=inp + 2 * f64 + 8.0 * H * W),
            dict(name=f'(b) C={C:2d}  window_merge_classes', run=new, bytes=inp + 1.0 * H * W)], ring, check


say(f'# tools/classmap_micro.py on {torch.cuda.get_device_name(0)}: {a.launches} runs per measurement, {a.reps} measurements per path, '
    f'alternating; buffer sets of a case add up to >= {a.ring_mb:.0f} MB')
say(f'{"path":52s} {"ring":>4s} {"MB":>8s} {"min us":>9s} {"median":>9s} {"max":>9s} {"TB/s at median":>15s}')
for make, C in ((resize_case, 3), (resize_case, 16), (merge_case, 3), (merge_case, 16)):
    cfgs, ring, check = make(C)
    check()                                          # the two paths give the same class map
    for c in cfgs:                                   # warm-up: code objects, every buffer of the ring touched
        c['t'] = []
        for i in range(ring):
            c['run'](i)
    torch.cuda.synchronize()
    for rep in range(a.reps):
        for c in cfgs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(a.launches):
                c['run'](k % ring)
            e1.record()
            e1.synchronize()
            c['t'].append(e0.elapsed_time(e1) * 1e3 / a.launches)          # us per run of the path
    for c in cfgs:
        t = np.array(c['t'])
        say(f'{c["name"]:52s} {ring:4d} {c["bytes"] / 1e6:8.1f} {t.min():9.2f} {np.median(t):9.2f} {t.max():9.2f} '
            f'{c["bytes"] / 1e12 / (np.median(t) * 1e-6):15.3f}')
    old_t, new_t = np.median(cfgs[0]['t']), np.median(cfgs[1]['t'])
    say(f'    median time old / new {old_t / new_t:.2f}, bytes old / new {cfgs[0]["bytes"] / cfgs[1]["bytes"]:.2f}')
    del cfgs, check
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
