"""Stain normalisation alone (csrc/stain.hip): the fit, the apply and fit + apply on a training batch (4 x 480 x 480) and on one
slide-sized image (8192 x 8192, the stride ops.stain_stride picks), and the numpy host path of wesup_amd.stain on the same box.

  python tools/stain_micro.py [--reps N] [--launches N] [--out profiles/stain_micro.txt]

Per line: `launches` back-to-back calls between two device events, `reps` times, the three device lines ALTERNATING inside every
repetition; min, median and max per call in us, and the bytes the algorithm moves over that time beside the HBM roofline (8.0 TB/s
peak; ~6.3 TB/s is what a streaming kernel reaches on this part).  Each call works on the next of a ring of images: three slides
(201 MB each) are past the 256 MiB Infinity Cache, the 2.8 MB batch lives in L2 whatever the ring -- its lines are launch-bound
and say so.  Bytes per sample of a fit: 3 (moments) + 3 + 4 (phi keys) + 3 + 8 (concentrations) + 12 select passes x 4 = 69;
per pixel of an apply: 3 in + 3 out.  With a stride the strided reads still fetch whole lines: the fit's figure is a lower bound
of the traffic then.

Per-kernel times come from a run of their own under the profiler, reduced by this tool (no GPU needed for the second step):

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/stain_micro.py --launches 3 --reps 2 --host-slide 512
  python tools/stain_micro.py --trace DIR/*/*_kernel_trace.csv --out profiles/stain_micro.txt        (appends the table to the file)"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=9)
ap.add_argument('--launches', type=int, default=20)
ap.add_argument('--ring', type=int, default=3)
ap.add_argument('--slide', type=int, default=8192)
ap.add_argument('--host-slide', type=int, default=4096, help='side of the image the numpy path is timed on (fp64 temporaries: 200 B / pixel)')
ap.add_argument('--out', default='')
ap.add_argument('--trace', default='', help='a rocprofv3 kernel trace (csv) of this tool: append its per-kernel table to --out and stop')
a = ap.parse_args()

# a fit: moments, eigen, phi, 4 x (hist, pick), vectors, conc, 2 x 4 x (hist, pick), final
FIT_LAUNCHES = 3 + 8 + 2 + 16 + 1
# kernel -> (bytes per item, 's' per sample of the fit / 'p' per pixel of the image) or None for the one-block kernels
KERNEL_BYTES = {'st_moments_kernel': ('3 B / sample', 3, 's'), 'st_phi_kernel': ('3 + 4 B / sample', 7, 's'),
                'st_conc_kernel': ('3 + 8 B / sample', 11, 's'), 'sel_hist_kernel': ('4 B / key', 4, 's'),
                'st_apply_kernel': ('3 + 3 B / pixel', 6, 'p'), 'sel_pick_kernel': None, 'st_eigen_kernel': None,
                'st_vectors_kernel': None, 'st_final_kernel': None}


def reduce_trace(path, slide):
    """Per kernel and shape of a traced run of this tool: launches, min / median / max us, algorithmic bytes over the median."""
    import collections
    import csv
    d = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        name = r['Kernel_Name']
        if '::sel_' not in name and '::st_' not in name:
            continue
        k = name.split('::')[1].split('(')[0]
        # the batch: grid y of the per-sample kernels, 64 threads per image of the one-block kernels of the fit
        B = int(r['Grid_Size_X']) // 64 if k in ('st_eigen_kernel', 'st_vectors_kernel', 'st_final_kernel') else int(r['Grid_Size_Y'])
        d[(k, B)].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    stride = 1
    while (-(-slide // stride)) ** 2 > 1 << 24:
        stride += 1
    shapes = {4: ('4 x 480 x 480, stride 1', 4 * 480 * 480, 4 * 480 * 480),
              1: (f'1 x {slide} x {slide}, stride {stride}', (-(-slide // stride)) ** 2, slide * slide)}
    out = ['', f'# per kernel: {os.path.basename(path)}, rocprofv3 --kernel-trace over this tool in a run of its own; us per launch (min / median / max),',
           f'# algorithmic bytes over the median beside the 8.0 TB/s HBM peak.  A fit is {FIT_LAUNCHES} launches: moments, eigen, phi, 4 x (hist, pick),',
           '# vectors, conc, 2 x 4 x (hist, pick), final.  The one-block kernels (pick, eigen, vectors, final) move a few KB: launch time.']
    for B in (4, 1):
        name, ns, npix = shapes[B]
        out.append(name)
        out.append(f'  {"kernel":20s} {"launches":>8s} {"min us":>8s} {"median":>8s} {"max":>8s}   {"bytes":>18s} {"MB":>8s} {"TB/s":>6s} {"of peak":>8s}')
        for k, info in KERNEL_BYTES.items():
            v = sorted(d[(k, B)])
            if not v:
                continue
            line = f'  {k:20s} {len(v):8d} {v[0]:8.1f} {v[len(v) // 2]:8.1f} {v[-1]:8.1f}'
            if info:
                nbytes = info[1] * (ns if info[2] == 's' else npix)
                tb = nbytes / (v[len(v) // 2] * 1e-6) / 1e12
                line += f'   {info[0]:>18s} {nbytes / 1e6:8.1f} {tb:6.2f} {tb / 8.0:8.1%}'
            out.append(line)
    return out


if a.trace:
    table = reduce_trace(a.trace, a.slide)
    print('\n'.join(table))
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(table) + '\n')
    sys.exit(0)

import torch                                         # noqa: E402  (the trace reduction above needs neither)

from wesup_amd import ops, stain as S                # noqa: E402

dev = torch.device('cuda:0')
PEAK = 8.0e12
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def he_tile(seed, n):
    """A synthetic H&E tile (n, n, 3) uint8: two gamma concentrations per pixel, 30 % near-empty background, noise."""
    rs = np.random.RandomState(seed)
    v = np.array([[0.650, 0.072], [0.704, 0.990], [0.286, 0.105]])
    v /= np.linalg.norm(v, axis=0)
    c = rs.gamma(2.0, 0.45, size=(n * n, 2))
    c[rs.rand(n * n) < 0.3] *= 0.02
    val = 240.0 * np.exp(-(c @ v.T)) - 1.0 + 1.5 * rs.standard_normal((n * n, 3))
    return np.rint(np.clip(val, 0, 255)).astype(np.uint8).reshape(n, n, 3)


def device_lines(name, imgs):
    """imgs: a ring of (B, H, W, 3) device tensors."""
    B, H, W, _ = imgs[0].shape
    stride = ops.stain_stride(H, W)
    n = -(-H // stride) * -(-W // stride)
    target = torch.from_numpy(S.default_target().astype(np.float32)).to(dev)
    outs = [torch.empty_like(i) for i in imgs]
    blocks = [ops.stain_fit(i) for i in imgs]
    cfgs = [dict(name='fit', bytes=69 * B * n, run=lambda k: ops.stain_fit(imgs[k], blocks=blocks[k])),
            dict(name='apply', bytes=6 * B * H * W, run=lambda k: ops.stain_apply(imgs[k], blocks[k], target, out=outs[k])),
            dict(name='fit + apply', bytes=69 * B * n + 6 * B * H * W,
                 run=lambda k: ops.stain_apply(imgs[k], ops.stain_fit(imgs[k], blocks=blocks[k]), target, out=outs[k]))]
    for c in cfgs:
        c['t'] = []
        for k in range(len(imgs)):
            c['run'](k)
    torch.cuda.synchronize()
    assert all(float(b[:, 15].min()) == 1.0 for b in blocks), 'a fit of the synthetic images is invalid'
    for rep in range(a.reps):
        for c in cfgs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(a.launches):
                c['run'](k % len(imgs))
            e1.record()
            e1.synchronize()
            c['t'].append(e0.elapsed_time(e1) * 1e3 / a.launches)
    say(f'{name}: {B} x {H} x {W}, stride {stride} ({n} samples per image), ring of {len(imgs)}')
    say(f'  {"call":12s} {"MB moved":>9s} {"min us":>10s} {"median":>10s} {"max":>10s}   {"TB/s at median":>14s} {"of 8.0 TB/s":>11s}')
    for c in cfgs:
        t = np.array(c['t'])
        tb = c['bytes'] / (np.median(t) * 1e-6)
        say(f'  {c["name"]:12s} {c["bytes"] / 1e6:9.1f} {t.min():10.1f} {np.median(t):10.1f} {t.max():10.1f}   {tb / 1e12:14.3f} {tb / PEAK:11.1%}')
    return outs[0]


def host_line(name, imgs):
    norm = S.StainNormalizer(host=True)
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        out = norm(imgs)
        t.append(time.perf_counter() - t0)
    say(f'{name}: numpy host path, fit + apply, {imgs.shape}: min {min(t) * 1e3:.1f} ms, median {sorted(t)[1] * 1e3:.1f} ms '
        f'({imgs.size / 3 / sorted(t)[1] / 1e6:.2f} Mpixel/s)')
    return out


say(f'# tools/stain_micro.py on {torch.cuda.get_device_name(0)}: {a.launches} calls per measurement, {a.reps} measurements per line, alternating')
batch = np.stack([he_tile(s, 480) for s in range(4)])
got = device_lines('training batch', [torch.from_numpy(batch).to(dev) for _ in range(a.ring)])
want = host_line('training batch', batch)
say(f'  device vs host output: {int((got.cpu().numpy() != want).sum())} of {want.size} values differ (float32 chain against float64, by one level)')
tile = torch.from_numpy(he_tile(9, 512)).to(dev)
reps = a.slide // 512
slides = [tile.repeat(reps, reps, 1)[None].contiguous() for _ in range(a.ring)]
device_lines('slide', slides)
del slides
h = a.host_slide // 512
host_line('slide (a part of it)', np.tile(he_tile(9, 512), (h, h, 1)))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
