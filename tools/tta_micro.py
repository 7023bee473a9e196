"""The view kernels of test-time augmentation (csrc/tiles.hip, csrc/classmap.hip) beside what the same run could
do with torch, and beside the forward pass they stand around.  No speed was fixed in advance; the yardstick is the composition of
the entries without views and ``torch.rot90`` / ``torch.flip`` copies, at 1000 x 1400, p = 464 (12 windows) under all eight views:

  (a) gather: ops.window_gather of the 12 windows, then per view one torch flip / rot90 copy into the (12, 8, 3, p, p) input, against
      ops.window_gather(views=...) of the 96 slots;
  (b) merge, C = 1 and C = 3: per view one inverse torch rot90 / flip copy into an upright (12, p, p, 8 C) buffer, ops.window_merge
      over it and the mean over the views, against ops.window_merge(views=...) (the composition adds in another order: equal to rounding,
      not bit for bit);
  (c) class merge, C = 3 probabilities: (b)'s composition followed by torch.argmax, against ops.window_merge_classes(views=...);
  (d) one view at a time: the gather and the merge of all 12 windows under the single view 0, 4 (mirror), 2 (half turn), 1 and 3
      (odd quarter turns: a wave's source reads are one image row, resp. one window row, apart);
  (e) one forward pass of the superpixel model at batch 4, p = 464 (GPU SLIC, the network, the painted map), next to one gather
      pass of 4 slots and the share of one merge that falls to 4 slots.

  python tools/tta_micro.py [--reps N] [--launches N] [--out profiles/tta_micro.txt]

Per path: `launches` back-to-back runs of the whole path between two device events, `reps` times, the paths ALTERNATING inside
every repetition; min, median and max per run in us.  Each run of a series works on the next of a ring of buffer sets whose sum
is well past the 256 MiB Infinity Cache: HBM figures.  MB: the bytes a path cannot avoid -- every input read once, every output
written once, every intermediate written once and read once."""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from wesup_amd import infer_tile, ops

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--launches', type=int, default=20)
ap.add_argument('--ring-mb', type=float, default=768.0, help='the buffer sets of a case add up to at least this')
ap.add_argument('--out', default='')
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit('tta_micro.py measures the device path: it needs a GPU')

dev = torch.device('cuda:0')
H, W, P = 1000, 1400, 464
D4 = infer_tile.VIEW_SETS['d4']
tops, lefts = infer_tile.window_grid(H, W, P)
N = len(tops) * len(lefts)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def ring_of(set_bytes):
    return max(3, math.ceil(a.ring_mb * 1e6 / set_bytes))


def torch_view(x, v, dims):
    """apply_view on the two dimensions ``dims`` = (rows, columns) of a tensor (a view of x: the copy is the caller's)."""
    r, f = v & 3, v >> 2
    return torch.rot90(x.flip(dims[1]) if f else x, r, dims)


def torch_inverse(x, v, dims):
    r, f = v & 3, v >> 2
    x = torch.rot90(x, -r, dims)
    return x.flip(dims[1]) if f else x


def image(seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randint(0, 256, (H, W, 3), device=dev, generator=g, dtype=torch.uint8)


def gather_case(views=D4, old=True):
    V = len(views)
    set_bytes = 3 * H * W + 12 * N * P * P * (V + (1 if old else 0))
    ring = ring_of(set_bytes)
    sets = [dict(img=image(i), plain=torch.empty(N, 3, P, P, device=dev) if old else None,
                 turned=torch.empty(N, V, 3, P, P, device=dev) if old else None, x=torch.empty(N * V, 3, P, P, device=dev))
            for i in range(ring)]

    def composed(i):
        s = sets[i]
        ops.window_gather(s['img'], tops, lefts, P, 0, N, out=s['plain'])
        for t, v in enumerate(views):
            s['turned'][:, t].copy_(torch_view(s['plain'], v, (2, 3)))

    def new(i):
        s = sets[i]
        ops.window_gather(s['img'], tops, lefts, P, 0, N * V, out=s['x'], views=views)

    def check():
        composed(0); new(0)
        assert torch.equal(sets[0]['turned'].view(N * V, 3, P, P), sets[0]['x'])
    win = 3.0 * N * P * P                                           # the bytes of the windows, read once
    name = f'views {views}' if V < 8 else 'all eight views'
    cfgs = [dict(name=f'(a) window_gather + {V} torch view copies', run=composed, bytes=win + 4 * win * (1 + 2 * V)),
            dict(name=f'(a) window_gather(views), {name}', run=new, bytes=win * V + 4 * win * V)]
    return (cfgs if old else cfgs[1:]), ring, (check if old else None)


def merge_case(C, classes=False, views=D4, old=True):
    V = len(views)
    pred_b, f64 = 4 * N * V * P * P * C, 8 * H * W * C
    set_bytes = pred_b * (2 if old else 1) + f64 * ((V + 1) if old else 1) + 9 * H * W
    ring = ring_of(set_bytes)
    g = torch.Generator(device=dev).manual_seed(7 + C)
    sets = [dict(pred=torch.rand(N, V, P, P, C, device=dev, generator=g),
                 upright=torch.empty(N, P, P, V, C, device=dev) if old else None,
                 per_view=torch.empty(H, W, V * C, dtype=torch.float64, device=dev) if old else None,
                 f64=torch.empty(H, W, C, dtype=torch.float64, device=dev), f64_new=torch.empty(H, W, C, dtype=torch.float64, device=dev),
                 idx=torch.empty(H, W, dtype=torch.int64, device=dev), u8=torch.empty(H, W, dtype=torch.uint8, device=dev),
                 st=torch.zeros(1, dtype=torch.int32, device=dev)) for _ in range(ring)]

    def composed(i):
        s = sets[i]
        for t, v in enumerate(views):
            s['upright'][:, :, :, t].copy_(torch_inverse(s['pred'][:, t], v, (1, 2)))
        ops.window_merge(s['upright'].view(N, P, P, V * C), tops, lefts, H, W, out=s['per_view'])
        torch.mean(s['per_view'].view(H, W, V, C), dim=2, out=s['f64'])
        if classes:
            torch.argmax(s['f64'], dim=-1, out=s['idx'])

    def new(i):
        s = sets[i]
        if classes:
            ops.window_merge_classes(s['pred'], tops, lefts, H, W, out=s['u8'], status=s['st'], views=views)
        else:
            ops.window_merge(s['pred'], tops, lefts, H, W, out=s['f64_new'], views=views)

    def check():
        composed(0); new(0)
        s = sets[0]
        if classes:
            differ = int((s['idx'].to(torch.uint8) != s['u8']).sum())
            say(f'    (c) C={C}: {differ} of {H * W} classes differ between the two orders of the sum')
            assert differ <= H * W // 10000
        else:
            err = float((s['f64'] - s['f64_new']).abs().max())
            say(f'    (b) C={C}: max |composition - window_merge(views)| = {err:.2e} (another order of the sum)')
            assert err < 1e-12
    tag = '(c)' if classes else '(b)'
    name = f'views {views}' if V < 8 else 'all eight views'
    tail_old = 8.0 * H * W if classes else 0.0
    cfgs = [dict(name=f'{tag} C={C}  {V} inverse copies + window_merge + mean' + (' + argmax' if classes else ''), run=composed,
                 bytes=3.0 * pred_b + 2.0 * V * f64 + (2.0 if classes else 1.0) * f64 + tail_old),
            dict(name=f'{tag} C={C}  window_merge{"_classes" if classes else ""}(views), {name}', run=new,
                 bytes=1.0 * pred_b + (1.0 * H * W if classes else 1.0 * f64))]
    return (cfgs if old else cfgs[1:]), ring, (check if old else None)


def measure(cfgs, ring, check, launches=None):
    """The alternating series of classmap_micro.py; returns the medians in us."""
    launches = launches or a.launches
    if check is not None:
        check()
    for c in cfgs:                                   # warm-up: code objects, every buffer of the ring touched
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
            c['t'].append(e0.elapsed_time(e1) * 1e3 / launches)            # us per run of the path
    for c in cfgs:
        t = np.array(c['t'])
        say(f'{c["name"]:64s} {ring:4d} {c["bytes"] / 1e6:8.1f} {t.min():9.1f} {np.median(t):9.1f} {t.max():9.1f} '
            f'{c["bytes"] / 1e12 / (np.median(t) * 1e-6):15.3f}')
    return [float(np.median(c['t'])) for c in cfgs]


say(f'# tools/tta_micro.py on {torch.cuda.get_device_name(0)}: {H} x {W}, p = {P}, {N} windows; {a.launches} runs per measurement, '
    f'{a.reps} measurements per path, alternating; buffer sets of a case add up to >= {a.ring_mb:.0f} MB')
say(f'{"path":64s} {"ring":>4s} {"MB":>8s} {"min us":>9s} {"median":>9s} {"max":>9s} {"TB/s at median":>15s}')
d4_us = {}
for what, make in (('gather', lambda: gather_case()), ('merge C=1', lambda: merge_case(1)), ('merge C=3', lambda: merge_case(3)),
                   ('classes C=3', lambda: merge_case(3, classes=True))):
    cfgs, ring, check = make()
    old_t, new_t = measure(cfgs, ring, check)
    d4_us[what] = new_t
    say(f'    median time composition / view kernel {old_t / new_t:.2f}, bytes {cfgs[0]["bytes"] / cfgs[1]["bytes"]:.2f}')
    del cfgs, check
    torch.cuda.empty_cache()

say('')
say(f'(d) one view at a time, all {N} windows: the stride of the source reads')
one = {}
for v in (0, 4, 2, 1, 3):
    for what, make in (('gather', lambda: gather_case((v,), old=False)), ('merge C=1', lambda: merge_case(1, views=(v,), old=False))):
        cfgs, ring, check = make()
        one[what, v] = measure(cfgs, ring, check)[0]
        del cfgs
        torch.cuda.empty_cache()
for what in ('gather', 'merge C=1'):
    say(f'    {what}: time under view 4 / 2 / 1 / 3 over time under view 0: ' +
        ' / '.join(f'{one[what, v] / one[what, 0]:.2f}' for v in (4, 2, 1, 3)))

say('')
say('(e) one forward pass of the superpixel model at batch 4 (GPU SLIC + network + painted map), p = 464, beside the view kernels')
from oracle import wesup_oracle as orc                      # noqa: E402
from wesup_amd.models import initialize_trainer             # noqa: E402
trainer = initialize_trainer('wesup', device='cuda:0')
trainer.model.load_state_dict({k: torch.from_numpy(v) for k, v in orc.make_weights(3).items()})
trainer.model.eval()
img_d = image(99)
B = 4
x = torch.empty(B, 3, P, P, device=dev)
passes = [(first, D4) for first in range(0, N * 8, B)]


def forward():
    with torch.no_grad():
        input_, _ = trainer.preprocess(x)
        return trainer.model(input_)


def gather_pass(k):
    ops.window_gather(img_d, tops, lefts, P, passes[k % len(passes)][0], B, out=x, views=D4)


gather_pass(1)                                       # (slots 4 .. 7: the views 4 .. 7 of window 0)
for _ in range(3):
    forward()
torch.cuda.synchronize()
fwd, gat = [], []
for rep in range(a.reps):
    for series, run, n in ((fwd, lambda k: forward(), 3), (gat, gather_pass, len(passes))):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(n):
            run(k)
        e1.record()
        e1.synchronize()
        series.append(e0.elapsed_time(e1) * 1e3 / n)
fwd_us, gat_us = float(np.median(fwd)), float(np.median(gat))
merge_share = d4_us['merge C=1'] * B / (N * 8)
say(f'    forward pass, batch {B}:                         median {fwd_us:10.1f} us (min {min(fwd):.1f}, max {max(fwd):.1f})')
say(f'    window_gather(views), one pass of {B} slots:     median {gat_us:10.1f} us (min {min(gat):.1f}, max {max(gat):.1f}; all 24 passes '
    f'of the 96 slots in turn, every view among them)')
say(f'    window_merge(views) C=1, the share of {B} slots: {merge_share:10.1f} us ({d4_us["merge C=1"]:.1f} us once per image / 24 passes)')
say(f'    gather + merge share over the forward pass: {(gat_us + merge_share) / fwd_us:.4f}')
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
