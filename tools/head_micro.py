"""The classifier kernels alone: wesup_classifier_fwd (two classes, the kernel every commit so far has had) beside
wesup_classifier_fwd_c (2 <= C <= 16) at C = 2, 3, 8, 16, D = 32, for the pixel-inference size R = 480*480 and the step's R = 4*576.

  python tools/head_micro.py [--reps N] [--launches N] [--out profiles/head_micro.txt]

Per configuration: `launches` back-to-back launches between two device events, `reps` times, the configurations ALTERNATING inside
every repetition (whatever else the box does hits all of them alike); median and min .. max per launch, and GB/s on the model
R * (D + C) * 4 bytes (every feature read once, every probability written once).  Each launch of a series works on the next of
a ring of buffers larger than the 256 MiB Infinity Cache, so the R = 480*480 figure is an HBM figure; the R = 4*576 launch is
3 us of work and measures the launch rate.  Results of both entries at C = 2 are compared bit for bit before anything is timed."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from wesup_amd import _lib, ops

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=15)
ap.add_argument('--launches', type=int, default=100)
ap.add_argument('--out', default='')
a = ap.parse_args()

dev = torch.device('cuda:0')
lib = _lib.load()
D = 32
RING_BYTES = 640 << 20
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def p(t):
    return ops._p(t)


say(f'# tools/head_micro.py on {torch.cuda.get_device_name(0)}: {a.launches} launches per measurement, {a.reps} measurements per '
    f'configuration, alternating; D = {D}')
for R, what in ((480 * 480, 'pixel inference, one 480x480 image'), (4 * 576, "the step's superpixel rows, 4 x 576")):
    n_ring = max(2, min(64, -(-RING_BYTES // (R * (D + 16) * 4))))
    rs = np.random.RandomState(R % 1000)
    feats = [torch.from_numpy(np.maximum(rs.randn(R, D), 0).astype(np.float32)).to(dev) for _ in range(n_ring)]
    cfgs = []
    for name, C in (('wesup_classifier_fwd', 2), ('wesup_classifier_fwd_c', 2), ('wesup_classifier_fwd_c', 3),
                    ('wesup_classifier_fwd_c', 8), ('wesup_classifier_fwd_c', 16)):
        Wc = torch.from_numpy((rs.randn(C, D) * 0.2).astype(np.float32)).to(dev)
        bc = torch.from_numpy((rs.randn(C) * 0.05).astype(np.float32)).to(dev)
        outs = [torch.empty(R, C, device=dev) for _ in range(n_ring)]
        fn = getattr(lib, name)
        if name == 'wesup_classifier_fwd':
            run = lambda i, fn=fn, Wc=Wc, bc=bc, outs=outs: fn(p(feats[i]), p(Wc), p(bc), p(outs[i]), R, D, ops._stream())
        else:
            run = lambda i, fn=fn, Wc=Wc, bc=bc, outs=outs, C=C: fn(p(feats[i]), p(Wc), p(bc), p(outs[i]), R, D, C, ops._stream())
        cfgs.append(dict(name=name, C=C, run=run, outs=outs, Wc=Wc, bc=bc, t=[]))
    # same bits at C = 2 (same weights: re-run the generic entry with the old entry's)
    old, new = cfgs[0], cfgs[1]
    assert old['run'](0) == 0
    assert lib.wesup_classifier_fwd_c(p(feats[0]), p(old['Wc']), p(old['bc']), p(new['outs'][0]), R, D, 2, ops._stream()) == 0
    torch.cuda.synchronize()
    same = torch.equal(old['outs'][0], new['outs'][0])
    assert same, 'wesup_classifier_fwd_c at C = 2 differs from wesup_classifier_fwd'
    for c in cfgs:                                   # warm-up: code objects, every buffer of the ring touched
        for i in range(n_ring):
            assert c['run'](i) == 0
    torch.cuda.synchronize()
    for rep in range(a.reps):
        for c in cfgs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(a.launches):
                c['run'](k % n_ring)
            e1.record()
            e1.synchronize()
            c['t'].append(e0.elapsed_time(e1) * 1e3 / a.launches)          # us per launch
    say(f'\nR = {R} ({what}); ring of {n_ring} buffer pairs; both entries give the same bits at C = 2: {same}')
    say(f'{"entry":26s} {"C":>3s} {"median us":>10s} {"min":>8s} {"max":>8s} {"model MB":>9s} {"GB/s (median)":>14s}')
    for c in cfgs:
        t = np.array(c['t'])
        mb = R * (D + c['C']) * 4 / 1e6
        say(f'{c["name"]:26s} {c["C"]:3d} {np.median(t):10.2f} {t.min():8.2f} {t.max():8.2f} {mb:9.2f} {mb / 1e3 / (np.median(t) * 1e-6):14.1f}')
    t_old, t_new = np.array(cfgs[0]['t']), np.array(cfgs[1]['t'])
    say(f'generic / two-class kernel at C = 2: median ratio {np.median(t_new) / np.median(t_old):.3f}; the two-class kernel\'s own '
        f'spread (max / min) {t_old.max() / t_old.min():.3f}')
    del feats, cfgs
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
