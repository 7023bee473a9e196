"""The optimiser kernels alone, at the model's flat parameter count: wesup_adam_step (Adam and AdamW) beside wesup_sgd_step, the
kernel every commit so far has had and the only yardstick there is -- both stream the flat buffers once, 28 resp. 20 bytes per
element (p, g, m, v in, p, m, v out / p, g, v in, p, v out).

  python tools/optim_micro.py [--reps N] [--launches N] [--out profiles/optim_micro.txt]

Per kernel: `launches` back-to-back launches between two device events, `reps` times, the kernels ALTERNATING inside every
repetition (whatever else the box does hits all of them alike); min, median and max per launch in us and in TB/s.  Each launch of
a series works on the next of a ring of buffer sets; one set alone (226 resp. 302 MB) is about the size of the 256 MiB Infinity
Cache, three of them are well past it: HBM figures.  The Adam launches read their factors from a device block one tick has filled
(the tick, one thread, is timed on its own line)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from wesup_amd import _lib, ops
from wesup_amd.models.wesup import WESUP

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=15)
ap.add_argument('--launches', type=int, default=100)
ap.add_argument('--ring', type=int, default=3)
ap.add_argument('--out', default='')
a = ap.parse_args()

dev = torch.device('cuda:0')
lib = _lib.load()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def p(t):
    return ops._p(t)


# the flat buffer's length: every parameter of WESUP in a slot of whole 64-float lines (models/wesup.py _ensure_engine)
N = sum((q.numel() + 63) // 64 * 64 for q in WESUP().parameters())
g = torch.Generator(device=dev).manual_seed(0)
sets = []
for _ in range(a.ring):
    P, G = torch.randn(N, device=dev, generator=g) * 0.03, torch.randn(N, device=dev, generator=g) * 1e-3
    sets.append(dict(p=P, g=G, m=torch.zeros_like(P), v=torch.zeros_like(P), buf=torch.zeros_like(P)))       # (buf: SGD's momentum)
state = ops.adam_state(5e-5, dev)
betas, omb = (0.9, 0.999), (1.0 - 0.9, 1.0 - 0.999)
ops.adam_tick(state, betas, 1e-3)


def adam(decoupled):
    def run(i):
        s = sets[i]
        return lib.wesup_adam_step(p(s['p']), p(s['g']), p(s['m']), p(s['v']), N, p(state), betas[0], omb[0], betas[1], omb[1], 1e-8,
                                   1e-3, 1.0, decoupled, ops._stream())
    return run


def sgd(i):
    s = sets[i]
    return lib.wesup_sgd_step(p(s['p']), p(s['g']), p(s['buf']), N, 5e-5, 0.9, 1e-3, 1.0, 0, ops._stream())


def tick(i):
    return lib.wesup_adam_tick(p(state), omb[0], omb[1], 1e-3, ops._stream())


cfgs = [dict(name='wesup_sgd_step', run=sgd, bytes=20, t=[]), dict(name='wesup_adam_step (Adam)', run=adam(0), bytes=28, t=[]),
        dict(name='wesup_adam_step (AdamW)', run=adam(1), bytes=28, t=[]), dict(name='wesup_adam_tick', run=tick, bytes=0, t=[])]
say(f'# tools/optim_micro.py on {torch.cuda.get_device_name(0)}: n = {N} floats ({N * 4 / 1e6:.1f} MB per buffer), ring of {a.ring} buffer '
    f'sets, {a.launches} launches per measurement, {a.reps} measurements per kernel, alternating')
for c in cfgs:                                       # warm-up: code objects, every buffer of the ring touched
    for i in range(a.ring):
        assert c['run'](i) == 0
torch.cuda.synchronize()
for rep in range(a.reps):
    for c in cfgs:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(a.launches):
            c['run'](k % a.ring)
        e1.record()
        e1.synchronize()
        c['t'].append(e0.elapsed_time(e1) * 1e3 / a.launches)              # us per launch
assert all(bool(torch.isfinite(s[k]).all()) for s in sets for k in s)
say(f'{"kernel":26s} {"B/elem":>6s} {"min us":>9s} {"median":>9s} {"max":>9s}   {"TB/s at max us":>14s} {"median":>8s} {"at min us":>9s}')
for c in cfgs:
    t = np.array(c['t'])
    tb = [c['bytes'] * N / 1e12 / (x * 1e-6) for x in (t.max(), np.median(t), t.min())]
    say(f'{c["name"]:26s} {c["bytes"]:6d} {t.min():9.2f} {np.median(t):9.2f} {t.max():9.2f}   {tb[0]:14.3f} {tb[1]:8.3f} {tb[2]:9.3f}')
s_, ad = cfgs[0], cfgs[1]
rate = lambda c, f: c['bytes'] * N / f(np.array(c['t']))
say(f'Adam / SGD bytes per second: at the medians {rate(ad, np.median) / rate(s_, np.median):.3f}; SGD\'s own spread (max / min us) '
    f'{max(s_["t"]) / min(s_["t"]):.3f}, Adam\'s {max(ad["t"]) / min(ad["t"]):.3f}')
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
