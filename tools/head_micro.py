"""The head kernels alone.  Classifier forward: wesup_classifier_fwd (two classes) beside wesup_classifier_fwd_c at C = 2, 3, 8,
16, D = 32, for the pixel-inference size R = 480*480 and the step's R = 4*576.  The step's two-class head at its own shape (B = 4,
Kmax = 576, D = 32): wesup_head_fwd, wesup_head_bwd + wesup_classifier_bwd_finish, and wesup_classifier_bwd at R = 2304.

  python tools/head_micro.py [--reps N] [--launches N] [--baseline-lib PATH [--baseline-name COMMIT]] [--out profiles/head_micro.txt]

--baseline-lib: another build of the library (the parent commit's, same C ABI), loaded beside the tree's; every two-class entry is
then measured from both, alternating, their results compared bit for bit before anything is timed, and the head-kernel rule printed
per entry: the tree's median is not above the baseline's median by more than the baseline's own max - min of this run.

Per configuration: `launches` back-to-back launches between two device events, `reps` times, the configurations ALTERNATING inside
every repetition (whatever else the box does hits all of them alike); median and min .. max per launch, and for the classifier
forward GB/s on the model R * (D + C) * 4 bytes (every feature read once, every probability written once).  Each launch of a
forward series works on the next of a ring of buffers larger than the 256 MiB Infinity Cache, so the R = 480*480 figure is an HBM
figure; a launch at the step's shape is a few us of work and measures the launch rate."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from wesup_amd import _lib, ops

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=15)
ap.add_argument('--launches', type=int, default=100)
ap.add_argument('--baseline-lib', default='')
ap.add_argument('--baseline-name', default='baseline', help='what the rows of --baseline-lib are called (its commit)')
ap.add_argument('--out', default='')
a = ap.parse_args()

dev = torch.device('cuda:0')
D = 32
RING_BYTES = 640 << 20
lines = []
p = ops._p


def say(s):
    print(s, flush=True)
    lines.append(s)


def bound(path):
    """A second copy of the library with the signatures of _lib._SIGS on the entries timed here."""
    lib = ctypes.CDLL(path)
    assert lib.wesup_abi_version() == _lib.ABI_VERSION, path
    for name in ('wesup_classifier_fwd', 'wesup_classifier_bwd_workspace_bytes', 'wesup_classifier_bwd', 'wesup_head_fwd',
                 'wesup_head_bwd', 'wesup_classifier_bwd_finish'):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._SIGS[name][0], [_lib._T[c] for c in _lib._SIGS[name][1]]
    return lib


libs = [('tree', _lib.load())] + ([(a.baseline_name, bound(a.baseline_lib))] if a.baseline_lib else [])


def measure(cfgs):
    for rep in range(a.reps):
        for c in cfgs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(a.launches):
                c['run'](k)
            e1.record()
            e1.synchronize()
            c['t'].append(e0.elapsed_time(e1) * 1e3 / a.launches)          # us per launch


def rule(cfgs):
    """The head-kernel rule, per two-class entry measured from both libraries."""
    for c in (c for c in cfgs if c['lib'] == 'tree' and c['C'] == 2):
        base = next((b for b in cfgs if b['lib'] != 'tree' and b['name'] == c['name']), None)
        if base is not None:
            t, tb = np.array(c['t']), np.array(base['t'])
            ok = np.median(t) <= np.median(tb) + (tb.max() - tb.min())
            say(f'{c["name"]}: tree / baseline median {np.median(t) / np.median(tb):.3f}; tree {np.median(t):.2f} us, baseline '
                f'{np.median(tb):.2f} us + its max - min {tb.max() - tb.min():.2f} us: {"within" if ok else "SLOWER THAN"} the rule')


say(f'# tools/head_micro.py on {torch.cuda.get_device_name(0)}: {a.launches} launches per measurement, {a.reps} measurements per '
    f'configuration, alternating; D = {D}' + (f'; baseline library: {a.baseline_name}' if a.baseline_lib else ''))
for R, what in ((480 * 480, 'pixel inference, one 480x480 image'), (4 * 576, "the step's superpixel rows, 4 x 576")):
    n_ring = max(2, min(64, -(-RING_BYTES // (R * (D + 16) * 4))))
    rs = np.random.RandomState(R % 1000)
    feats = [torch.from_numpy(np.maximum(rs.randn(R, D), 0).astype(np.float32)).to(dev) for _ in range(n_ring)]
    Wcs = {C: torch.from_numpy((rs.randn(C, D) * 0.2).astype(np.float32)).to(dev) for C in (2, 3, 8, 16)}
    bcs = {C: torch.from_numpy((rs.randn(C) * 0.05).astype(np.float32)).to(dev) for C in (2, 3, 8, 16)}
    cfgs = []
    for tag, lib in libs:
        outs = [torch.empty(R, 2, device=dev) for _ in range(n_ring)]
        run = lambda k, fn=lib.wesup_classifier_fwd, outs=outs: fn(p(feats[k % n_ring]), p(Wcs[2]), p(bcs[2]), p(outs[k % n_ring]), R, D,
                                                                   ops._stream())
        cfgs.append(dict(lib=tag, name='wesup_classifier_fwd', C=2, run=run, outs=outs, t=[]))
    for C in (2, 3, 8, 16):
        outs = [torch.empty(R, C, device=dev) for _ in range(n_ring)]
        run = lambda k, outs=outs, C=C: libs[0][1].wesup_classifier_fwd_c(p(feats[k % n_ring]), p(Wcs[C]), p(bcs[C]), p(outs[k % n_ring]), R,
                                                                          D, C, ops._stream())
        cfgs.append(dict(lib='tree', name='wesup_classifier_fwd_c', C=C, run=run, outs=outs, t=[]))
    for c in cfgs:                                   # warm-up: code objects, every buffer of the ring touched
        for i in range(n_ring):
            assert c['run'](i) == 0
    torch.cuda.synchronize()
    same = all(torch.equal(cfgs[0]['outs'][0], c['outs'][0]) for c in cfgs if c['C'] == 2)
    assert same, 'the two-class results differ between the entries or the libraries'
    measure(cfgs)
    say(f'\nR = {R} ({what}); ring of {n_ring} buffer pairs; every C = 2 row gives the same bits: {same}')
    say(f'{"library":9s} {"entry":26s} {"C":>3s} {"median us":>10s} {"min":>8s} {"max":>8s} {"model MB":>9s} {"GB/s (median)":>14s}')
    for c in cfgs:
        t = np.array(c['t'])
        mb = R * (D + c['C']) * 4 / 1e6
        say(f'{c["lib"]:9s} {c["name"]:26s} {c["C"]:3d} {np.median(t):10.2f} {t.min():8.2f} {t.max():8.2f} {mb:9.2f} '
            f'{mb / 1e3 / (np.median(t) * 1e-6):14.1f}')
    rule(cfgs)
    del feats, cfgs
    torch.cuda.empty_cache()

# the step's two-class head at its own shape
B, Kmax, C = 4, 576, 2
R = B * Kmax
rs = np.random.RandomState(7)
feat = torch.from_numpy(np.maximum(rs.randn(R, D), 0).astype(np.float32) * 0.3).to(dev)
Wc, bc = torch.from_numpy((rs.randn(C, D) * 0.2).astype(np.float32)).to(dev), torch.from_numpy((rs.randn(C) * 0.05).astype(np.float32)).to(dev)
n_sp = torch.tensor([576, 540, 500, 433], dtype=torch.int32, device=dev)
n_l = torch.tensor([170, 160, 150, 130], dtype=torch.int32, device=dev)
labels = torch.from_numpy(np.eye(C, dtype=np.float32)[rs.randint(0, C, (B, Kmax))]).to(dev)
dloss = torch.ones(1, device=dev)
extra = torch.from_numpy(rs.randn(R, D).astype(np.float32)).to(dev)
cfgs = []
for tag, lib in libs:
    o = dict(pred=torch.empty(R, C, device=dev), y_all=torch.empty(B, Kmax, C, device=dev),
             src=torch.empty(B, Kmax, dtype=torch.int32, device=dev), sim=torch.empty(B, Kmax, device=dev),
             terms=torch.empty(B, 8, device=dev), dpred=torch.empty(R, C, device=dev), dfeat=torch.empty(R, D, device=dev),
             dWc=torch.empty(C, D, device=dev), dbc=torch.empty(C, device=dev), dfeat_u=torch.empty(R, D, device=dev),
             dWc_u=torch.empty(C, D, device=dev), dbc_u=torch.empty(C, device=dev))
    nb = lib.wesup_classifier_bwd_workspace_bytes(R, D)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)

    def head_fwd(k, lib=lib, o=o):
        return lib.wesup_head_fwd(p(feat), p(Wc), p(bc), p(o['pred']), p(labels), p(n_sp), p(n_l), 0.8, 1, p(o['y_all']), p(o['src']),
                                  p(o['sim']), B, Kmax, D, C, ops._stream())

    def head_bwd(k, lib=lib, o=o, ws=ws, nb=nb):
        rc = lib.wesup_head_bwd(p(feat), p(Wc), p(o['pred']), p(o['y_all']), p(n_sp), p(n_l), p(dloss), 1e-7, 0.5, p(o['terms']),
                                p(o['dpred']), p(o['dfeat']), B, Kmax, D, C, p(ws), nb, ops._stream())
        return rc or lib.wesup_classifier_bwd_finish(p(ws), nb, p(o['dWc']), p(o['dbc']), R, D, ops._stream())

    def cls_bwd(k, lib=lib, o=o, ws=ws, nb=nb):
        return lib.wesup_classifier_bwd(p(feat), p(Wc), p(o['pred']), p(o['dpred']), p(extra), p(o['dfeat_u']), p(o['dWc_u']),
                                        p(o['dbc_u']), R, D, p(ws), nb, ops._stream())

    for name, run in (('wesup_head_fwd', head_fwd), ('wesup_head_bwd + finish', head_bwd), ('wesup_classifier_bwd', cls_bwd)):
        cfgs.append(dict(lib=tag, name=name, C=C, run=run, outs=o, t=[]))
for c in cfgs:                                       # (in order: head_bwd reads what head_fwd wrote, classifier_bwd what head_bwd wrote)
    for i in range(3):
        assert c['run'](i) == 0
torch.cuda.synchronize()
same = all(torch.equal(cfgs[0]['outs'][k], c['outs'][k]) for c in cfgs for k in c['outs'])
assert same, 'the libraries differ in a result of the two-class head'
measure(cfgs)
say(f"\nthe step's two-class head: B = {B}, Kmax = {Kmax}, D = {D} (R = {R}); both libraries give the same bits: {same}")
say(f'{"library":9s} {"entry":26s} {"median us":>10s} {"min":>8s} {"max":>8s}')
for c in cfgs:
    t = np.array(c['t'])
    say(f'{c["lib"]:9s} {c["name"]:26s} {np.median(t):10.2f} {t.min():8.2f} {t.max():8.2f}')
rule(cfgs)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
