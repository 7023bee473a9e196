"""Time of one painted comparison (wesup_amd/paint.py) at the size of a CRAG image: the host path (numpy / scipy) against the
device path (csrc/regions.hip + csrc/paint.hip through ops), whole and stage by stage, on one seeded pair of 1512 x 1516 maps
with about 60 ellipses on each side.

  python tools/paint_micro.py [--out profiles/paint_micro.txt]

Each stage warm (it has run before it is timed), host clock around work that ends in a device synchronise, median and min .. max
over the repetitions.  The whole-call rows are ``paint_pred_and_gt`` as a caller pays it, uploads and the copy back included; the
device stages run on resident tensors, except the rows that say they copy.  The paint kernel also gets its rate over the bytes it
must move (4 per pixel read, 3 written).  Both paths must give the same two arrays, or the tool fails.

The reference's own function is not timed here (it needs the reference checkout): ``tools/make_paint_golden.py`` times it on the
96 x 120 cases and stores the seconds in ``tests/golden/paint.npz``; the header below quotes them with the operation count
nP * nG * H * W of its loop, at both sizes, as counts and not as a time."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W, N = 1512, 1516, 60


def _cpu_model():
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                return line.split(':', 1)[1].strip()
    except OSError:
        pass
    return 'unknown'


def _timed(fn, sync, min_time=0.3, max_reps=30):
    """(median, min, max) seconds per call of ``fn`` (already warm) and its last result."""
    times, spent = [], 0.0
    while len(times) < max_reps and (spent < min_time or len(times) < min(3, max_reps)):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        times.append(time.perf_counter() - t0)
        spent += times[-1]
    return (statistics.median(times), min(times), max(times)), out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('paint_micro.py measures the device path: it needs a GPU')
    from wesup_amd import ops, paint, synth
    from wesup_amd.utils import metrics as M
    dev = torch.device('cuda:0')
    sync = torch.cuda.synchronize
    nothing = lambda: None
    G = synth.gland_map(11, H, W, N, 30, 80)
    S = np.roll(G, 9, axis=(0, 1)) | synth.gland_map(12, H, W, N // 4, 20, 60)
    rows = []

    def row(name, fn, sync_fn, reps):
        fn()
        (med, lo, hi), out = _timed(fn, sync_fn, 0.3, reps)
        rows.append((name, med, lo, hi))
        return out

    # ---- whole calls
    want = row('host: paint_pred_and_gt', lambda: paint.paint_pred_and_gt(S, G), nothing, 5)
    paint.paint_pred_and_gt(S, G, device=dev)
    got = row('device: paint_pred_and_gt(device=)', lambda: paint.paint_pred_and_gt(S, G, device=dev), sync, 200)
    if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
        raise SystemExit('host and device paintings differ')

    # ---- host stages
    P, T = row('host: label both maps', lambda: (M.label(S), M.label(G)), nothing, 5)
    nP, nG = int(P.max()), int(T.max())
    C = row('host: contingency table', lambda: M._contingency(P, T)[0], nothing, 5)
    match = row('host: match_objects_from_table', lambda: paint.match_objects_from_table(C), nothing, 10)
    row('host: relabel + paint both maps', lambda: (paint.paint(match[P], paint.reference_rng()), paint.paint(T)), nothing, 5)

    # ---- device stages
    both_h = np.stack([S != 0, G != 0])
    both = row('device: upload both maps (bool -> uint8)', lambda: torch.from_numpy(both_h).to(dev).to(torch.uint8), sync, 200)
    labels, n = row('device: cc_label, batch of 2', lambda: ops.cc_label(both, 8, 1), sync, 200)
    row('device: copy the two counts back', lambda: n.cpu(), sync, 200)
    assert [int(v) for v in n.cpu()] == [nP, nG]
    table, _ = row('device: contingency', lambda: ops.contingency(labels[0], labels[1], nP, nG), sync, 200)
    n_s, n_g = n[0:1].contiguous(), n[1:2].contiguous()
    m_d = row('device: object_match', lambda: ops.object_match(table, n_s, n_g), sync, 200)
    row('device: copy the match vector back', lambda: m_d.cpu(), sync, 200)
    if not np.array_equal(m_d.cpu().numpy(), match):
        raise SystemExit('host and device matches differ')
    n_lut = max(nP, nG) + 1
    luts = torch.from_numpy(np.random.RandomState(0).randint(0, 1 << 24, (2, n_lut)).astype(np.int32)).to(dev)
    out, _ = row('device: label_paint, batch of 2', lambda: ops.label_paint(labels, luts), sync, 200)
    t_paint = rows[-1][1]
    row('device: copy both paintings back', lambda: out.cpu(), sync, 200)

    gold = os.path.join(ROOT, 'tests', 'golden', 'paint.npz')
    ref = ''
    if os.path.exists(gold):
        g = np.load(gold)
        h, w = (int(v) for v in g['shape'])
        sp, sg = (np.unpackbits(g[f'{k}_many'])[:h * w].reshape(h, w) for k in 'SG')
        p_, g_ = int(M.label(sp).max()), int(M.label(sg).max())
        ref = (f"the reference's own paint_pred_and_gt, timed by tools/make_paint_golden.py on the development machine (not on this "
               f"host) on the {h} x {w} case 'many' ({p_} x {g_} objects): {float(g['seconds_many']):.3f} s.  Its loop builds one "
               f'boolean mask per pair of objects: nP * nG * H * W = {p_ * g_ * h * w:.3g} pixel operations there, '
               f'{nP * nG * H * W:.3g} for this pair ({nP} x {nG} objects, {H} x {W}), {nP * nG * H * W / (p_ * g_ * h * w):.0f} '
               f'times as many -- a count, not a measured time')
    moved = 2 * H * W * 7
    lines = ['painted comparison of one prediction / ground-truth pair, seconds per call: median (min .. max)',
             f'host: {_cpu_model()}, {len(os.sched_getaffinity(0))} CPUs available to the process, OMP_NUM_THREADS='
             f'{os.environ.get("OMP_NUM_THREADS", "unset")}',
             f'device: {torch.cuda.get_device_name(0)}',
             f'{H} x {W}, {nP} predicted and {nG} ground-truth objects (synth.gland_map: {N} ellipses, the prediction a shifted copy '
             f'plus {N // 4} strangers); both paths give the same two arrays',
             f'label_paint alone: {moved / 1e6:.1f} MB of labels read and RGB written in {t_paint * 1e6:.1f} us = '
             f'{moved / t_paint / 1e9:.0f} GB/s'] + ([ref] if ref else []) + ['', f'{"stage":46s} {"median [s]":>12s} {"min [s]":>12s} {"max [s]":>12s}']
    for name, med, lo, hi in rows:
        lines.append(f'{name:46s} {med:12.6f} {lo:12.6f} {hi:12.6f}')
    lines.append(f'{"host / device, whole call":46s} {rows[0][1] / rows[1][1]:12.1f}')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
