"""Per-image time of mask post-processing + GlaS challenge scoring: the host path (numpy / scipy, the default of
evaluate.py / infer.py) against the device path (csrc/regions.hip through ops and utils/metrics_gpu.py), on the same seeded
synthetic gland maps (wesup_amd.synth.gland_pair): GlaS size 522 x 775 and one 2048 x 2048 case.

  python tools/score_micro.py [--pairs 6] [--out profiles/score_micro.txt]

Each stage and the whole, warm (every shape has run once before it is timed), host clock around work that ends in a device
synchronise, median over the repetitions.  Both paths must give the same masks and the same scores, or the tool fails."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _cpu_model():
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                return line.split(':', 1)[1].strip()
    except OSError:
        pass
    return 'unknown'


def _timed(fn, sync, min_time, max_reps):
    """Median seconds per call of ``fn`` (already warm): repeated until ``min_time`` has been spent or ``max_reps`` calls."""
    times, spent = [], 0.0
    while len(times) < max_reps and (spent < min_time or len(times) < 3):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        times.append(time.perf_counter() - t0)
        spent += times[-1]
    return statistics.median(times), out


def _same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--pairs', type=int, default=6, help='seeded 522 x 775 pairs')
    ap.add_argument('--min-size', type=int, default=2000)
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    import torch
    from scipy import ndimage
    if not torch.cuda.is_available():
        raise SystemExit('score_micro.py measures the device path: it needs a GPU')
    from wesup_amd import ops, synth
    from wesup_amd.evaluate import remove_small_regions
    from wesup_amd.infer import _cross
    from wesup_amd.utils import metrics as M
    from wesup_amd.utils import metrics_gpu as MG
    dev = torch.device('cuda:0')
    sync = torch.cuda.synchronize
    nothing = lambda: None
    cross = _cross(9)
    cases = [('522x775', synth.gland_pair(s)) for s in range(a.pairs)]
    cases.append(('2048x2048', synth.gland_pair(100, 2048, 2048, n=40, shift=9, square=120)))

    stages = ['opening', 'remove_small_regions', 'f1 + object dice', 'object hausdorff', 'whole']
    acc = {}
    for size, (S, G) in cases:
        rs = np.random.RandomState(1)
        raw = S.copy()
        raw[rs.rand(*S.shape) < 0.001] ^= 1                # what a network leaves behind: specks and pin holes
        big = size != '522x775'
        reps = (1, 1) if big else (3, 20)                  # (host, device) upper bounds; the device side is cheap to repeat
        x = raw.astype(np.float64)

        # ---- host path: the functions evaluate.py / infer.py use by default
        def h_open():
            return ndimage.grey_opening(x, footprint=cross)

        def h_whole():
            p = remove_small_regions(ndimage.grey_opening(x, footprint=cross), a.min_size)
            return p, (M.detection_f1(p, G), M.object_dice(p, G), M.object_hausdorff(p, G) if p.any() and G.any() else float('nan'))
        t = {}
        h_open()
        t['opening'], opened = _timed(h_open, nothing, 0.3, reps[0] * 3)
        t['remove_small_regions'], clean = _timed(lambda: remove_small_regions(opened, a.min_size), nothing, 0.3, reps[0] * 3)
        t['f1 + object dice'], _ = _timed(lambda: (M.detection_f1(clean, G), M.object_dice(clean, G)), nothing, 0.3, reps[0] * 3)
        t['object hausdorff'], _ = _timed(lambda: M.object_hausdorff(clean, G), nothing, 0.3, reps[0])
        t['whole'], (h_mask, h_scores) = _timed(h_whole, nothing, 0.3, reps[0])

        # ---- device path: the prediction is on the GPU (infer.predict(device_post=True)), the ground truth is uploaded
        d_raw = torch.from_numpy(raw).to(dev)
        Gt = torch.from_numpy(G)

        def d_open():
            return ops.binary_opening(d_raw, cross)

        def d_f1_dice(p, g):
            lab = MG._Labelled(p, g)
            return M.detection_f1_from_table(lab.C), M.object_dice_from_table(lab.C)

        def d_whole():
            p = ops.remove_small_regions(ops.binary_opening(d_raw, cross), a.min_size)
            sc = MG.challenge_scores(p, Gt.to(dev))
            return p, (sc['detection_f1'], sc['object_dice'], sc['object_hausdorff'])
        u = {}
        d_whole()                                          # warm: code objects, workspaces, every shape
        d_whole()
        u['opening'], d_opened = _timed(d_open, sync, 0.2, reps[1] * 5)
        u['remove_small_regions'], d_clean = _timed(lambda: ops.remove_small_regions(d_opened, a.min_size), sync, 0.2, reps[1] * 5)
        d_G = Gt.to(dev)
        d_f1_dice(d_clean, d_G)
        u['f1 + object dice'], _ = _timed(lambda: d_f1_dice(d_clean, d_G), sync, 0.2, reps[1] * 5)
        u['object hausdorff'], _ = _timed(lambda: MG.object_hausdorff(d_clean, d_G), sync, 0.2, reps[1] * 5)
        u['whole'], (d_mask, d_scores) = _timed(d_whole, sync, 0.3, reps[1] * 5)

        if not np.array_equal(d_mask.cpu().numpy(), h_mask.astype(np.uint8)):
            raise SystemExit(f'{size}: the post-processed masks differ')
        if not all(_same(float(p), float(q)) for p, q in zip(h_scores, d_scores)):
            raise SystemExit(f'{size}: the scores differ: host {h_scores}, device {d_scores}')
        for k in stages:
            acc.setdefault(size, {}).setdefault(k, []).append((t[k], u[k]))

    lines = ['mask post-processing + GlaS challenge scoring, seconds per image (median per image, mean over the images)',
             f'host: {_cpu_model()}, {len(os.sched_getaffinity(0))} CPUs available to the process, torch threads '
             f'{torch.get_num_threads()}, OMP_NUM_THREADS={os.environ.get("OMP_NUM_THREADS", "unset")}',
             f'device: {torch.cuda.get_device_name(0)}',
             'masks and scores of the two paths are equal on every image', '']
    for size, per in acc.items():
        n = len(per['whole'])
        lines.append(f'{size}  ({n} image{"s" if n > 1 else ""})')
        lines.append(f'  {"stage":24s} {"host [s]":>12s} {"device [s]":>12s} {"host/device":>12s}')
        for k in stages:
            h = sum(v[0] for v in per[k]) / n
            d = sum(v[1] for v in per[k]) / n
            lines.append(f'  {k:24s} {h:12.5f} {d:12.5f} {h / d:12.1f}')
        lines.append('')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
