"""Per-image time of weak-label preparation (wesup_amd/prepare.py): the host path (numpy / scipy) against the device path
(csrc/prepare.hip + csrc/regions.hip through ops), stage by stage, on seeded synthetic data: a GlaS-sized gland mask and image
(522 x 775, superpixels of ``ops.slic`` at area 200) and one 1024 x 1024 mask with a few thousand small regions.

  python tools/prepare_micro.py [--out profiles/prepare_micro.txt]

Each stage warm (it has run once before it is timed), host clock around work that ends in a device synchronise, median over the
repetitions.  The ``device`` column of the pipeline stages includes the upload of the mask / label map and the download of the
result, as a caller of ``prepare.py`` pays them; the ``kernels alone`` rows run on resident tensors.  Both paths must give the
same result, or the tool fails.  ``oracle_accuracy`` has two host rows: the reference's own per-superpixel loop
(search_slic_params.py:34-36) and the bincount form that ``prepare.oracle_accuracy`` uses on the host."""
import argparse
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


def _timed(fn, sync, min_time=0.3, max_reps=30):
    """Median seconds per call of ``fn`` (already warm): repeated until ``min_time`` has been spent or ``max_reps`` calls."""
    times, spent = [], 0.0
    while len(times) < max_reps and (spent < min_time or len(times) < min(3, max_reps)):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        times.append(time.perf_counter() - t0)
        spent += times[-1]
    return statistics.median(times), out


def _loop_accuracy(segments, mask):
    """The reference's formulation: one ``segments == id`` pass per superpixel."""
    pred = np.zeros_like(mask)
    for sp_idx in range(segments.max() + 1):
        sp_mask = segments == sp_idx
        if sp_mask.any():
            pred[sp_mask] = mask[sp_mask].mean().round()
    return np.mean(pred == mask)


def _blob_mask(seed, H, W, n):
    rs = np.random.RandomState(seed)
    m = np.zeros((H, W), dtype=np.uint8)
    for _ in range(n):
        h, w = rs.randint(2, 12), rs.randint(2, 12)
        y, x = rs.randint(0, H - h + 1), rs.randint(0, W - w + 1)
        m[y:y + h, x:x + w] = rs.randint(1, 3)
    return m


def _equal(a, b):
    if isinstance(a, (tuple, list)):
        return all(_equal(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('prepare_micro.py measures the device path: it needs a GPU')
    from wesup_amd import ops, synth
    from wesup_amd import prepare as P
    dev = torch.device('cuda:0')
    sync = torch.cuda.synchronize
    nothing = lambda: None
    rows = []

    def stage(case, name, host, device, host_reps=5):
        host()
        device()
        device()
        th, h = _timed(host, nothing, 0.3, host_reps)
        td, d = _timed(device, sync, 0.2, 30)
        if not _equal(h, d):
            raise SystemExit(f'{case} / {name}: host and device results differ')
        rows.append((case, name, th, td))

    # ---- GlaS size
    H, W = 522, 775
    case = f'{H}x{W}'
    mask = synth.gland_map(0, H, W).astype(np.uint8)
    img = (synth.synth_image(0, H, W) * 255).astype(np.uint8).transpose(1, 2, 0)
    x = torch.from_numpy(np.ascontiguousarray(img)).to(dev).permute(2, 0, 1)[None].float().div(255.0).contiguous()
    n_segments = H * W // 200
    seg_d, n_d = ops.slic(x, n_segments, 40.0)
    seg_d, K = seg_d[0].contiguous(), int(n_d[0].item())
    seg = seg_d.cpu().numpy()
    t_slic, _ = _timed(lambda: ops.slic(x, n_segments, 40.0), sync, 0.2, 30)
    for ratio in (1e-4, 1e-3):
        stage(case, f'generate_points, ratio {ratio:g}', lambda: P.generate_points(mask, ratio, np.random.RandomState(1)),
              lambda: P.generate_points(mask, ratio, np.random.RandomState(1), device=dev))
    points = P.generate_points(mask, 1e-3, np.random.RandomState(1))
    stage(case, f'spl_mask, {len(points)} points, K = {K}', lambda: P.spl_mask(seg, points, 2),
          lambda: P.spl_mask(seg, points, 2, device=dev))
    stage(case, 'oracle_accuracy (reference loop)', lambda: _loop_accuracy(seg, mask),
          lambda: P.oracle_accuracy(seg, mask, device=dev), host_reps=1)
    stage(case, 'oracle_accuracy (bincount)', lambda: P.oracle_accuracy(seg, mask), lambda: P.oracle_accuracy(seg, mask, device=dev))
    mask_d = torch.from_numpy(mask).to(dev)
    pts_d = torch.from_numpy(points.astype(np.int32)).to(dev)
    seg64 = seg.astype(np.int64).ravel()
    rr, cc = (v.ravel().astype(np.float64) for v in np.meshgrid(np.arange(H), np.arange(W), indexing='ij'))
    stage(case, 'kernels alone: label_stats',
          lambda: np.stack([np.bincount(seg64, minlength=K), np.bincount(seg64, weights=rr, minlength=K),
                            np.bincount(seg64, weights=cc, minlength=K)], axis=1).astype(np.int64),
          lambda: ops.label_stats(seg_d, K - 1)[0].cpu().numpy())
    stage(case, 'kernels alone: sp_vote', lambda: int(round(P.oracle_accuracy(seg, mask) * H * W)),
          lambda: int(ops.sp_vote(seg_d, mask_d, K, paint=False)[1].item()))
    stage(case, 'kernels alone: spl_paint', lambda: P.spl_mask(seg, points, 2),
          lambda: ops.spl_paint(seg_d, pts_d, K, 2)[0].cpu().numpy())

    # ---- many regions
    H2 = W2 = 1024
    case2 = f'{H2}x{W2}'
    blobs = _blob_mask(3, H2, W2, 4000)
    from scipy import ndimage
    n_regions = sum(ndimage.label(blobs == c, structure=np.ones((3, 3), dtype=np.int32))[1] for c in (1, 2))
    for ratio in (1e-4, 0.05):
        stage(case2, f'generate_points, ratio {ratio:g}', lambda: P.generate_points(blobs, ratio, np.random.RandomState(1)),
              lambda: P.generate_points(blobs, ratio, np.random.RandomState(1), device=dev), host_reps=1)

    lines = ['weak-label preparation, seconds per image (median)',
             f'host: {_cpu_model()}, {len(os.sched_getaffinity(0))} CPUs available to the process, OMP_NUM_THREADS='
             f'{os.environ.get("OMP_NUM_THREADS", "unset")}',
             f'device: {torch.cuda.get_device_name(0)}',
             f'{case}: gland mask of synth.gland_map(0), {K} superpixels of ops.slic (area 200, compactness 40: '
             f'{t_slic * 1e3:.3f} ms per call); {case2}: {n_regions} regions of two classes',
             'the results of the two paths are equal in every row', '',
             f'{"case":10s} {"stage":44s} {"host [s]":>12s} {"device [s]":>12s} {"host/device":>12s}']
    for case_, name, th, td in rows:
        lines.append(f'{case_:10s} {name:44s} {th:12.6f} {td:12.6f} {th / td:12.1f}')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
