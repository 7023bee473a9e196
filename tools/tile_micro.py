"""Window inference on large images, wall time per image: the per-window path (infer_tile.predict_array /
pixel_predict_array: one upload, one forward at batch 1 and one blocking copy per window, merge on the host) against the
device-resident path (predict_array_batched / pixel_predict_array_batched: csrc/tiles.hip at both ends, ``batch`` windows per
pass, one copy per image), and the two kernels of csrc/tiles.hip alone.

  python tools/tile_micro.py [--reps 5] [--out profiles/tile_micro.txt]

One MI355X, seeded oracle weights, synthetic images (wesup_amd.synth) of 522 x 775 (a GlaS image, 2 x 2 windows), 2320 x 2320
(25 windows, no overlap) and 3000 x 3000 (49 overlapping windows) at patch size 464.  Every configuration runs two warm-up
images first; then ``--reps`` rounds, each round one new image through every configuration in turn (the configurations
alternate, so a drift of the box hits all of them), host clock around work that ends in a device synchronise.  Reported:
median and min .. max per configuration; a size passes when the best batch size is not slower than the per-window path by
more than that path's own spread (max - min) in this run.  The kernels alone: device events, median over 20 launches, GB/s
on the bytes the wrappers count (ops.window_gather / window_merge)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PATCH = 464
SIZES = [(522, 775), (2320, 2320), (3000, 3000)]
SP_BATCHES = (1, 2, 4, 8)
PIXEL_BATCHES = (1, 2, 4)


def _image(seed, H, W):
    from wesup_amd import synth
    return np.ascontiguousarray((synth.synth_image(seed, H, W).transpose(1, 2, 0) * 255).astype(np.uint8))


def _time_configs(configs, images_warm, images_timed, sync):
    """configs: name -> fn(img).  Returns name -> (list of seconds, last result)."""
    for fn in configs.values():
        for img in images_warm:
            fn(img)
    sync()
    times = {k: [] for k in configs}
    last = {}
    for img in images_timed:
        for name, fn in configs.items():
            sync()
            t0 = time.perf_counter()
            out = fn(img)
            sync()
            times[name].append(time.perf_counter() - t0)
            last[name] = out
    return times, last


def _kernel_gbs(fn, nbytes, torch, launches=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    med = statistics.median(ms)
    return med * 1e3, nbytes / (med * 1e-3) / 1e9


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=5, help='timed images per configuration (at least 5)')
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tile_micro.py measures the device path: it needs a GPU')
    reps = max(5, a.reps)
    from oracle import wesup_oracle as orc
    from wesup_amd import infer_tile as T
    from wesup_amd import ops
    from wesup_amd.models import initialize_trainer
    from wesup_amd.models.wesup import WESUPPixelInference
    dev = 'cuda:0'
    sync = torch.cuda.synchronize
    state = {k: torch.from_numpy(v) for k, v in orc.make_weights(3).items()}
    trainer = initialize_trainer('wesup', device=dev)
    trainer.model.load_state_dict(state)
    trainer.model.eval()
    pixel = WESUPPixelInference().to(dev)
    pixel.load_state_dict(state)
    pixel.eval()

    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
    for line in [f'window inference at patch size {PATCH}, wall seconds per image: median (min .. max) over {reps} images, 2 warm-up '
             'images per configuration, configurations alternating image by image',
             f'device: {torch.cuda.get_device_name(0)}; weights: oracle.make_weights(3); images: wesup_amd.synth.synth_image', '']:
        emit(line)
    verdicts = []
    for H, W in SIZES:
        tops, lefts = T.window_grid(H, W, PATCH)
        n = len(tops) * len(lefts)
        warm = [_image(s, H, W) for s in (0, 1)]
        timed = [_image(10 + r, H, W) for r in range(reps)]
        emit(f'{H} x {W}  ({len(tops)} x {len(lefts)} = {n} windows)')
        for kind, batches, old, new in (
                ('superpixel', SP_BATCHES, lambda im: T.predict_array(trainer, im, PATCH, device=dev),
                 lambda im, b: T.predict_array_batched(trainer, im, PATCH, batch=b, device=dev)),
                ('pixel', PIXEL_BATCHES, lambda im: T.pixel_predict_array(pixel, im, PATCH, device=dev),
                 lambda im, b: T.pixel_predict_array_batched(pixel, im, PATCH, batch=b, device=dev))):
            configs = {'per window': old}
            for b in batches:
                configs[f'batch {b}'] = (lambda im, b=b: new(im, b))
            times, last = _time_configs(configs, warm, timed, sync)
            base = times['per window']
            base_med, spread = statistics.median(base), max(base) - min(base)
            emit(f'  {kind:10s} {"configuration":14s} {"median":>9s} {"min":>9s} {"max":>9s} {"per window/this":>16s}   result against per window')
            best = None
            for name, ts in times.items():
                med = statistics.median(ts)
                if name == 'per window':
                    same = ''
                elif kind == 'superpixel':
                    same = f'{int((last[name] != last["per window"]).sum())} of {H * W} pixels differ'
                else:
                    same = f'max |dp| {float(np.abs(last[name] - last["per window"]).max()):.2e}'
                emit(f'  {"":10s} {name:14s} {med:9.4f} {min(ts):9.4f} {max(ts):9.4f} {base_med / med:16.2f}   {same}')
                if name != 'per window' and (best is None or med < best[1]):
                    best = (name, med)
            ok = best[1] <= base_med + spread
            verdicts.append(ok)
            emit(f'  {"":10s} best: {best[0]} at {best[1]:.4f} s against {base_med:.4f} s (spread of the per-window path '
                         f'{spread:.4f} s): {"not slower" if ok else "SLOWER than the per-window path"}')
            for m in (trainer.model, pixel):                  # (the pixel model has no engine before its first forward)
                if m.engine is not None:
                    m.engine.release_buffers()
            torch.cuda.empty_cache()
        emit('')

    # the two kernels alone, at the largest size
    H, W = SIZES[-1]
    tops, lefts = T.window_grid(H, W, PATCH)
    n = len(tops) * len(lefts)
    img_d = torch.from_numpy(_image(3, H, W)).to(dev)
    x = torch.empty(n, 3, PATCH, PATCH, dtype=torch.float32, device=dev)
    emit(f'kernels of csrc/tiles.hip alone, {H} x {W}, {n} windows of {PATCH} (device events, median of 20 launches)')
    us, gbs = _kernel_gbs(lambda: ops.window_gather(img_d, tops, lefts, PATCH, 0, n, out=x), 15.0 * n * PATCH * PATCH, torch)
    emit(f'  window_gather, all {n} windows        {us:9.1f} us {gbs:9.1f} GB/s')
    x4 = x[:4]
    us, gbs = _kernel_gbs(lambda: ops.window_gather(img_d, tops, lefts, PATCH, 8, 4, out=x4), 15.0 * 4 * PATCH * PATCH, torch)
    emit(f'  window_gather, one pass of 4 windows  {us:9.1f} us {gbs:9.1f} GB/s')
    for C in (1, 2):
        pred = torch.rand(n, PATCH, PATCH, C, device=dev)
        out = torch.empty(H, W, C, dtype=torch.float64, device=dev)
        for rf in (False, True):
            us, gbs = _kernel_gbs(lambda: ops.window_merge(pred, tops, lefts, H, W, round_first=rf, out=out),
                                  4.0 * n * PATCH * PATCH * C + 8.0 * H * W * C, torch)
            emit(f'  window_merge, C = {C}, round_first={str(rf):5s}  {us:9.1f} us {gbs:9.1f} GB/s')
    emit('')
    text = '\n'.join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    if not all(verdicts):
        print('at least one size is slower with the device-resident path at its best batch size: see the table')


if __name__ == '__main__':
    main()
