"""Whole-slide evaluation, wall time per slide: the device-resident path (slide.slide_predict / slide_pixel_predict: one
upload, csrc/slide.hip at both ends of every pass, one copy back) against the same work done patch by patch with what the
project had before -- pad on the host, upload a patch, ``F.interpolate``, ``infer.predict_single_image`` resp.
``pixel_infer.pixel_predict``, a blocking copy per patch, paste on the host -- and the three kernels of csrc/slide.hip alone.

  python tools/slide_micro.py [--reps 5] [--out profiles/slide_micro.txt]

One MI355X, seeded oracle weights, a synthetic slide (wesup_amd.synth) of 3000 x 2600 at patch size 1000 (3 x 3 patches, the
last row and column padded) -> 400 x 400 (the reference's input size; scale 0.4 for the pixel path).  Every configuration runs
one warm-up slide first; then ``--reps`` rounds, each round one new slide through every configuration in turn (the
configurations alternate, so a drift of the machine hits all of them), host clock around work that ends in a device
synchronise.  Reported: median and min .. max per configuration, and whether the best resident configuration is faster beyond
the spread (its slowest slide against the per-patch path's fastest).  The kernels alone: device events, median over 20 launches,
GB/s of their compulsory bytes (the slide's bytes in and the network's floats out for the gather, the predictions in and the
map out for the scatter, both maps for the scores)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W, PATCH, SIZE, SCALE = 3000, 2600, 1000, (400, 400), 0.4


def _image(seed, h, w):
    from wesup_amd import synth
    return np.ascontiguousarray((synth.synth_image(seed, h, w).transpose(1, 2, 0) * 255).astype(np.uint8))


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
    ap.add_argument('--reps', type=int, default=5, help='timed slides per configuration (at least 5)')
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit('slide_micro.py measures the device path: it needs a GPU')
    reps = max(5, a.reps)
    from oracle import wesup_oracle as orc
    from wesup_amd import infer as I
    from wesup_amd import ops
    from wesup_amd import pixel_infer as PI
    from wesup_amd import slide as S
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
    zero_mask = torch.zeros(1, 2, *SIZE, device=dev)

    def per_patch_superpixel(img):
        maps = []
        for patch in S.split_patches_array(img, PATCH):                      # host pad
            x = torch.from_numpy(patch).to(dev).permute(2, 0, 1).float().div_(255.).unsqueeze(0)
            x = F.interpolate(x, size=SIZE, mode='bilinear')
            pred = I.predict_single_image(trainer, x, zero_mask, (PATCH, PATCH))
            maps.append((pred[0, 0].cpu().numpy() * 255).astype(np.uint8))
        return S.combine_single_array(np.stack(maps), img.shape[:2]).astype(np.uint8)

    def per_patch_pixel(img):
        maps = [PI.pixel_predict(pixel, patch, (SCALE,), device=dev).round() * 255 for patch in S.split_patches_array(img, PATCH)]
        return S.combine_single_array(np.stack(maps), img.shape[:2]).astype(np.uint8)

    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
    n_h, n_w = S.patch_grid(H, W, PATCH)
    n = n_h * n_w
    for line in [f'whole-slide evaluation, {H} x {W} at patch size {PATCH} ({n_h} x {n_w} = {n} patches) -> {SIZE[0]} x {SIZE[1]}, wall '
                 f'seconds per slide: median (min .. max) over {reps} slides, 1 warm-up slide per configuration, configurations '
                 'alternating slide by slide',
                 f'device: {torch.cuda.get_device_name(0)}; weights: oracle.make_weights(3); slides: wesup_amd.synth.synth_image', '']:
        emit(line)
    warm = [_image(0, H, W)]
    timed = [_image(10 + r, H, W) for r in range(reps)]
    for kind, old, new, batches in (
            ('superpixel', per_patch_superpixel, lambda im, b: S.slide_predict(trainer, im, PATCH, SIZE, batch=b, device=dev), (1, 3, 9)),
            ('pixel', per_patch_pixel, lambda im, b: S.slide_pixel_predict(pixel, im, PATCH, SCALE, batch=b, device=dev), (1, 3))):
        configs = {'per patch': old}
        for b in batches:
            configs[f'resident, batch {b}'] = (lambda im, b=b: new(im, b))
        for fn in configs.values():
            for img in warm:
                fn(img)
        sync()
        times, last = {k: [] for k in configs}, {}
        for img in timed:
            for name, fn in configs.items():
                sync()
                t0 = time.perf_counter()
                out = fn(img)
                sync()
                times[name].append(time.perf_counter() - t0)
                last[name] = out
        base = times['per patch']
        base_med, spread = statistics.median(base), max(base) - min(base)
        emit(f'  {kind:10s} {"configuration":20s} {"median":>9s} {"min":>9s} {"max":>9s} {"per patch/this":>15s}   map against per patch')
        best = None
        for name, ts in times.items():
            med = statistics.median(ts)
            same = '' if name == 'per patch' else f'{int((last[name] != last["per patch"]).sum())} of {H * W} pixels differ'
            emit(f'  {"":10s} {name:20s} {med:9.4f} {min(ts):9.4f} {max(ts):9.4f} {base_med / med:15.2f}   {same}')
            if name != 'per patch' and (best is None or med < best[1]):
                best = (name, med)
        if max(times[best[0]]) < min(base):
            verdict = 'faster beyond the spread (its slowest slide is faster than the per-patch path\'s fastest)'
        elif best[1] <= base_med + spread:
            verdict = 'not slower, but the two ranges overlap'
        else:
            verdict = 'SLOWER than the per-patch path'
        emit(f'  {"":10s} best: {best[0]} at {best[1]:.4f} s against {base_med:.4f} s (spread of the per-patch path {spread:.4f} s): '
             f'{verdict}')
        for m in (trainer.model, pixel):
            if m.engine is not None:
                m.engine.release_buffers()
        torch.cuda.empty_cache()
        emit('')

    img_d = torch.from_numpy(_image(3, H, W)).to(dev)
    h, w = SIZE
    x = torch.empty(n, 3, h, w, dtype=torch.float32, device=dev)
    emit(f'kernels of csrc/slide.hip alone, {H} x {W}, {n} patches of {PATCH} -> {h} x {w} (device events, median of 20 launches, '
         'GB/s of compulsory bytes)')
    for ac in (False, True):
        us, gbs = _kernel_gbs(lambda: ops.patch_gather_resize(img_d, PATCH, h, w, 0, n, align_corners=ac, out=x),
                              3.0 * H * W + 12.0 * n * h * w, torch)
        emit(f'  patch_gather_resize, all {n} patches, align_corners={str(ac):5s}  {us:9.1f} us {gbs:9.1f} GB/s')
    us, gbs = _kernel_gbs(lambda: ops.patch_gather_resize(img_d, PATCH, h, w, 0, 3, out=x[:3]), 3.0 * PATCH * W + 12.0 * 3 * h * w, torch)
    emit(f'  patch_gather_resize, one pass of 3 patches               {us:9.1f} us {gbs:9.1f} GB/s')
    out = torch.empty(H, W, dtype=torch.uint8, device=dev)
    pred1, pred2 = torch.rand(n, h, w, device=dev), torch.rand(n, h, w, 2, device=dev)
    for mode, src, label in ((0, pred1, 'nearest, stride 1'), (1, pred2[..., 1], 'bilinear, stride 2')):
        us, gbs = _kernel_gbs(lambda: ops.patch_scatter_u8(src, out, PATCH, 0, mode=mode), 4.0 * n * h * w + 1.0 * H * W, torch)
        emit(f'  patch_scatter_u8, all {n} patches, {label:18s}        {us:9.1f} us {gbs:9.1f} GB/s')
    gt = (torch.rand(H, W, device=dev) < 0.5).to(torch.uint8) * 255
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    us, gbs = _kernel_gbs(lambda: ops.mask_scores(out, gt, False, out=counts), 2.0 * H * W, torch)
    emit(f'  mask_scores, {H * W} pixels (fill + count)                 {us:9.1f} us {gbs:9.1f} GB/s')
    emit('')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
