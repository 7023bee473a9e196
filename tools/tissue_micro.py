"""Whole-slide evaluation with and without ``skip_background``, wall time per slide, and the selection chain of
csrc/tissue.hip alone.

  python tools/tissue_micro.py [--reps 5] [--out profiles/tissue_micro.txt]

One MI355X, seeded oracle weights, the synthetic slide of tools/slide_micro.py: 3000 x 2600 at patch size 1000 (3 x 3 patches,
the last row and column padded) -> 400 x 400 (scale 0.4 for the pixel path), at the driver's default batch sizes (4 and 2).
Tissue is left in 9, 5 and 2 of the 9 patches; the others are painted 255 (glass).  Per model and slide kind two configurations,
without the selection (the path as it was: the baseline) and with ``skip_background=True``; every configuration runs one warm-up
slide, then ``--reps`` rounds, each round one new slide through both configurations in turn (they alternate, so a drift of the
machine hits both), host clock around work that ends in a device synchronise.  Reported: median (min .. max), and the rule of
DESIGN.md 3.9: a gain is claimed only where the slowest slide with skipping beats the fastest without.  With 9 of 9 kept the same
rule states the overhead.

The selection chain alone (``ops.patch_value_hist`` + ``ops.tissue_select``, no read-back): device events, median of 20, in us
and GB/s of the slide's 3 H W bytes, on a noise slide and on an all-255 slide (every lane of a wave on one bin), beside the
histogram kernel alone and the mask."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W, PATCH, SIZE, SCALE = 3000, 2600, 1000, (400, 400), 0.4
TISSUE_IN = {9: range(9), 5: (0, 2, 4, 6, 8), 2: (4, 8)}        # the patches that keep their tissue


def _image(seed, h, w):
    from wesup_amd import synth
    return np.ascontiguousarray((synth.synth_image(seed, h, w).transpose(1, 2, 0) * 255).astype(np.uint8))


def _slide(seed, kept):
    img = _image(seed, H, W)
    n_w = -(-W // PATCH)
    for k in range(9):
        if k not in TISSUE_IN[kept]:
            y, x = k // n_w * PATCH, k % n_w * PATCH
            img[y:y + PATCH, x:x + PATCH] = 255
    return img


def _events_us(fn, torch, launches=20):
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
    return statistics.median(ms) * 1e3, min(ms) * 1e3, max(ms) * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=5, help='timed slides per configuration (at least 5)')
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tissue_micro.py measures the device path: it needs a GPU')
    reps = max(5, a.reps)
    from oracle import wesup_oracle as orc
    from wesup_amd import ops
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
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
    for line in [f'whole-slide evaluation with and without skip_background, {H} x {W} at patch size {PATCH} (3 x 3 = 9 patches) -> '
                 f'{SIZE[0]} x {SIZE[1]}, wall seconds per slide: median (min .. max) over {reps} slides, 1 warm-up slide per '
                 'configuration, the two configurations alternating slide by slide',
                 f'device: {torch.cuda.get_device_name(0)}; weights: oracle.make_weights(3); slides: wesup_amd.synth.synth_image, '
                 'the patches without tissue painted 255', '']:
        emit(line)
    models = (('superpixel', 4, lambda im, b, **kw: S.slide_predict(trainer, im, PATCH, SIZE, batch=b, device=dev, **kw)),
              ('pixel', 2, lambda im, b, **kw: S.slide_pixel_predict(pixel, im, PATCH, SCALE, batch=b, device=dev, **kw)))
    for kind, batch, predict in models:
        emit(f'  {kind}, batch {batch}')
        emit(f'  {"tissue in":>10s} {"kept":>5s} {"t":>4s}   {"without: median (min .. max)":>32s}   {"with: median (min .. max)":>32s}   '
             f'{"without/with":>12s}   kept patches equal   verdict')
        for kept in (9, 5, 2):
            warm, timed = _slide(kept, kept), [_slide(10 * kept + r, kept) for r in range(reps)]
            configs = {'without': lambda im: predict(im, batch), 'with': lambda im: predict(im, batch, skip_background=True)}
            for fn in configs.values():
                fn(warm)
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
            sel = S.tissue_patches(timed[-1], PATCH, device=dev)
            mask = np.zeros((H, W), bool)
            for k in sel.list.cpu().tolist():
                y, x = k // 3 * PATCH, k % 3 * PATCH
                mask[y:y + PATCH, x:x + PATCH] = True
            differ = int((last['with'][mask] != last['without'][mask]).sum())
            off, on = times['without'], times['with']
            if max(on) < min(off):
                verdict = 'faster beyond the spread'
            elif min(on) > max(off):
                verdict = 'SLOWER beyond the spread'
            else:
                verdict = 'the two ranges overlap: no difference claimed'
            fmt = lambda ts: f'{statistics.median(ts):9.4f} ({min(ts):7.4f} .. {max(ts):7.4f})'
            emit(f'  {kept:>7d}/9 {sel.n_keep:>5d} {sel.t:>4d}   {fmt(off):>32s}   {fmt(on):>32s}   '
                 f'{statistics.median(off) / statistics.median(on):12.2f}   {differ:>8d} differ    {verdict}')
        for m in (trainer.model, pixel):
            if m.engine is not None:
                m.engine.release_buffers()
        torch.cuda.empty_cache()
        emit('')

    emit(f'the selection alone, {H} x {W} at patch size {PATCH} (device events, median (min .. max) of 20, GB/s of the slide\'s '
         f'{3 * H * W} bytes at the median)')
    nbytes = 3.0 * H * W
    slides = (('noise', torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev)),
              ('synthetic slide, tissue in 5/9', torch.from_numpy(_slide(3, 5)).to(dev)),
              ('all 255', torch.full((H, W, 3), 255, dtype=torch.uint8, device=dev)))
    for channel in ('luma', 'chroma'):
        for name, img_d in slides:
            hist = ops.patch_value_hist(img_d, PATCH, channel)
            info = ops.tissue_select(hist, H, W, PATCH, channel)[0]
            out = torch.empty(H, W, dtype=torch.uint8, device=dev)
            for label, fn in (('patch_value_hist (fill + histogram)', lambda: ops.patch_value_hist(img_d, PATCH, channel, out=hist)),
                              ('tissue_select (5 launches)', lambda: ops.tissue_select(hist, H, W, PATCH, channel)),
                              ('the chain: both', lambda: ops.tissue_select(ops.patch_value_hist(img_d, PATCH, channel, out=hist),
                                                                            H, W, PATCH, channel)),
                              ('tissue_mask', lambda: ops.tissue_mask(img_d, info, channel, out=out))):
                med, lo, hi = _events_us(fn, torch)
                rate = f'{nbytes / (med * 1e-6) / 1e9:9.1f} GB/s' if 'select (' not in label else ' ' * 14
                emit(f'  {channel:6s} {name:32s} {label:38s} {med:9.1f} us ({lo:8.1f} .. {hi:8.1f}) {rate}')
    emit('')
    emit('beside them (profiles/slide_micro.txt, the same slide size): patch_gather_resize of all 9 patches 22.8 us = 1784 GB/s, '
         'mask_scores 33.0 us = 473 GB/s')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
