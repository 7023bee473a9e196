"""Whole-image pixel inference, one forward per image: the shipped ``WESUPPixelInference.forward`` (the 2112-channel map, the
first fc layer on every pixel) against ``forward_per_resolution`` (that layer at each resolution), and the
gather kernel of csrc/pixel.hip alone.

  python tools/pixel_micro.py [--reps 9] [--out profiles/pixel_micro.txt]

One MI355X, seeded oracle weights, synthetic images (wesup_amd.synth) at 400 x 400 (the DP2019 operating point: 1000 x 1000
patches at scale 0.4) and 387 x 261 (a GlaS image at 0.5).  Both paths run three warm-up forwards per size; then ``--reps``
rounds, each round one new image through both paths in turn (they alternate, so a drift of the box hits both), host clock
around a forward that ends in a device synchronise.  Reported: median and min .. max per path, the largest difference of the two
results, and whether the per-resolution path is faster by more than the spread (max - min) of either path in this run.  The
gather alone: device events, median over 20 launches, GB/s on its compulsory bytes (P0 read, h1 written, each coarse map
read once)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(400, 400), (387, 261)]


def gather_bytes(B, H, W, N, coarse):
    """Compulsory bytes of ops.pixel_gather_fwd: P0 read, h1 written, each coarse map once."""
    return 4.0 * B * N * (2 * H * W + sum(h * w for h, w in coarse))


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
    ap.add_argument('--reps', type=int, default=9, help='timed images per path (at least 5)')
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('pixel_micro.py measures the device path: it needs a GPU')
    reps = max(5, a.reps)
    from oracle import wesup_oracle as orc
    from wesup_amd import ops, synth
    from wesup_amd.layer_plan import layer_dims
    from wesup_amd.models.wesup import WESUPPixelInference
    dev = 'cuda:0'
    sync = torch.cuda.synchronize
    model = WESUPPixelInference().to(dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in orc.make_weights(4, feat_scale=0.3).items()})
    model.eval()
    paths = {'forward (full maps)': lambda x: model(x), 'forward_per_resolution': lambda x: model.forward_per_resolution(x)[0]}

    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
    emit(f'pixel inference, one forward at batch 1, wall milliseconds: median (min .. max) over {reps} images, 3 warm-up forwards '
         'per path, the two paths alternating image by image')
    emit(f'device: {torch.cuda.get_device_name(0)}; weights: oracle.make_weights(4, feat_scale=0.3); images: wesup_amd.synth.synth_image')
    emit('')
    faster = []
    for H, W in SIZES:
        imgs = [torch.from_numpy(synth.synth_image(s, H, W))[None].to(dev) for s in range(reps + 1)]
        for fn in paths.values():
            for _ in range(3):
                fn(imgs[0])
        sync()
        times = {k: [] for k in paths}
        worst = 0.0
        for x in imgs[1:]:
            outs = {}
            for name, fn in paths.items():
                sync()
                t0 = time.perf_counter()
                out = fn(x)
                sync()
                times[name].append((time.perf_counter() - t0) * 1e3)
                outs[name] = out.clone()
            full, per = outs.values()
            worst = max(worst, float((full - per).abs().max()))
        emit(f'{H} x {W}')
        emit(f'  {"path":24s} {"median":>9s} {"min":>9s} {"max":>9s}')
        for name, ts in times.items():
            emit(f'  {name:24s} {statistics.median(ts):9.3f} {min(ts):9.3f} {max(ts):9.3f}')
        full, per = times.values()
        spread = max(max(full) - min(full), max(per) - min(per))
        gain = statistics.median(full) - statistics.median(per)
        faster.append(gain > spread)
        emit(f'  full maps / per resolution = {statistics.median(full) / statistics.median(per):.2f}; difference of the medians '
             f'{gain:.3f} ms against a spread of {spread:.3f} ms: per resolution is '
             f'{"faster" if gain > spread else "NOT faster beyond the spread"};  max |dp| between the paths {worst:.2e}')
        # the gather alone, on buffers of its own at this size
        N = model.engine.p['fc_layers.0.weight'].shape[0]
        coarse = sorted(set(layer_dims(H, W)), reverse=True)[1:]
        p0 = torch.randn(1, H, W, N, device=dev)
        out = torch.empty_like(p0)
        maps = [torch.randn(1, h, w, N, device=dev) for h, w in coarse]
        bias = model.engine.p['fc_layers.0.bias']
        nbytes = gather_bytes(1, H, W, N, coarse)
        us, gbs = _kernel_gbs(lambda: ops.pixel_gather_fwd(p0, bias, maps, out=out), nbytes, torch)
        emit(f'  pixel_gather_fwd alone, N = {N}, coarse maps {coarse}: out of place {us:9.1f} us {gbs:8.1f} GB/s '
             f'({nbytes / 1e6:.0f} MB compulsory)')
        us, gbs = _kernel_gbs(lambda: ops.pixel_gather_fwd(p0, bias, maps), nbytes, torch)
        emit(f'  {"":71s} in place     {us:9.1f} us {gbs:8.1f} GB/s')
        emit('')
        del p0, out, maps, imgs
        model.engine.release_buffers()
        model._pixel_sets = None
        torch.cuda.empty_cache()
    emit('per resolution faster than full maps beyond the spread at every size: ' + ('yes' if all(faster) else 'NO'))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
