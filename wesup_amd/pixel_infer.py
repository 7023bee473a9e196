"""Whole-image multi-scale pixel inference (mirror of the reference's ``pixel_infer.py``).

Every image of ``DATA/images`` is rescaled (bilinear, ``align_corners=True``) by each factor of ``--scales``, run through
``WESUPPixelInference`` as a whole, class 1 is resized back to the image's size and the scales are averaged; the rounded mean
is written as a PNG.  The image is uploaded once as uint8 and everything up to the averaged probability map stays on the
device (``ops.image_resize_u8`` -> the model -> ``ops.plane_resize_acc``); one copy brings the map back.

    python -m wesup_amd.pixel_infer DATA -c CKPT [-s 0.5,0.75] [-o OUT] [--device D] [--full-maps]

The model's forward is ``WESUPPixelInference.forward_per_resolution`` (the first fc layer at each resolution, DESIGN.md
3.8); ``--full-maps`` runs the shipped ``forward`` on the (HW, 2112) feature map instead, for cross-checking.
"""
import argparse
from pathlib import Path

import numpy as np
import torch

from . import ops
from .infer_tile import _load_pixel_model, _upload


def parse_scales(text):
    """``'0.5,0.75'`` -> ``(0.5, 0.75)`` (pixel_infer.py:67)."""
    scales = tuple(float(s) for s in str(text).split(',') if s.strip())
    if not scales or any(not s > 0 for s in scales):
        raise ValueError(f'scales {text!r}: expected positive factors separated by commas')
    return scales


def target_size(H, W, scale):
    """The size an (H, W) image is run at under ``scale`` (pixel_infer.py:44-45)."""
    return int(H * scale), int(W * scale)


def output_name(name):
    """The file a prediction for image ``name`` is written to (pixel_infer.py:54)."""
    return str(name).replace('.jpg', '.png')


def default_output_dir(checkpoint):
    """``main``'s output directory when none is given (pixel_infer.py:26-30)."""
    return Path(checkpoint).expanduser().parent.parent / 'results'


def cli_output_dir(checkpoint, scales_text, data_root):
    """The command line's output directory without ``-o`` (pixel_infer.py:75-76)."""
    return Path(checkpoint).expanduser().parent.parent / f'results-pixel-{scales_text}' / Path(data_root).expanduser().name


def image_paths(data_root):
    """The files of ``data_root/images``, sorted; ``data_root`` a str or a Path (the reference's ``__main__`` hands ``main`` a
    str and fails on ``/``)."""
    return sorted((Path(data_root).expanduser() / 'images').iterdir())


def _scale_loop(name, model, img_u8_hwc, scales, device, full_maps, stain, tail, accumulate):
    """The walk over the scales: one upload; per scale the down-resize, the model and ``accumulate(pred (h, w, C), mean, alpha,
    i > 0)`` into the running mean (``alpha = 1 / len(scales)``: no pass of its own for the mean).  Returns the (H, W, *tail) fp32
    mean on the device."""
    scales = tuple(scales)
    if not scales:
        raise ValueError(f'{name}: no scales')
    img_d = _upload(img_u8_hwc, device, stain)
    H, W = img_d.shape[:2]
    mean = torch.empty(H, W, *tail, dtype=torch.float32, device=img_d.device)
    with torch.no_grad():
        for i, scale in enumerate(scales):
            h, w = target_size(H, W, scale)
            if h < 1 or w < 1:
                raise ValueError(f'scale {scale} leaves nothing of a {H} x {W} image')
            x = ops.image_resize_u8(img_d, h, w)
            pred = model(x) if full_maps else model.forward_per_resolution(x)[0]          # (h, w, C)
            accumulate(pred, mean, 1.0 / len(scales), i > 0)
    return mean


def pixel_predict(model, img_u8_hwc, scales=(0.5,), device='cuda', full_maps=False, stain=None):
    """(H, W, 3) uint8 image -> (H, W) fp32 class-1 probability averaged over ``scales`` (pixel_infer.py:40-53; the caller
    rounds).  Per scale class 1 is resized back into the running mean (``ops.plane_resize_acc``); one copy to the host."""
    def accumulate(pred, mean, alpha, more):
        ops.plane_resize_acc(pred[..., 1], mean, alpha=alpha, accumulate=more)
    return _scale_loop('pixel_predict', model, img_u8_hwc, scales, device, full_maps, stain, (), accumulate).cpu().numpy()


def pixel_predict_classes(model, img_u8_hwc, scales=(0.5,), device='cuda', full_maps=False, stain=None):
    """``pixel_predict`` for a model of more than two classes: (H, W, 3) uint8 image -> (H, W) uint8 class map.  Per scale all C
    probabilities are resized back in one pass into one (H, W, C) running mean (``ops.planes_resize_acc``, every plane the
    arithmetic of ``plane_resize_acc``), then the first maximum per pixel (``ops.class_argmax_u8``) and one copy to the host."""
    def accumulate(pred, mean, alpha, more):
        ops.planes_resize_acc(pred.contiguous(), mean, alpha=alpha, accumulate=more)
    mean = _scale_loop('pixel_predict_classes', model, img_u8_hwc, scales, device, full_maps, stain, (model.n_classes,), accumulate)
    return ops.class_argmax_u8(mean).cpu().numpy()


def main(data_root, checkpoint=None, output_dir=None, scales=(0.5,), device=None, full_maps=False, stain_normalize=None):
    """pixel_infer.py:20-56 on ``data_root/images``: one PNG of ``round(mean probability) * 255`` per image -- of the class
    indices for a checkpoint of more than two classes (``pixel_predict_classes``).  Returns the written paths."""
    from PIL import Image
    if device is None:
        device = 'cuda'
    if output_dir is None and checkpoint is not None:
        output_dir = default_output_dir(checkpoint)
    if output_dir is None:
        raise ValueError('pixel_infer: neither an output directory nor a checkpoint to derive one from')
    output_dir = Path(output_dir).expanduser()
    output_dir.mkdir(parents=True, exist_ok=True)
    model = _load_pixel_model(checkpoint, device, multiclass=True)
    model.eval()
    kw = {}
    if stain_normalize not in (None, False):                   # --stain-normalize [TARGET]: one fit per image on the resident tensor
        from .stain import make_normalizer
        kw['stain'] = make_normalizer(stain_normalize, device)
    written = []
    for path in image_paths(data_root):
        img = np.asarray(Image.open(path).convert('RGB'))
        out = output_dir / output_name(path.name)
        if model.n_classes > 2:                      # the class indices themselves, no x 255 (infer.save_predictions)
            pred = pixel_predict_classes(model, img, scales, device=device, full_maps=full_maps, **kw)
        else:
            pred = pixel_predict(model, img, scales, device=device, full_maps=full_maps, **kw).round().astype('uint8') * 255
        Image.fromarray(pred).save(out, format='PNG')
        written.append(out)
    return written


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('data_root')
    ap.add_argument('-c', '--checkpoint', required=True)
    ap.add_argument('-s', '--scales', default='0.5')
    ap.add_argument('-o', '--output')
    ap.add_argument('--device', default=None)
    ap.add_argument('--full-maps', action='store_true',
                    help="the shipped forward on the (HW, 2112) feature map instead of the per-resolution one (cross-check)")
    from .stain import add_argument
    add_argument(ap)
    a = ap.parse_args(argv)
    a.scale_values = parse_scales(a.scales)
    a.output_dir = Path(a.output).expanduser() if a.output else cli_output_dir(a.checkpoint, a.scales, a.data_root)
    return a


def cli(argv=None):
    a = parse_args(argv)
    main(a.data_root, checkpoint=a.checkpoint, output_dir=a.output_dir, scales=a.scale_values, device=a.device,
         full_maps=a.full_maps, **({} if a.stain_normalize is None else {'stain_normalize': a.stain_normalize}))


if __name__ == '__main__':
    cli()
