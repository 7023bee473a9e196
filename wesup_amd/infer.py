"""Superpixel inference on a directory of images (reference infer.py:24-153).

Same flow as the reference: resize (fixed ``input_size`` or every factor in ``scales``), ``trainer.preprocess`` (GPU
SLIC here) -> model forward -> ``postprocess`` (round) -> nearest upsample to the original size; multi-scale
predictions are averaged and rounded, then opened with the reference's 9x9 cross.  Everything stays on the GPU until
the final mask; the opening runs on the CPU (scipy.ndimage instead of skimage.morphology, which is absent: parity
of that step unpinned) unless ``device_post`` / ``--device-post`` asks for the GPU opening (ops.binary_opening: scipy's result
bit for bit).  ``evaluate_predictions`` scores masks with the challenge metrics (utils/metrics.py; ``device=``:
utils/metrics_gpu.py)."""
import argparse
from math import ceil
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

from .models import initialize_trainer
from .utils import metrics as M
from .utils.data import SegmentationDataset


def predict_single_image(trainer, img, mask, output_size):
    """img (1,3,h,w), mask (1,C,h,w) or a 0-dim tensor -> (1,1,H,W) {0,1} at ``output_size`` (infer.py:24-35)."""
    data = (img, mask.long()) if mask.dim() == 4 else (img,)
    input_, target = trainer.preprocess(*data)
    with torch.no_grad():
        pred = trainer.model(input_)
    pred, _ = trainer.postprocess(pred, target)
    pred = pred.float().unsqueeze(0)
    return F.interpolate(pred, size=output_size, mode='nearest')


def _cross(size=9):
    """The reference's structuring element (infer.py:84-90): a cross through index (size+1)/2 -- one past the centre."""
    assert size % 2 == 1
    selem = np.zeros((size, size))
    center = int((size + 1) / 2)
    selem[center, :] = 1
    selem[:, center] = 1
    return selem


def n_classes_of(trainer):
    """Classes of the trainer's model (2 when neither the model nor the trainer's kwargs say)."""
    C = getattr(getattr(trainer, 'model', None), 'n_classes', None)
    return int(C or (getattr(trainer, 'kwargs', None) or {}).get('n_classes') or 2)


def predict(trainer, dataset, input_size=None, scales=(0.5,), device='cuda', device_post=False, stain=None):
    """Predict every image of ``dataset`` (raw items of utils.data.SegmentationDataset).  Returns a list of (H,W) masks --
    class-index maps for a model of more than two classes, which single-scale and fixed-size inference handle unchanged.
    ``device_post``: the opening of a multi-scale prediction runs on the device too (ops.binary_opening: scipy's conventions
    bit for bit) and the mask is copied to the host once, after it."""
    if n_classes_of(trainer) > 2 and input_size is None and len(scales) > 1:
        raise ValueError('multi-scale inference averages the rounded maps of the scales and rounds again: undefined for class '
                         f'indices ({n_classes_of(trainer)} classes) -- use one scale or a fixed input size')
    from scipy import ndimage
    predictions = []
    for i in range(len(dataset)):
        raw = dataset[i]
        img, mask = dataset.to_reference_item(raw)
        img = img.unsqueeze(0).to(device)
        if stain is not None:                        # the raw uint8 image, normalised on the device in front of ToTensor's scaling
            img = stain(raw[0].to(device).contiguous()).permute(2, 0, 1).float().div_(255.).unsqueeze(0)
        mask = mask.unsqueeze(0).to(device).float() if mask.dim() == 3 else mask
        orig_size = (img.size(2), img.size(3))

        def resized(size):
            im = F.interpolate(img, size=size, mode='bilinear')
            mk = F.interpolate(mask, size=size, mode='nearest') if mask.dim() == 4 else mask
            return im, mk

        if input_size is not None:
            prediction = predict_single_image(trainer, *resized(input_size), orig_size)
        else:
            multi = []
            for scale in scales:
                # (the reference rescales the already rescaled image at the second scale, infer.py:74-76; every scale
                #  starts from the original here)
                target_size = [ceil(s * scale) for s in orig_size]
                multi.append(predict_single_image(trainer, *resized(target_size), orig_size))
            prediction = torch.cat(multi).mean(dim=0).round()
        if device_post and input_size is None and len(scales) > 1:
            from . import ops
            prediction = prediction.squeeze()
            opened = ops.binary_opening((prediction != 0).to(torch.uint8).contiguous(), _cross(9))
            predictions.append(opened.to(prediction.dtype).cpu().numpy())
            continue
        prediction = prediction.squeeze().cpu().numpy()
        if input_size is None and len(scales) > 1:
            prediction = ndimage.grey_opening(prediction, footprint=_cross(9))
        predictions.append(prediction)
    return predictions


def save_predictions(predictions, dataset, output_dir='predictions', n_classes=2):
    """One PNG per image: {0, 255} for two classes, the class indices themselves for more."""
    from PIL import Image
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    for pred, img_path in zip(predictions, dataset.img_paths):
        Image.fromarray(pred.astype('uint8') * (255 if n_classes == 2 else 1)).save(output_dir / f'{img_path.stem}.png')


def evaluate_predictions(predictions, dataset, device=None):
    """Challenge metrics of the predictions against the dataset's masks (scripts/evaluate_glas.py:29-69); with ``device`` the
    object-level metrics are computed there (utils/metrics_gpu.py: the same values)."""
    rows = []
    for i, pred in enumerate(predictions):
        gt = dataset[i][1].numpy()
        gt = (gt == 1).astype(np.uint8)
        if device is not None:
            from .utils import metrics_gpu
            with torch.cuda.device(device):
                obj = metrics_gpu.challenge_scores(torch.tensor(np.asarray(pred)).to(device),
                                                   torch.from_numpy(gt).to(device))
            rows.append({'accuracy': M.accuracy(pred, gt), 'dice': M.dice(pred, gt), 'detection_f1': obj['detection_f1'],
                         'object_dice': obj['object_dice'], 'object_hausdorff': obj['object_hausdorff']})
            continue
        rows.append({'accuracy': M.accuracy(pred, gt), 'dice': M.dice(pred, gt), 'detection_f1': M.detection_f1(pred, gt),
                     'object_dice': M.object_dice(pred, gt),
                     'object_hausdorff': M.object_hausdorff(pred, gt) if pred.any() and gt.any() else float('nan')})
    keys = rows[0].keys() if rows else []
    return {k: float(np.nanmean([r[k] for r in rows])) for k in keys}, rows


def infer(trainer, data_dir, output_dir=None, input_size=None, scales=(0.5,), device='cuda', device_post=False, stain=None):
    trainer.model.eval()
    dataset = SegmentationDataset(data_dir, train=False, n_classes=n_classes_of(trainer))
    predictions = predict(trainer, dataset, input_size=input_size, scales=scales, device=device, device_post=device_post,
                          **({} if stain is None else {'stain': stain}))
    if output_dir is not None:
        save_predictions(predictions, dataset, output_dir, n_classes=n_classes_of(trainer))
    return predictions


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('data_dir')
    ap.add_argument('--model-type', default='wesup')
    ap.add_argument('--checkpoint')
    ap.add_argument('--output-dir')
    ap.add_argument('--input-size', type=int, nargs=2)
    ap.add_argument('--scales', type=float, nargs='+', default=[0.5])
    ap.add_argument('--device', default='cuda')
    ap.add_argument('--device-post', action='store_true', help='open multi-scale predictions on the device (default: scipy on the CPU)')
    from .stain import add_argument
    add_argument(ap)
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    output_dir = a.output_dir
    if output_dir is None and a.checkpoint is not None:
        output_dir = Path(a.checkpoint).parent.parent / 'results'
    from .models import checkpoint_n_classes
    from .stain import make_normalizer
    C = checkpoint_n_classes(a.checkpoint) if a.checkpoint is not None else 2
    trainer = initialize_trainer(a.model_type, device=a.device, n_classes=C)
    if a.checkpoint is not None:
        trainer.load_checkpoint(a.checkpoint)
    infer(trainer, a.data_dir, output_dir, input_size=a.input_size, scales=tuple(a.scales), device=a.device,
          device_post=a.device_post, **({} if a.stain_normalize is None else {'stain': make_normalizer(a.stain_normalize, a.device)}))


if __name__ == '__main__':
    main()
