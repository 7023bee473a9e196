"""Weak-label preparation: the mirror of the reference's ``scripts/generate_points.py``, ``scripts/generate_spl_masks.py`` and
``scripts/search_slic_params.py`` (and the ``area.csv`` that ``AreaConstraintDataset`` reads), so that a folder of images and
masks becomes the ``points*/*.csv`` and ``spl-masks*/*.npy`` the datasets of ``utils/data.py`` read without the reference
checkout, skimage, cv2, joblib or fire.

Every function has a host path in numpy that restates the reference (held to its outputs by tests/test_prepare_cpu.py against
tests/golden/prepare.npz) and a ``device=`` path on the kernels of csrc/prepare.hip and csrc/regions.hip that equals the host path
exactly: everything is integer, or a float64 formed the same way on both sides (tests/test_prepare_gpu.py).  The random draws of
``generate_points`` always happen on the host, in the reference's order and number.

    python -m wesup_amd.prepare points ROOT [-p RATIO] [--seed N] [--host]
    python -m wesup_amd.prepare spl-masks ROOT [--n-classes 2] [--sp-area 200] [--compactness 40]
    python -m wesup_amd.prepare slic-search ROOT [-r 0.5] [-a 50,60,70,80,90,100] [-c 10,20,30,40,50]
    python -m wesup_amd.prepare area ROOT
"""
import argparse
import csv
import glob
import os
from itertools import product
from pathlib import Path

import numpy as np

IMAGE_EXTENSIONS = ('jpg', 'jpeg', 'png', 'bmp')
DEFAULT_AREAS = (50, 60, 70, 80, 90, 100)
DEFAULT_COMPACTNESSES = (10, 20, 30, 40, 50)


def _torch_device(device):
    import torch
    return torch.device(device)


def _check_status(status, what):
    s = int(status.max().item())
    if s & 1:
        raise ValueError(f'{what}: a label lies outside its table')
    if s & 2:
        raise ValueError(f'{what}: a point lies outside the image or the classes')


def _round_half_even_div(num, den):
    """round(num / den) half to even in integers (int64 arrays, den > 0): numpy's ``xs.mean().round()`` of integers."""
    q, r = np.divmod(num, den)
    return q + np.where(2 * r > den, 1, np.where(2 * r == den, q & 1, 0))


# ------------------------------------------------------------------------------------------------------------ points
def _sample_within_region(region_mask, class_label, num_samples, rs):
    """generate_points.py:17-45 with an explicit RandomState."""
    xs, ys = np.where(region_mask)
    if num_samples == 1:
        x_center, y_center = int(xs.mean().round()), int(ys.mean().round())
        for _ in range(6):                                  # `retry > 5` after the increment: six tries
            x = x_center + rs.randint(-5, 6)
            y = y_center + rs.randint(-5, 6)
            try:
                if region_mask[x, y]:                       # (a negative index wraps; the point is returned as drawn)
                    return np.array([[x, y, class_label]], dtype=np.int64)
            except IndexError:
                pass
    selected = rs.permutation(len(xs))[:num_samples]
    xs, ys = xs[selected], ys[selected]
    return np.c_[xs, ys, np.full_like(xs, class_label)].astype(np.int64).reshape(-1, 3)


def _generate_points_host(mask, point_ratio, rs):
    from scipy import ndimage
    points = []
    for class_label in np.unique(mask):
        class_mask = mask == class_label
        if class_label == 0:
            points.append(_sample_within_region(class_mask, int(class_label), int(class_mask.sum() * point_ratio), rs))
        else:
            regions, n = ndimage.label(class_mask, structure=np.ones((3, 3), dtype=np.int32))    # skimage.measure.label, 8-connected
            for idx in range(1, n + 1):
                region_mask = regions == idx
                num_samples = max(1, int(region_mask.sum() * point_ratio))
                points.append(_sample_within_region(region_mask, int(class_label), num_samples, rs))
    return np.concatenate(points)


def _generate_points_device(mask, point_ratio, rs, device):
    import torch
    from . import ops
    H, W = mask.shape
    m = torch.from_numpy(np.ascontiguousarray(mask)).to(device)
    classes = [int(c) for c in np.unique(mask)]
    # one label map for the whole image: 0 = the background region, then every class's components in raster order of their first
    # pixel, class after class -- the order in which the reference walks them
    merged = torch.zeros(H, W, dtype=torch.int32, device=device)
    region_class = [0]
    for c in classes:
        if c == 0:
            continue
        lab, n = ops.cc_label((m == c).to(torch.uint8), 8, 1)
        n = int(n.item())
        merged += torch.where(lab > 0, lab + (len(region_class) - 1), torch.zeros_like(lab))
        region_class += [c] * n
    L = len(region_class) - 1
    stats, status = ops.label_stats(merged, L)
    _check_status(status, 'generate_points')
    stats = stats.cpu().numpy()
    count, sum_r, sum_c = stats[:, 0], stats[:, 1], stats[:, 2]
    safe = np.maximum(count, 1)
    center_r, center_c = _round_half_even_div(sum_r, safe), _round_half_even_div(sum_c, safe)
    merged_host = None
    out, picks = [], []                                     # picks: (position in out, region, k-th pixel in raster order)
    for region in range(0 if 0 in classes else 1, L + 1):
        cls, cnt = region_class[region], int(count[region])
        num_samples = int(np.int64(cnt) * point_ratio)
        if region > 0:
            num_samples = max(1, num_samples)
        hit = None
        if num_samples == 1:
            if merged_host is None:
                merged_host = merged.cpu().numpy()           # one copy per image serves every membership look-up
            for _ in range(6):
                x = int(center_r[region]) + rs.randint(-5, 6)
                y = int(center_c[region]) + rs.randint(-5, 6)
                if -H <= x < H and -W <= y < W and merged_host[x, y] == region:
                    hit = (x, y, cls)
                    break
        if hit is not None:
            out.append(hit)
            continue
        for k in rs.permutation(cnt)[:num_samples]:
            picks.append((len(out), region, int(k)))
            out.append((0, 0, cls))
    out = np.array(out, dtype=np.int64).reshape(-1, 3)
    if picks:
        if L >= ops.LABEL_SORT_MAX_LABELS:
            raise ValueError(f'generate_points: {L} regions in one mask, the device pixel lists hold fewer than '
                             f'{ops.LABEL_SORT_MAX_LABELS} (use the host path)')
        lists = ops.label_sort(merged, L)
        _check_status(lists.status, 'generate_points')
        start = lists.start.cpu().numpy().astype(np.int64)
        where, region, k = (np.array(v, dtype=np.int64) for v in zip(*picks))
        idx = torch.from_numpy(start[region] + k).to(device)
        pix = lists.pix[idx].cpu().numpy().astype(np.int64)  # the selected pixels, gathered once per image
        out[where, 0], out[where, 1] = pix // W, pix % W
    return out


def generate_points(mask, point_ratio=1e-4, rs=None, device=None):
    """Point labels of a class-index mask (H, W): int64 (P, 3) rows of (row, col, class), what the reference's
    ``_generate_points`` returns (generate_points.py:48-78).  Background (class 0) is ONE region without any labelling and gets
    ``int(pixels * point_ratio)`` points (possibly none); every 8-connected component of a class above 0 gets
    ``max(1, int(pixels * point_ratio))``.  A region that gets one point tries up to six times the rounded centroid displaced by
    ``randint(-5, 6)`` per axis and returns the first candidate inside the region; otherwise (and for more points)
    ``permutation(pixels)[:n]`` picks pixels in raster order -- drawn even for n = 0.

    ``rs``: an ``np.random.RandomState`` (default: a fresh unseeded one).  The draws happen on the host in the reference's order
    and number, so ``RandomState(s)`` gives what the reference gives under ``np.random.seed(s)``.

    The reference's quirks are kept: a negative candidate index wraps around like any numpy index and the point is returned AS
    DRAWN, possibly negative (the csv then holds a negative coordinate); a candidate outside [-H, H) x [-W, W) is a miss.

    ``device``: connected components, region sizes and centroids (integer sums, rounded half to even like ``mean().round()``)
    and the k-th pixel of a region come from the device; equal to the host path for equal ``rs`` state."""
    mask = np.asarray(mask)
    if mask.ndim != 2:
        raise ValueError(f'generate_points: a 2-D class-index mask, got shape {mask.shape}')
    if mask.dtype == np.bool_:
        mask = mask.astype(np.uint8)
    if mask.dtype != np.uint8:
        raise ValueError(f'generate_points: a uint8 mask, got {mask.dtype}')
    rs = rs if rs is not None else np.random.RandomState()
    if device is None:
        return _generate_points_host(mask, point_ratio, rs)
    return _generate_points_device(mask, point_ratio, rs, _torch_device(device))


def generate_points_dir(root_dir, point_ratio=1e-4, seed=None, device=None, name=None, log=print):
    """The script: ``root_dir/masks/*`` -> ``root_dir/points-RATIO/STEM.csv`` (``name`` overrides the folder), rows
    ``col,row,class``.  The masks are walked in sorted order with one RandomState(seed).  Returns the folder."""
    from PIL import Image
    root = Path(root_dir).expanduser()
    mask_dir = root / 'masks'
    if not mask_dir.exists():
        raise FileNotFoundError('Cannot generate dot annotation without masks.')
    label_dir = root / (name or f'points-{str(point_ratio)}')
    label_dir.mkdir(exist_ok=True)
    log('Generating point annotation ...')
    rs = np.random.RandomState(seed)
    nums = []
    for path in sorted(mask_dir.iterdir()):
        with Image.open(path) as im:
            mask = np.array(im)
        points = generate_points(mask, point_ratio, rs, device)
        points[:, [0, 1]] = points[:, [1, 0]]               # conform to the xy format
        with open(label_dir / f'{path.stem}.csv', 'w') as fp:
            csv.writer(fp).writerows(points.tolist())
        nums.append(len(points))
    log(f'Average number of points: {np.mean(nums)}.')
    return label_dir


# ---------------------------------------------------------------------------------------------------------- spl-masks
def _segments_array(segments):
    import torch
    return segments.detach().cpu().numpy() if isinstance(segments, torch.Tensor) else np.asarray(segments)


def _segments_tensor(segments, device):
    import torch
    t = segments if isinstance(segments, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(segments))
    return t.to(device=device, dtype=torch.int32).contiguous()


def _wrap_points(points, H, W, C):
    """(P, 3) of (row, col, class) with numpy's index rules: [-n, n) wraps, anything else is an IndexError."""
    p = np.asarray(points, dtype=np.int64).reshape(-1, 3).copy()
    for axis, n in enumerate((H, W, C)):
        bad = (p[:, axis] < -n) | (p[:, axis] >= n)
        if bad.any():
            raise IndexError(f'index {int(p[bad, axis][0])} is out of bounds for axis {axis} with size {n}')
        p[:, axis] += np.where(p[:, axis] < 0, n, 0)
    return p


def spl_mask(segments, points, n_classes=2, device=None):
    """uint8 (H, W, C): 1 where some point of class c lies in the pixel's superpixel (generate_spl_masks.py:28-33).  ``points``
    are (row, col, class) rows as ``generate_points`` returns them; indexes in [-H, H) x [-W, W) x [-C, C) wrap as numpy's do,
    anything else raises IndexError on the host.  ``segments``: an (H, W) integer label map (array or tensor); on the device its
    ids must be >= 0."""
    if device is None:
        segments = _segments_array(segments)
        H, W = segments.shape
        points = _wrap_points(points, H, W, n_classes)
        mask = np.zeros((H, W, n_classes), dtype='uint8')
        for x, y, class_ in points:
            mask[segments == segments[x, y], class_] = 1
        return mask
    import torch
    from . import ops
    device = _torch_device(device)
    seg = _segments_tensor(segments, device)
    if seg.dim() != 2:
        raise ValueError(f'spl_mask: an (H, W) label map, got {tuple(seg.shape)}')
    H, W = seg.shape
    points = _wrap_points(points, H, W, n_classes)
    K = int(seg.max().item()) + 1
    if K < 1:
        raise ValueError('spl_mask: negative superpixel ids')
    pts = torch.from_numpy(points.astype(np.int32)).to(device)
    out, status = ops.spl_paint(seg, pts, K, n_classes)
    _check_status(status, 'spl_mask')
    return out.cpu().numpy()


def _read_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert('RGB'), dtype=np.uint8)


def _device_slic(imgs_u8, n_segments, compactness, device):
    """ops.slic of a stack of (H, W, 3) uint8 images of one size -> (labels (B, H, W) int32 on the device, n_labels (B,))."""
    import torch
    from . import ops
    x = torch.from_numpy(np.ascontiguousarray(np.stack(imgs_u8))).to(device)
    return _slic_resident(x.permute(0, 3, 1, 2).float().div(255.0).contiguous(), n_segments, compactness)


def _slic_resident(x, n_segments, compactness):
    from . import ops
    return ops.slic(x, int(n_segments), float(compactness))


def generate_spl_masks(data_root, n_classes=2, sp_area=200, compactness=40, segment_fn=None, device=None, log=print):
    """For every ``points*`` folder of ``data_root``: ``spl-masks*/STEM.npy`` of shape (H, W, C) uint8, one per image of
    ``data_root/images`` (generate_spl_masks.py:12-55; images and csv files pair up in sorted order, csv rows are
    ``col,row,class``).  ``n_segments = H * W // sp_area``.  The segmentation is ``ops.slic`` on ``device`` (default: the current
    one); ``segment_fn(img_hwc_u8, n_segments, compactness)`` plugs in another one, and the masks are then painted on the host
    unless ``device`` is given.  Returns the list of folders written."""
    data_root = Path(data_root).expanduser()
    img_dir = data_root / 'images'
    written = []
    for point_dir in sorted(data_root.glob('points*')):
        if not point_dir.is_dir():
            continue
        log(f'Processing {point_dir} ...')
        img_paths = sorted(img_dir.iterdir())
        point_paths = sorted(point_dir.iterdir())
        output_dir = data_root / point_dir.name.replace('points', 'spl-masks')
        output_dir.mkdir(exist_ok=True)
        for img_path, point_path in zip(img_paths, point_paths):
            img = _read_rgb(img_path)
            height, width = img.shape[:2]
            with open(point_path) as fp:
                rows = [[int(d) for d in point] for point in csv.reader(fp) if point]
            points = np.array(rows, dtype=np.int64).reshape(-1, 3)[:, [1, 0, 2]]
            n_segments = (height * width) // sp_area
            if segment_fn is not None:
                segments, dev = segment_fn(img, n_segments, compactness), device
            else:
                dev = device if device is not None else 'cuda'
                segments = _device_slic([img], n_segments, compactness, _torch_device(dev))[0][0]
            mask = spl_mask(segments, points, n_classes, device=dev)
            np.save(output_dir / img_path.name.replace(img_path.suffix, '.npy'), mask)
        log(f'Saved to {output_dir}.')
        written.append(output_dir)
    return written


# -------------------------------------------------------------------------------------------------------- SLIC search
def list_images(path):
    """search_slic_params.py:12-18: the jpg / jpeg / png / bmp files of a folder, sorted by path."""
    images = []
    for ext in IMAGE_EXTENSIONS:
        images.extend(glob.glob(os.path.join(str(path), f'*.{ext}')))
    return sorted(images)


def read_image(img_path, rescale_factor=0.5, mode=None):
    """search_slic_params.py:21-27: PIL, ``int()`` of the scaled sizes, BILINEAR unless ``mode`` says otherwise."""
    from PIL import Image
    mode = Image.BILINEAR if mode is None else mode
    with Image.open(img_path) as img:
        target_width = int(img.width * rescale_factor)
        target_height = int(img.height * rescale_factor)
        return np.array(img.resize((target_width, target_height), resample=mode))


def _mask_2d(mask):
    mask = _segments_array(mask)
    if mask.ndim != 2:
        raise ValueError(f'oracle_accuracy: a 2-D mask, got shape {mask.shape}')
    if mask.dtype == np.bool_:
        mask = mask.astype(np.uint8)
    if mask.dtype != np.uint8:
        raise ValueError(f'oracle_accuracy: a uint8 mask, got {mask.dtype}')
    return mask


def oracle_accuracy(segments, mask, device=None):
    """The reference's ``run_param_group`` (search_slic_params.py:30-38) for given segments: every superpixel is painted with the
    rounded mean of ``mask`` (uint8, 2-D) over its pixels -- ``mean().round()``, half to even, cast to uint8 -- and the result is
    compared with ``mask``: float64 ``agree / (H * W)``.  An id without pixels paints nothing."""
    if device is None:
        segments, mask = _segments_array(segments), _mask_2d(mask)
        if segments.shape != mask.shape:
            raise ValueError(f'oracle_accuracy: segments {segments.shape} and mask {mask.shape}')
        if segments.min() < 0:
            raise ValueError('oracle_accuracy: negative superpixel ids')
        seg = segments.ravel().astype(np.int64)
        n = int(seg.max()) + 1
        count = np.bincount(seg, minlength=n)
        total = np.bincount(seg, weights=mask.ravel().astype(np.float64), minlength=n)     # integers: exact in float64
        with np.errstate(invalid='ignore', divide='ignore'):
            mean = total / count                             # mask[sp_mask].mean()
        vote = np.where(count > 0, mean.round(), 0).astype(np.uint8)
        oracle_pred = vote[seg].reshape(mask.shape)
        return np.mean(oracle_pred == mask)
    import torch
    from . import ops
    device = _torch_device(device)
    seg = _segments_tensor(segments, device)
    if isinstance(mask, torch.Tensor) and mask.is_cuda:
        if mask.dim() != 2 or mask.dtype != torch.uint8:
            raise ValueError(f'oracle_accuracy: a 2-D uint8 mask, got {mask.dtype} {tuple(mask.shape)}')
        m = mask.to(device).contiguous()
    else:
        m = torch.from_numpy(np.ascontiguousarray(_mask_2d(mask))).to(device)
    if seg.shape != m.shape:
        raise ValueError(f'oracle_accuracy: segments {tuple(seg.shape)} and mask {tuple(m.shape)}')
    K = int(seg.max().item()) + 1
    _, agree, status = ops.sp_vote(seg, m, K, paint=False)
    _check_status(status, 'oracle_accuracy')
    return np.float64(int(agree[0].item())) / np.float64(seg.numel())


def format_search_line(area, compactness, acc):
    return f'# Segments = {area}, Compactness = {compactness}, Acc = {acc:.4f}'


def slic_search(dataset_path, rescale_factor=0.5, areas=DEFAULT_AREAS, compactnesses=DEFAULT_COMPACTNESSES, segment_fn=None,
                device=None, log=print):
    """search_slic_params.py:41-69: the mean oracle accuracy over ``dataset_path/images`` + ``/masks`` for every (area,
    compactness) pair, ``n_segments = int(H * W / area)`` -> ``{(area, compactness): np.mean(accs)}``, one line per pair in the
    reference's words.  Every image and mask is uploaded once; all pairs run against the resident copies, images of equal size
    as one ``ops.slic`` batch.  ``segment_fn(img_hwc_u8, n_segments, compactness)`` plugs in another segmentation (the accuracy
    is then ``oracle_accuracy`` per image, on ``device`` when given, else on the host).  The reference parses ``-r`` and never
    uses it (it always halves); here ``rescale_factor`` is honoured, and the default is the reference's behaviour."""
    from PIL import Image
    log('Reading images and masks ...')
    images = [read_image(p, rescale_factor) for p in list_images(os.path.join(str(dataset_path), 'images'))]
    mask_paths = list_images(os.path.join(str(dataset_path), 'masks'))
    masks = [read_image(p, rescale_factor, mode=Image.NEAREST) for p in mask_paths]
    for p, m in zip(mask_paths, masks):
        if m.ndim != 2:
            raise ValueError(f'slic_search: {p} is not a single-channel mask (shape {m.shape})')
    n = min(len(images), len(masks))                         # zip(images, masks)
    images, masks = images[:n], [_mask_2d(m) for m in masks[:n]]
    for i, (img, m) in enumerate(zip(images, masks)):
        if img.shape[:2] != m.shape:
            raise ValueError(f'slic_search: image {i} is {img.shape[:2]}, its mask {m.shape}')
    results = {}
    if segment_fn is not None:
        for area, comp in product(areas, compactnesses):
            accs = [oracle_accuracy(segment_fn(img, int(img.shape[0] * img.shape[1] / area), comp), m, device=device)
                    for img, m in zip(images, masks)]
            results[(area, comp)] = np.mean(accs)
            log(format_search_line(area, comp, results[(area, comp)]))
        return results
    import torch
    from . import ops
    dev = _torch_device(device if device is not None else 'cuda')
    groups = {}                                              # size -> image indexes
    for i, img in enumerate(images):
        if img.ndim == 2:
            images[i] = img = np.stack([img] * 3, axis=-1)
        groups.setdefault(img.shape[:2], []).append(i)
    resident = []
    for (H, W), idx in groups.items():
        x = torch.from_numpy(np.stack([images[i][..., :3] for i in idx])).to(dev)
        x = x.permute(0, 3, 1, 2).float().div(255.0).contiguous()
        m = torch.from_numpy(np.stack([masks[i] for i in idx])).to(dev)
        resident.append((H, W, idx, x, m))
    for area, comp in product(areas, compactnesses):
        accs = np.zeros(n, dtype=np.float64)
        for H, W, idx, x, m in resident:
            labels, n_labels = _slic_resident(x, int(H * W / area), comp)
            K = max(int(n_labels.max().item()), 1)
            _, agree, status = ops.sp_vote(labels, m, K, paint=False)
            _check_status(status, 'slic_search')
            accs[idx] = agree.cpu().numpy().astype(np.float64) / np.float64(H * W)
        results[(area, comp)] = np.mean(accs) if n else np.float64('nan')
        log(format_search_line(area, comp, results[(area, comp)]))
    return results


# --------------------------------------------------------------------------------------------------------------- area
def generate_area(root_dir, log=print):
    """``root_dir/area.csv`` as the reference's scripts/generate_area.py writes it and ``AreaConstraintDataset`` reads it: the
    header ``,img,area`` (pandas' index column first) and one row ``i,NAME,mean`` per file of ``root_dir/masks`` in sorted order,
    ``mean`` the mean of the mask as read (the foreground fraction of a {0, 1} mask).  Host only: one ``mean()`` per mask."""
    from PIL import Image
    root = Path(root_dir).expanduser()
    mask_dir = root / 'masks'
    if not mask_dir.exists():
        raise FileNotFoundError('Cannot generate area information without masks.')
    path = root / 'area.csv'
    rows = []
    for idx, name in enumerate(sorted(os.listdir(mask_dir))):
        with Image.open(mask_dir / name) as im:
            rows.append((idx, name, repr(float(np.array(im).mean()))))
    with open(path, 'w', newline='') as fp:
        writer = csv.writer(fp, lineterminator='\n')
        writer.writerow(['', 'img', 'area'])
        writer.writerows(rows)
    log(f'Area information saved to {path}.')
    return path


# ------------------------------------------------------------------------------------------------------- command line
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog='python -m wesup_amd.prepare', description='Weak-label preparation.')
    sub = ap.add_subparsers(dest='command', required=True)
    p = sub.add_parser('points', help='Dot annotation generator.')
    p.add_argument('root_dir', help='Path to data root directory with mask-level annotation.')
    p.add_argument('-p', '--point-ratio', type=float, default=1e-4, help='Percentage of labeled objects (regions) for each class')
    p.add_argument('--seed', type=int, default=None, help='Seed of the RandomState shared by all masks')
    s = sub.add_parser('spl-masks', help='Superpixel label masks from points.')
    s.add_argument('data_root')
    s.add_argument('--n-classes', '--n_classes', type=int, default=2)
    s.add_argument('--sp-area', '--sp_area', type=int, default=200)
    s.add_argument('--compactness', type=float, default=40)
    q = sub.add_parser('slic-search', help='Oracle accuracy of SLIC parameter pairs.')
    q.add_argument('dataset_path', help='Path to dataset with images and masks')
    q.add_argument('-r', '--rescale-factor', type=float, default=0.5, help='Rescale factor for resizing images and masks')
    q.add_argument('-a', '--area', default=','.join(str(v) for v in DEFAULT_AREAS), help='Approximate number of superpixels')
    q.add_argument('-c', '--compactness', default=','.join(str(v) for v in DEFAULT_COMPACTNESSES),
                   help='Compactness parameter for SLIC')
    a = sub.add_parser('area', help='area.csv of the masks.')
    a.add_argument('root_dir')
    for x in (p, s, q):
        x.add_argument('--host', action='store_true', help='label maps on the host (the segmentation itself stays on the device)')
        x.add_argument('--device', default=None)
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    if a.command == 'area':
        return generate_area(a.root_dir)
    device = None if a.host else (a.device or 'cuda')
    if a.command == 'points':
        return generate_points_dir(a.root_dir, a.point_ratio, a.seed, device)
    if a.command == 'spl-masks':
        if a.host:                                           # segment on the device, paint on the host
            dev = _torch_device(a.device or 'cuda')
            return generate_spl_masks(a.data_root, a.n_classes, a.sp_area, a.compactness,
                                      segment_fn=lambda img, n, c: _device_slic([img], n, c, dev)[0][0])
        return generate_spl_masks(a.data_root, a.n_classes, a.sp_area, a.compactness, device=device)
    areas = [int(v) for v in a.area.split(',')]
    comps = [int(v) for v in a.compactness.split(',')]
    if a.host:
        dev = _torch_device(a.device or 'cuda')
        return slic_search(a.dataset_path, a.rescale_factor, areas, comps,
                           segment_fn=lambda img, n, c: _device_slic([img[..., :3]], n, c, dev)[0][0])
    return slic_search(a.dataset_path, a.rescale_factor, areas, comps, device=device)


if __name__ == '__main__':
    main()
