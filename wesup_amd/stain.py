"""Macenko stain normalisation and stain jitter of H&E images (Macenko et al., ISBI 2009).

H&E colour differs from lab to lab and scanner to scanner; a model trained on one collection and scored on another meets that
first.  The fit finds an image's two stain vectors (the extreme directions of its optical density in the plane of the two leading
eigenvectors of the tissue covariance) and the 99th percentile of their concentrations; normalisation re-expresses the image
with a target's vectors and concentrations, jitter scales and shifts the image's own concentrations and keeps the residual.

The device path (``ops.stain_fit`` / ``ops.stain_apply``, csrc/stain.hip) works on uint8 tensors that already live on the GPU
and reads nothing back; ``host=True`` runs the same definition in numpy (float64) for users without the library.

    python -m wesup_amd.stain SRC_DIR OUT_DIR [--target IMG] [--host]
"""
import argparse
from pathlib import Path

import numpy as np

IO, ALPHA, BETA, MIN_TISSUE = 240.0, 1.0, 0.15, 16
PARALLEL_DET = 1e-6
MIN_MAXC = 1e-6
BLOCK = 16
TARGET_HE = ((0.5626, 0.2159), (0.7201, 0.8012), (0.4062, 0.5581))
TARGET_MAXC = (1.9705, 1.0308)
IMAGE_SUFFIXES = ('.png', '.jpg', '.jpeg', '.bmp', '.tif', '.tiff')


# ---------------------------------------------------------------- the host path (numpy, float64)
def _table(io):
    return -np.log((np.arange(256, dtype=np.float64) + 1.0) / float(io))


def _percentile(a, q):
    s = np.sort(a)
    pos = float(q) * float(len(s) - 1) / 100.0
    lo = min(max(int(np.floor(pos)), 0), len(s) - 1)
    hi = min(lo + 1, len(s) - 1)
    return s[lo] + (s[hi] - s[lo]) * (pos - np.floor(pos))


def _pinv(he):
    g = he.T @ he
    det = g[0, 0] * g[1, 1] - g[0, 1] * g[1, 0]
    if not abs(det) >= PARALLEL_DET:                 # parallel stain vectors: no inverse to speak of
        return None, det
    return np.array([[g[1, 1], -g[0, 1]], [-g[1, 0], g[0, 0]]]) / det @ he.T, det


def host_fit(img, stride=1, io=IO, alpha=ALPHA, beta=BETA, min_tissue=MIN_TISSUE):
    """(H, W, 3) uint8 -> the fit as 16 float64 {HE[3][2], pinv[2][3], maxC[2], n_tissue, valid}; all zeros but n_tissue when the
    image has fewer than ``min_tissue`` tissue samples, parallel stain vectors or no concentration to speak of."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[-1] != 3:
        raise ValueError(f'host_fit: expected an (H, W, 3) uint8 image, got {img.dtype} {img.shape}')
    od = _table(io)[np.ascontiguousarray(img[::stride, ::stride]).reshape(-1, 3)]
    tissue = (od >= beta).all(1)
    blk = np.zeros(BLOCK)
    blk[14] = n = int(tissue.sum())
    if n < max(int(min_tissue), 2):
        return blk
    odt = od[tissue]
    _, v = np.linalg.eigh(np.cov(odt.T))
    v = v[:, ::-1][:, :2].copy()
    if v[:, 0].sum() < 0:
        v[:, 0] = -v[:, 0]
    if v[np.argmax(np.abs(v[:, 1])), 1] < 0:
        v[:, 1] = -v[:, 1]
    t = odt @ v
    phi = np.arctan2(t[:, 1], t[:, 0])
    lo, hi = _percentile(phi, alpha), _percentile(phi, 100.0 - alpha)
    a = v @ np.array([np.cos(lo), np.sin(lo)])
    c = v @ np.array([np.cos(hi), np.sin(hi)])
    he = np.stack([a, c], 1) if a[0] > c[0] else np.stack([c, a], 1)
    pv, det = _pinv(he)
    if not abs(det) >= PARALLEL_DET:
        return blk
    conc = od @ pv.T
    maxc = np.array([_percentile(conc[:, 0], 99.0), _percentile(conc[:, 1], 99.0)])
    if not (maxc >= MIN_MAXC).all():
        return blk
    blk[0:6], blk[6:12], blk[12:14], blk[15] = he.reshape(-1), pv.reshape(-1), maxc, 1.0
    return blk


def host_apply(img, src, dst, jitter=(1.0, 0.0, 1.0, 0.0), keep_residual=0.0, io=IO):
    """One (H, W, 3) uint8 image through c = pinv_s OD; c' = c (maxC_d / maxC_s) a + b; OD' = HE_d c' + keep (OD - HE_s c)."""
    img = np.asarray(img)
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    if not (src[15] and dst[15]):
        return img.copy()
    od = _table(io)[img.reshape(-1, 3)]
    hs, ps, hd = src[0:6].reshape(3, 2), src[6:12].reshape(2, 3), dst[0:6].reshape(3, 2)
    j = np.asarray(jitter, dtype=np.float64)
    c = od @ ps.T
    c2 = c * (dst[12:14] / src[12:14]) * j[[0, 2]] + j[[1, 3]]
    od2 = c2 @ hd.T + float(keep_residual) * (od - c @ hs.T)
    return np.rint(np.clip(float(io) * np.exp(-od2) - 1.0, 0, 255)).astype(np.uint8).reshape(img.shape)


def default_target():
    """The target in common use as a block of 16 float64: HE = [[0.5626, 0.2159], [0.7201, 0.8012], [0.4062, 0.5581]],
    maxC = [1.9705, 1.0308]."""
    blk = np.zeros(BLOCK)
    he = np.array(TARGET_HE)
    blk[0:6], blk[6:12], blk[12:14], blk[15] = he.reshape(-1), _pinv(he)[0].reshape(-1), TARGET_MAXC, 1.0
    return blk


def read_image(path):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(path).convert('RGB'), dtype=np.uint8))


# ---------------------------------------------------------------- the public surface
def _is_tensor(x):
    import torch
    return isinstance(x, torch.Tensor)


class StainNormalizer:
    """``target``: None (default_target()), an (H, W, 3) uint8 image (array or tensor) that is fitted once, or a path to one.
    ``host=True``: numpy in and out, no library.  Otherwise tensors on ``device`` in and out:

        norm = StainNormalizer(device='cuda:0')
        block = norm.fit(img_u8)                    # (B, 16) on the device, nothing read back
        out = norm(img_u8)                          # (H, W, 3) or (B, H, W, 3) uint8, device in, device out
        norm(img_u8, out=img_u8)                    # in place (the inference tools: one extra pass per image / slide)

    An image whose fit is invalid (empty glass, a single colour, too little tissue) comes back as it is."""

    def __init__(self, target=None, device='cuda:0', host=False, stride=None, io=IO, alpha=ALPHA, beta=BETA, min_tissue=MIN_TISSUE):
        self.host, self.stride = bool(host), stride
        self.kw = dict(io=io, alpha=alpha, beta=beta, min_tissue=min_tissue)
        self.device = None
        if not self.host:
            import torch
            self.device = torch.device(device)
        if isinstance(target, (str, Path)):
            target = read_image(target)
        if target is None:
            blk = default_target()
        elif self.host:
            target = target.cpu().numpy() if _is_tensor(target) else np.asarray(target)
            blk = host_fit(target, self._stride(target.shape[:2]), **self.kw)
        else:
            import torch
            t = target if _is_tensor(target) else torch.from_numpy(np.ascontiguousarray(target))
            blk = self.fit(t.to(self.device).contiguous()).double().cpu().numpy().reshape(BLOCK)     # (once, at construction)
        if not blk[15]:
            raise ValueError('StainNormalizer: the target image has no valid stain fit '
                             f'({int(blk[14])} tissue samples; too little tissue, or one colour)')
        self.target_host = blk
        self.target = None
        if not self.host:
            import torch
            self.target = torch.from_numpy(blk.astype(np.float32)).to(self.device)

    def _stride(self, hw):
        if self.stride is not None:
            return int(self.stride)
        s = 1
        while -(-hw[0] // s) * -(-hw[1] // s) > (1 << 24):
            s += 1
        return s

    def fit(self, img):
        """The fit block(s) of ``img``: (B, 16) fp32 on the device, or (B, 16) float64 arrays on the host path."""
        if self.host:
            img = np.asarray(img)
            imgs = img[None] if img.ndim == 3 else img
            return np.stack([host_fit(i, self._stride(i.shape[:2]), **self.kw) for i in imgs])
        from . import ops
        return ops.stain_fit(img, stride=self.stride, **self.kw)

    def __call__(self, img, out=None):
        if self.host:
            img = np.asarray(img)
            imgs = img[None] if img.ndim == 3 else img
            res = np.stack([host_apply(i, b, self.target_host, io=self.kw['io']) for i, b in zip(imgs, self.fit(imgs))])
            return res[0] if img.ndim == 3 else res
        from . import ops
        return ops.stain_apply(img, self.fit(img), self.target, keep_residual=0.0, io=self.kw['io'], out=out)


def stain_jitter(img, params, host=False, stride=None, io=IO, alpha=ALPHA, beta=BETA, min_tissue=MIN_TISSUE, out=None):
    """Scales and shifts the image's own stain concentrations: params (B, 4) or (4,) = {a_H, b_H, a_E, b_E}, c' = c a + b, residual
    kept.  (1, 0, 1, 0) returns the image bit for bit.  Device tensors in and out unless ``host``."""
    kw = dict(io=io, alpha=alpha, beta=beta, min_tissue=min_tissue)
    if host:
        img = np.asarray(img)
        imgs = img[None] if img.ndim == 3 else img
        par = np.broadcast_to(np.asarray(params, dtype=np.float64).reshape(-1, 4), (len(imgs), 4))
        res = []
        for i, p in zip(imgs, par):
            f = host_fit(i, 1 if stride is None else stride, **kw)
            res.append(host_apply(i, f, f, jitter=p, keep_residual=1.0, io=io))
        res = np.stack(res)
        return res[0] if img.ndim == 3 else res
    import torch
    from . import ops
    B = 1 if img.dim() == 3 else img.shape[0]
    if not _is_tensor(params):
        params = torch.tensor(np.broadcast_to(np.asarray(params, dtype=np.float32).reshape(-1, 4), (B, 4)).copy(), device=img.device)
    blocks = ops.stain_fit(img, stride=stride, **kw)
    return ops.stain_apply(img, blocks, blocks, jitter=params.reshape(B, 4).contiguous(), keep_residual=1.0, io=io, out=out)


def make_normalizer(spec, device):
    """What the tools' ``--stain-normalize [TARGET]`` hands over: None (off), True or '' (the default target), or a path."""
    if spec is None or spec is False:
        return None
    if isinstance(spec, StainNormalizer):
        return spec
    return StainNormalizer(None if spec is True or spec == '' else spec, device=device)


def add_argument(ap):
    """``--stain-normalize [TARGET]``: off by default; without a value the default target, with one an image to fit."""
    ap.add_argument('--stain-normalize', nargs='?', const=True, default=None, metavar='TARGET',
                    help='Macenko stain normalisation in front of the model (optional: an image whose stains are the target)')


# ---------------------------------------------------------------- the program
def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Write Macenko-normalised PNGs of every image in SRC_DIR to OUT_DIR.')
    ap.add_argument('src_dir')
    ap.add_argument('out_dir')
    ap.add_argument('--target', default=None, help='an image whose stains are the target (default: the target in common use)')
    ap.add_argument('--host', action='store_true', help='numpy on the CPU instead of the device path')
    ap.add_argument('--device', default='cuda:0')
    return ap.parse_args(argv)


def run(a):
    from PIL import Image
    norm = StainNormalizer(a.target, device=a.device, host=a.host)
    out_dir = Path(a.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    paths = sorted(p for p in Path(a.src_dir).iterdir() if p.suffix.lower() in IMAGE_SUFFIXES)
    for p in paths:
        img = read_image(p)
        if a.host:
            res = norm(img)
        else:
            import torch
            res = norm(torch.from_numpy(img).to(norm.device)).cpu().numpy()
        Image.fromarray(res).save(out_dir / f'{p.stem}.png')
    return len(paths)


def main(argv=None):
    a = parse_args(argv)
    print(f'{run(a)} image(s) written to {a.out_dir}')


if __name__ == '__main__':
    main()
