"""Inputs of the stain tests: synthetic H&E images with known stain vectors, random uint8 images, degenerate images."""
import numpy as np

# (Ruifrok & Johnston's haematoxylin and eosin, and a pair turned away from them: another lab's stains)
VEC_A = np.array([[0.650, 0.072], [0.704, 0.990], [0.286, 0.105]])
VEC_B = np.array([[0.550, 0.150], [0.760, 0.900], [0.350, 0.410]])
SHAPES = [(7, 5), (33, 65), (64, 48), (96, 80)]


def he_image(seed, H, W, vectors=VEC_A, noise=1.5):
    """Two gamma-distributed concentrations per pixel, ~30 % near-empty background, 240 exp(-OD) - 1 plus noise, uint8.  The
    draws depend on (seed, H, W) only: two calls with different ``vectors`` differ in their stains and in nothing else."""
    rs = np.random.RandomState(seed)
    v = np.asarray(vectors, dtype=np.float64)
    v = v / np.linalg.norm(v, axis=0)
    c = rs.gamma(2.0, 0.45, size=(H * W, 2))
    c[rs.rand(H * W) < 0.3] *= 0.02
    od = c @ v.T
    val = 240.0 * np.exp(-od) - 1.0 + noise * rs.standard_normal((H * W, 3))
    return np.rint(np.clip(val, 0, 255)).astype(np.uint8).reshape(H, W, 3)


def random_u8(seed, H=64, W=48):
    """Uniform random bytes; every channel holds all 256 values."""
    img = np.random.RandomState(seed).randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    assert all(len(np.unique(img[..., c])) == 256 for c in range(3))
    return img


class RawItems:
    """A dataset of raw items for utils.data.DevicePrefetcher -- (img uint8 (H, W, 3), mask uint8 (H, W), points (P, 3) of x, y,
    class) -- whose images are synthetic H&E (SyntheticGlasDataset hands out float items, which the prefetcher refuses).
    ``images`` replaces the pictures (the pre-normalised, pre-jittered ones of the wiring test)."""

    def __init__(self, n, H, W, images=None):
        self.n, self.H, self.W = n, H, W
        self.images = [he_image(100 + i, H, W, VEC_B if i % 2 else VEC_A) for i in range(n)] if images is None else images

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        import torch
        img = self.images[i]
        mask = (he_image(100 + i, self.H, self.W)[..., 0] < 128).astype(np.uint8)
        rs = np.random.RandomState(i)
        pts = np.stack([rs.randint(0, self.W, 5), rs.randint(0, self.H, 5), rs.randint(0, 2, 5)], 1).astype(np.int64)
        return torch.from_numpy(np.ascontiguousarray(img)), torch.from_numpy(mask), torch.from_numpy(pts)


def degenerate(H=33, W=65):
    """name -> image with no valid fit: empty glass, one colour, a handful of tissue pixels on glass."""
    white = np.full((H, W, 3), 255, np.uint8)
    single = np.empty((H, W, 3), np.uint8)
    single[...] = (150, 90, 170)
    few = white.copy()
    few.reshape(-1, 3)[:9] = he_image(3, 3, 3).reshape(-1, 3).clip(0, 150)
    return {'white': white, 'single': single, 'few': few}
