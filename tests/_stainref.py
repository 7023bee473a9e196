"""numpy restatement of the stain definition: Macenko's fit and the per-pixel apply, stage by stage, in the
``dtype`` it is given -- float64 is the reference of the device path and of the host path of wesup_amd.stain, float32 measures
what "the same thing in single precision" costs, which is what the device stages are held to (four times that error).

Departures from the scripts in common use, on purpose: the output is rint(clamp(Io exp(-OD') - 1, 0, 255)) -- no ``+ 1`` left in the
output, no clamp at 254 -- so that OD and its inverse are each other's inverse on uint8 and the identity returns the image; the
percentiles interpolate linearly as numpy's default does; maxC is taken over all sampled pixels."""
import numpy as np

IO, ALPHA, BETA, MIN_TISSUE = 240.0, 1.0, 0.15, 16
PARALLEL_DET = 1e-6            # |det(HE^T HE)| = sin^2 of the angle between the two stain vectors
MIN_MAXC = 1e-6
TARGET_HE = np.array([[0.5626, 0.2159], [0.7201, 0.8012], [0.4062, 0.5581]])
TARGET_MAXC = np.array([1.9705, 1.0308])
BLOCK = 16


def od_table(io=IO, dtype=np.float64):
    """OD of the 256 values of a uint8 channel: computed in float64, rounded once."""
    return (-np.log((np.arange(256, dtype=np.float64) + 1.0) / float(io))).astype(dtype)


def sample(img, stride=1):
    """The lattice of every stride-th row and column, as rows of pixels."""
    return np.ascontiguousarray(img[::stride, ::stride]).reshape(-1, 3)


def tissue_mask(od, beta=BETA):
    return (od >= od.dtype.type(beta)).all(1)


def moments(od_tissue):
    """{n, sum r g b, sum rr rg rb gg gb bb} of the tissue OD, in its dtype."""
    r, g, b = od_tissue[:, 0], od_tissue[:, 1], od_tissue[:, 2]
    dt = od_tissue.dtype
    return np.array([len(od_tissue), r.sum(), g.sum(), b.sum(), (r * r).sum(), (r * g).sum(), (r * b).sum(), (g * g).sum(),
                     (g * b).sum(), (b * b).sum()], dtype=dt)


def cov_from_moments(m):
    n = m[0]
    mean = m[1:4] / n
    s2 = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]], dtype=m.dtype)
    return (s2 - n * np.outer(mean, mean)) / (n - 1)


def eigvecs(cov):
    """The two leading eigenvectors as columns (3, 2): the first with a non-negative component sum, the second with its largest
    component positive (its sign does not reach the stain vectors: phi and the percentiles mirror with it)."""
    w, v = np.linalg.eigh(cov)
    v = v[:, ::-1][:, :2].copy()
    if v[:, 0].sum() < 0:
        v[:, 0] = -v[:, 0]
    if v[np.argmax(np.abs(v[:, 1])), 1] < 0:
        v[:, 1] = -v[:, 1]
    return v


def ranks(q, n):
    """Order statistics floor(q (n - 1) / 100) and the next, and the weight of the second."""
    pos = float(q) * float(n - 1) / 100.0
    lo = int(np.floor(pos))
    lo = min(max(lo, 0), n - 1)
    return lo, min(lo + 1, n - 1), pos - np.floor(pos)


def percentile(a, q):
    """numpy's default (linear) percentile, restated: a[lo] + (a[hi] - a[lo]) * frac on the sorted array, in a's dtype."""
    s = np.sort(a)
    lo, hi, frac = ranks(q, len(s))
    return s[lo] + (s[hi] - s[lo]) * s.dtype.type(frac)


def phi(od_tissue, v):
    t = od_tissue @ v.astype(od_tissue.dtype)
    return np.arctan2(t[:, 1], t[:, 0])


def stain_vectors(phi_lo, phi_hi, v):
    """V (cos phi, sin phi) at both angles; the vector with the larger red component is column 0 ("H")."""
    dt = v.dtype
    a = v @ np.array([np.cos(phi_lo), np.sin(phi_lo)], dtype=dt)
    c = v @ np.array([np.cos(phi_hi), np.sin(phi_hi)], dtype=dt)
    return np.stack([a, c], 1) if a[0] > c[0] else np.stack([c, a], 1)


def gram_det(he):
    g = he.T @ he
    return g[0, 0] * g[1, 1] - g[0, 1] * g[1, 0]


def pinv(he):
    """(HE^T HE)^-1 HE^T (2, 3)."""
    g = he.T @ he
    det = g[0, 0] * g[1, 1] - g[0, 1] * g[1, 0]
    inv = np.array([[g[1, 1], -g[0, 1]], [-g[1, 0], g[0, 0]]], dtype=he.dtype) / det
    return inv @ he.T


def concentrations(od_all, pv):
    return od_all @ pv.astype(od_all.dtype).T            # (n, 2)


def invalid(n_tissue=0):
    return dict(HE=np.zeros((3, 2)), pinv=np.zeros((2, 3)), maxC=np.zeros(2), n_tissue=int(n_tissue), valid=False)


def fit(img, stride=1, io=IO, alpha=ALPHA, beta=BETA, min_tissue=MIN_TISSUE, dtype=np.float64, table=None, stages=False):
    """The fit of one (H, W, 3) uint8 image.  ``table`` replaces the OD table (the device's float32 one, for the stage tests)."""
    dt = np.dtype(dtype).type
    T = od_table(io, dtype) if table is None else np.asarray(table).astype(dtype)
    od = T[sample(img, stride)]
    tis = tissue_mask(od, beta)
    n = int(tis.sum())
    out = invalid(n)
    if n < min_tissue:
        return out
    odt = od[tis]
    cov = np.cov(odt.T).astype(dtype)
    v = eigvecs(cov)
    ph = phi(odt, v)
    he = stain_vectors(percentile(ph, alpha), percentile(ph, 100.0 - alpha), v)
    if stages:
        out.update(moments=moments(odt), eig=v, phi=ph, he_raw=he)
    if not abs(gram_det(he)) >= PARALLEL_DET:
        return out
    pv = pinv(he)
    c = concentrations(od, pv)
    maxc = np.array([percentile(c[:, 0], 99.0), percentile(c[:, 1], 99.0)], dtype=dt)
    if stages:
        out.update(conc=c)
    if not (maxc >= MIN_MAXC).all():
        return out
    out.update(HE=he, pinv=pv, maxC=maxc, valid=True)
    return out


def target(dtype=np.float64):
    he = TARGET_HE.astype(dtype)
    return dict(HE=he, pinv=pinv(he), maxC=TARGET_MAXC.astype(dtype), n_tissue=0, valid=True)


def to_block(f):
    """The 16 floats of the device block."""
    b = np.zeros(BLOCK, np.float32)
    b[14] = f['n_tissue']
    if f['valid']:
        b[0:6] = np.asarray(f['HE']).reshape(-1)
        b[6:12] = np.asarray(f['pinv']).reshape(-1)
        b[12:14] = f['maxC']
        b[15] = 1.0
    return b


def from_block(b, dtype=np.float64):
    b = np.asarray(b)
    return dict(HE=b[0:6].reshape(3, 2).astype(dtype), pinv=b[6:12].reshape(2, 3).astype(dtype), maxC=b[12:14].astype(dtype),
                n_tissue=int(b[14]), valid=bool(b[15] != 0))


def apply_pre(img, src, dst, jitter=(1.0, 0.0, 1.0, 0.0), keep_residual=0.0, io=IO, dtype=np.float64, table=None):
    """Io exp(-OD') - 1 in front of the clamp and the rounding, (H, W, 3) in ``dtype``; None when a fit is invalid (a copy)."""
    if not (src['valid'] and dst['valid']):
        return None
    dt = np.dtype(dtype).type
    T = od_table(io, dtype) if table is None else np.asarray(table).astype(dtype)
    od = T[img.reshape(-1, 3)]
    hs, ps, hd = np.asarray(src['HE']).astype(dtype), np.asarray(src['pinv']).astype(dtype), np.asarray(dst['HE']).astype(dtype)
    ms, md = np.asarray(src['maxC']).astype(dtype), np.asarray(dst['maxC']).astype(dtype)
    j = np.asarray(jitter, dtype=dtype)
    c = od @ ps.T
    c2 = c * (md / ms) * j[[0, 2]] + j[[1, 3]]
    od2 = c2 @ hd.T + dt(keep_residual) * (od - c @ hs.T)
    return (dt(io) * np.exp(-od2) - dt(1)).reshape(img.shape)


def apply(img, src, dst, jitter=(1.0, 0.0, 1.0, 0.0), keep_residual=0.0, io=IO, dtype=np.float64, table=None):
    pre = apply_pre(img, src, dst, jitter, keep_residual, io, dtype, table)
    if pre is None:
        return img.copy()
    return np.rint(np.clip(pre, 0, 255)).astype(np.uint8)


def normalize(img, dst=None, **kw):
    return apply(img, fit(img, **kw), target() if dst is None else dst, keep_residual=0.0, io=kw.get('io', IO),
                 dtype=kw.get('dtype', np.float64))


def jitter(img, params, **kw):
    f = fit(img, **kw)
    return apply(img, f, f, jitter=params, keep_residual=1.0, io=kw.get('io', IO), dtype=kw.get('dtype', np.float64))
