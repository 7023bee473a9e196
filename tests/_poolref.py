"""fp64 reference of the linear map "bilinear upsample (align_corners=True) of a side output s (h, w, C) to (H, W), then the
mean over every superpixel", of its adjoint and of its matrix form -- the anchor the pooling / upsampling kernels are held to
in tests/test_pooling_branches_gpu.py.  Plain numpy / torch float64; nothing of wesup_amd is imported except synth for the
label maps, and oracle.wesup_oracle.preprocess_superpixels gives the row order (labelled ids ascending, then unlabelled).

    pooled[r, c] = (1 / area_r) * sum_{p in row r} up(s)[p, c]            forward()
    ds[q, c]     = sum_r Wm[r, q] * g[r, c]                               adjoint() = up_adjoint(pool_bwd())
    Wm[r, q]     = (1 / area_r) * sum_{p in row r} wy(p, q) * wx(p, q)    dense_wm(), grids of h * w <= 8192 cells

Both measures of section "The measure" of the module under test are here (measures()): the suite's whole-tensor norm and a
per-row (per-cell for the adjoint) forward-error measure whose scale is the sum of the absolute terms of that row; so is the
"honest fp32" evaluation on the CPU whose distance from fp64 sets the bars (fp32_forward / fp32_adjoint).  tests/test_poolref_cpu.py
holds all of it to independent statements.  The builders of the label maps that force a kernel branch, and the host-side
restatement of the kernels' branch rules (segments of 512 list entries, the box of a segment on the coarse grid), are here too so
that the CPU test can check them without a GPU."""
import numpy as np
import torch
import torch.nn.functional as F

SP_SEG = 512            # pixels per pooling segment (csrc/superpixel.hip)
SP_CELL_CAP = 1024      # cells of a segment's box the cell-wise branch keeps
CAP_FUSED = 1e-5        # what test_sp_pool already demands of the fused forms against the unfused kernels
CAP_POOL = 1e-4         # TOL of tests/test_kernels_gpu.py (sp_pool_fwd / sp_pool_bwd against the oracle)
CHUNK = 64              # channels per pass: a 480 x 480 map in fp64 is 118 MB per 64 channels


# ---------------------------------------------------------------- the map
def axis_taps(H, h):
    """Bilinear align_corners=True taps of an axis: (i0, i1, l0, l1), each (H,).  The source position is dst * (h - 1) / (H - 1)
    in float64 (0 when H == 1); i0 = min(floor(src), h - 1), i1 = i0 + (i0 < h - 1), l1 = src - i0 (torch's rule)."""
    dst = np.arange(H, dtype=np.float64)
    src = dst * (float(h - 1) / float(H - 1)) if H > 1 else np.zeros(H)
    i0 = np.minimum(np.floor(src).astype(np.int64), h - 1)
    i1 = i0 + (i0 < h - 1)
    l1 = np.clip(src - i0, 0.0, 1.0)
    return i0, i1, 1.0 - l1, l1


def axis_weights(H, h):
    """The same as a dense (H, h) float64 matrix."""
    i0, i1, l0, l1 = axis_taps(H, h)
    A = np.zeros((H, h))
    np.add.at(A, (np.arange(H), i0), l0)
    np.add.at(A, (np.arange(H), i1), l1)
    return A


def rows_of(labels, mask=None):
    """(new_row (HW,) int64, area_new (K,) int64, K) of one (H, W) label map in the reference's row order."""
    from oracle import wesup_oracle as orc
    pp = orc.preprocess_superpixels(torch.from_numpy(np.asarray(labels)).long(),
                                    None if mask is None else torch.from_numpy(np.asarray(mask)).long())
    new_row = pp['inv_perm'][torch.from_numpy(np.asarray(labels)).long().reshape(-1)].numpy()
    return new_row, pp['area'][pp['perm']].numpy(), pp['K']


def upsample(s, H, W):
    """s (h, w, C) float64 -> (H, W, C)."""
    s = np.asarray(s, dtype=np.float64)
    h, w, C = s.shape
    t = axis_weights(H, h) @ s.reshape(h, w * C)                            # (H, w*C)
    return np.einsum('Xw,YwC->YXC', axis_weights(W, w), t.reshape(H, w, C), optimize=True)


def _segment_sum(x, order, starts):
    """x (HW, C) summed over the rows' pixels: pixels sorted by row, np.add.reduceat at the row starts."""
    return np.add.reduceat(x[order], starts, axis=0)


def forward(s, new_row, area, H, W, with_scale=True):
    """pooled (K, C) float64 and scale (K,) = max_c (1 / area_r) sum_p |up(s)[p, c]|, in chunks of CHUNK channels."""
    s = np.asarray(s, dtype=np.float64)
    K, C = len(area), s.shape[2]
    order = np.argsort(new_row, kind='stable')
    starts = np.concatenate([[0], np.cumsum(area)[:-1]])
    assert int(np.sum(area)) == H * W and np.all(area > 0)
    out = np.empty((K, C))
    scale = np.zeros(K)
    for c0 in range(0, C, CHUNK):
        up = upsample(s[:, :, c0:c0 + CHUNK], H, W).reshape(H * W, -1)
        out[:, c0:c0 + CHUNK] = _segment_sum(up, order, starts) / area[:, None]
        if with_scale:
            scale = np.maximum(scale, (_segment_sum(np.abs(up), order, starts) / area[:, None]).max(axis=1))
    return (out, scale) if with_scale else out


def pool_bwd(g, new_row, area):
    """dfm[p, c] = g[row(p), c] / area[row(p)]: the adjoint of the segment mean.  g (K, C) -> (HW, C)."""
    g = np.asarray(g, dtype=np.float64)
    return (g / area[:, None])[new_row]


def up_adjoint(dfm, H, W, h, w):
    """ds (h, w, C) = Ay^T dfm Ax: the adjoint of upsample().  dfm (HW, C) or (H, W, C)."""
    dfm = np.asarray(dfm, dtype=np.float64).reshape(H, W, -1)
    C = dfm.shape[2]
    t = axis_weights(H, h).T @ dfm.reshape(H, W * C)                        # (h, W*C)
    return np.einsum('Xw,yXC->ywC', axis_weights(W, w), t.reshape(h, W, C), optimize=True)


def adjoint(g, new_row, area, H, W, h, w, with_scale=True):
    """ds (h, w, C) = Wm^T g, and the per-cell scale (h, w) = max_c sum_r Wm[r, q] |g[r, c]| (every weight is >= 0)."""
    g = np.asarray(g, dtype=np.float64)
    C = g.shape[1]
    ds = np.empty((h, w, C))
    scale = np.zeros((h, w))
    for c0 in range(0, C, CHUNK):
        ds[:, :, c0:c0 + CHUNK] = up_adjoint(pool_bwd(g[:, c0:c0 + CHUNK], new_row, area), H, W, h, w)
        if with_scale:
            scale = np.maximum(scale, up_adjoint(pool_bwd(np.abs(g[:, c0:c0 + CHUNK]), new_row, area), H, W, h, w).max(axis=2))
    return (ds, scale) if with_scale else ds


def dense_wm(new_row, area, H, W, h, w):
    """Wm (K, h*w) float64, built tap by tap (four scatter-adds), not from the dense axis matrices."""
    assert h * w <= 8192
    K = len(area)
    yi0, yi1, yl0, yl1 = axis_taps(H, h)
    xi0, xi1, xl0, xl1 = axis_taps(W, w)
    Y, X = np.divmod(np.arange(H * W), W)
    Wm = np.zeros((K, h * w))
    for (iy, ly) in ((yi0, yl0), (yi1, yl1)):
        for (ix, lx) in ((xi0, xl0), (xi1, xl1)):
            np.add.at(Wm, (new_row, iy[Y] * w + ix[X]), ly[Y] * lx[X])
    return Wm / area[:, None]


# ---------------------------------------------------------------- the honest fp32 evaluation on the CPU
def fp32_forward(s, new_row, area, H, W):
    """F.interpolate in float32, then a float32 segment mean (index_add_ in pixel order and one divide).  s (h, w, C) float32."""
    s = torch.as_tensor(np.asarray(s), dtype=torch.float32)
    up = F.interpolate(s.permute(2, 0, 1)[None], (H, W), mode='bilinear', align_corners=True)[0]
    up = up.permute(1, 2, 0).reshape(H * W, -1)
    out = torch.zeros(len(area), up.shape[1], dtype=torch.float32)
    out.index_add_(0, torch.from_numpy(new_row), up)
    return (out / torch.from_numpy(area).float()[:, None]).numpy()


def fp32_adjoint(g, new_row, area, H, W, h, w):
    """torch's float32 autograd of fp32_forward: ds (h, w, C)."""
    g = torch.as_tensor(np.asarray(g), dtype=torch.float32)
    s = torch.zeros(h, w, g.shape[1], dtype=torch.float32, requires_grad=True)
    up = F.interpolate(s.permute(2, 0, 1)[None], (H, W), mode='bilinear', align_corners=True)[0]
    up = up.permute(1, 2, 0).reshape(H * W, -1)
    out = torch.zeros(len(area), up.shape[1], dtype=torch.float32).index_add(0, torch.from_numpy(new_row), up)
    (out / torch.from_numpy(area).float()[:, None]).backward(g)
    return s.grad.numpy()


def fp32_up_adjoint(dfm, H, W, h, w):
    """float32 autograd of F.interpolate alone: dfm (H, W, C) -> ds (h, w, C)."""
    dfm = torch.as_tensor(np.asarray(dfm), dtype=torch.float32).reshape(H, W, -1)
    s = torch.zeros(h, w, dfm.shape[2], dtype=torch.float32, requires_grad=True)
    F.interpolate(s.permute(2, 0, 1)[None], (H, W), mode='bilinear', align_corners=True)[0].backward(dfm.permute(2, 0, 1))
    return s.grad.numpy()


def fp32_pool_bwd(g, new_row, area):
    """float32 autograd of the segment mean: g (K, C) -> dfm (HW, C)."""
    g = torch.as_tensor(np.asarray(g), dtype=torch.float32)
    x = torch.zeros(len(new_row), g.shape[1], dtype=torch.float32, requires_grad=True)
    out = torch.zeros(len(area), g.shape[1], dtype=torch.float32).index_add(0, torch.from_numpy(new_row), x)
    (out / torch.from_numpy(area).float()[:, None]).backward(g)
    return x.grad.numpy()


# ---------------------------------------------------------------- the two measures and the bar
def measures(got, ref, scale):
    """(whole, per_row): max |got - ref| / max |ref|  and  max over rows r, channels c of |got - ref|[r, c] / scale_r.
    ``ref`` is (..., C) and ``scale`` has ref's leading shape; a row of scale 0 (all its terms are 0) must be met exactly."""
    got, ref, scale = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    assert got.shape == ref.shape and scale.shape == ref.shape[:-1], (got.shape, ref.shape, scale.shape)
    err = np.abs(got - ref)
    whole = float(err.max() / (np.abs(ref).max() + 1e-300))
    row_err = err.max(axis=-1)
    zero = scale == 0.0
    assert not np.any(row_err[zero] > 0.0), 'a row whose terms are all zero is not zero'
    per_row = float((row_err[~zero] / scale[~zero]).max()) if np.any(~zero) else 0.0
    return whole, per_row


def bar_from(fp32_figure, cap):
    """4 x the honest fp32 figure of the same case and measure, never above the suite's existing bar for that class."""
    return min(4.0 * float(fp32_figure), float(cap))


def relu_like(seed, shape, zero_mean=False):
    """|N(0, 1)| plus a per-channel offset in [0.5, 2.5) (side outputs are not zero-mean); zero_mean: N(0, 1), for cancellation."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    if zero_mean:
        return x.float()
    return (x.abs() + 0.5 + 2.0 * torch.rand(shape[-1], generator=g)).float()


# ---------------------------------------------------------------- the kernels' branch rules, restated on the host
def segments(area_row):
    """[(j0, j1)] list positions of the <= 512-entry segments of a row of ``area_row`` pixels, relative to its row start."""
    return [(j, min(area_row, j + SP_SEG)) for j in range(0, max(area_row, 1), SP_SEG)]


def lerp_f32(dst, H, h):
    """i0, i1 of lerp2_of / lerp_of, with the kernels' float32 arithmetic: scale = (float)(h-1) / (float)(H-1); src = scale * dst."""
    scale = np.float32(h - 1) / np.float32(H - 1) if H > 1 else np.float32(0)
    src = scale * np.asarray(dst).astype(np.float32)
    assert src.dtype == np.float32
    i0 = np.minimum(src.astype(np.int64), h - 1)
    return i0, i0 + (i0 < h - 1)


def segment_boxes(pix_row, W, H, h, w):
    """[(box height, box width)] in cells of the (h, w) grid, one per segment of a row's ascending pixel list ``pix_row``."""
    out = []
    for (j0, j1) in segments(len(pix_row)):
        p = np.asarray(pix_row[j0:j1])
        Y, X = np.divmod(p, W)
        y0, y1 = lerp_f32(Y, H, h)
        x0, x1 = lerp_f32(X, W, w)
        out.append((int(y1.max() - y0.min() + 1), int(x1.max() - x0.min() + 1)))
    return out


# ---------------------------------------------------------------- label maps that force a branch
LENGTHS = (1, 63, 64, 65, 511, 512, 513, 1025)


def _renumber(lab):
    _, inv = np.unique(lab, return_inverse=True)
    return inv.reshape(lab.shape).astype(np.int32)


def lengths_map(seed=3, H=128, W=128, g=8):
    """Voronoi background with one superpixel of exactly n pixels for every n of LENGTHS, painted as runs of consecutive
    raster pixels from row 8 on.  Returns (labels int32 with contiguous ids, {n: one pixel index of that superpixel})."""
    from wesup_amd import synth
    lab = synth.voronoi_labels(seed, H, W, g).astype(np.int64)
    flat = lab.reshape(-1)
    nxt, pos, probe = int(flat.max()) + 1, 8 * W + 5, {}
    for n in LENGTHS:
        flat[pos:pos + n] = nxt
        probe[n] = pos
        nxt += 1
        pos += n + 3
    assert pos < H * W
    return _renumber(lab), probe


def diagonal_map(seed=5, H=128, W=128, g=8, length=100):
    """A one-pixel-wide diagonal superpixel of ``length`` pixels over a Voronoi background: (labels, a pixel of it)."""
    from wesup_amd import synth
    lab = synth.voronoi_labels(seed, H, W, g).astype(np.int64)
    k = np.arange(length)
    lab[10 + k, 14 + k] = int(lab.max()) + 1
    return _renumber(lab), 10 * W + 14


def corner_map(H, W, h, w, rows_cells, cols_cells, seed=6, g=8, y_start=9, x_start=11):
    """A superpixel made of one horizontal and one vertical one-pixel run that share a corner (fewer than 512 pixels: one
    segment), whose box on the (h, w) grid is exactly rows_cells x cols_cells cells under the kernels' clamp rule.
    Returns (labels, a pixel of it)."""
    from wesup_amd import synth
    lab = synth.voronoi_labels(seed, H, W, g).astype(np.int64)

    def run_for(start, n_full, n_coarse, cells):
        for L in range(1, n_full - start):
            i0, i1 = lerp_f32(np.arange(start, start + L), n_full, n_coarse)
            if int(i1.max() - i0.min() + 1) == cells:
                return L
        raise AssertionError('no run gives that many cells')
    Ly, Lx = run_for(y_start, H, h, rows_cells), run_for(x_start, W, w, cols_cells)
    assert Ly + Lx - 1 <= SP_SEG
    new = int(lab.max()) + 1
    lab[y_start:y_start + Ly, x_start] = new
    lab[y_start, x_start:x_start + Lx] = new
    return _renumber(lab), y_start * W + x_start
