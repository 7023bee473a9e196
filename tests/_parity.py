"""Yardsticks shared by the shard-batch and multi-scale parity tests (tests/test_shards_gpu.py, tests/test_multiscale_gpu.py)
and by the full-size tests' per-slice comparison of the superpixel feature vectors.

  * ``check_sp_slices``: the 2112-wide superpixel input of the fc layers (engine buffer ``sp_in``, oracle ``sp_in``) is 13
    slices written by different layers and kernels (native-resolution gather, coarse gather, matrix GEMM) whose magnitudes
    differ by orders; one max over all 2112 columns lets a small slice be wrong far beyond the bar of its own scale.  Each
    slice is compared against its own max here, and the worst slice is what gets recorded.
  * ``conv3x3_fp64``: one conv layer recomputed in fp64 from the GPU's own input to it (``layer_input``: ReLU and the 2x2
    max-pool of the layer below, both exact in fp32), on a window of outputs with a one-pixel halo and zero padding at the
    border -- a direct pin of every layer of every image of a batch, where the full fp64 oracle does not fit in host memory.
  * ``decision_diffs``: the discrete decisions (ReLU sign of conv and fc units, 2x2 pooling arg-max) on which two runs of
    the same image differ, every one tested for being a near-tie.
All comparisons run on the device the tensors live on; only scalars come back to the host."""
import torch
import torch.nn.functional as F

from oracle import wesup_oracle as orc
import _gradcheck
import _tol

SLICES = [(off, off + co // 2) for off, (_, co) in zip(orc.SIDE_OFF, orc.CONV_CH)]


def slice_errors(got, ref):
    """got, ref: (..., 2112).  max |got - ref| / max |ref| over each layer's slice (13 values)."""
    got = torch.as_tensor(got)
    ref = torch.as_tensor(ref).to(got.device)
    out = []
    for a, b in SLICES:
        r = ref[..., a:b].double()
        out.append(float((got[..., a:b].double() - r).abs().max() / (r.abs().max() + 1e-30)))
    return out


def check_sp_slices(case, cls, got, ref, bar, what=''):
    """Records the worst of the 13 per-slice errors through _tol.within; returns (ok, the 13 errors)."""
    errs = slice_errors(got, ref)
    worst = max(range(len(errs)), key=errs.__getitem__)
    a, b = SLICES[worst]
    ok = _tol.within(case, cls, errs[worst], bar, f'{what}; max |a - b| / max |b| per side-output slice, worst slice recorded '
                     f'(here layer {worst}, columns {a}:{b})')
    return ok, errs


def layer_input(l, img, y_prev):
    """The input of conv layer l as the GPU's forward forms it.  img (3,H,W) for l = 0; else y_prev, the GPU's
    pre-activation of layer l - 1 as (C,h,w): ReLU, then the 2x2 max-pool (floor) where orc.POOL_AFTER[l - 1]."""
    if l == 0:
        return img
    x = torch.relu(y_prev)
    if orc.POOL_AFTER[l - 1]:
        x = F.max_pool2d(x[None], 2, 2)[0]
    return x


def conv3x3_fp64(x, weight, bias, r0, r1, c0, c1):
    """Outputs [r0:r1, c0:c1] of a 3x3, padding-1 convolution of x (C,h,w), in fp64, as the sum of the nine taps'
    products (independent of F.conv2d).  The input window carries a one-pixel halo, zero beyond the border."""
    _, h, w = x.shape
    weight = torch.as_tensor(weight).to(x.device, torch.float64)
    bias = torch.as_tensor(bias).to(x.device, torch.float64)
    xa, xb, ya, yb = max(r0 - 1, 0), min(r1 + 1, h), max(c0 - 1, 0), min(c1 + 1, w)
    xp = F.pad(x[:, xa:xb, ya:yb].double(), (ya - (c0 - 1), (c1 + 1) - yb, xa - (r0 - 1), (r1 + 1) - xb))
    rh, rw = r1 - r0, c1 - c0
    out = bias[:, None].expand(-1, rh * rw).clone()
    for dy in range(3):
        for dx in range(3):
            out += weight[:, :, dy, dx] @ xp[:, dy:dy + rh, dx:dx + rw].reshape(xp.shape[0], -1)
    return out.view(-1, rh, rw)


def windows(h, w, size=16):
    """The four corners and the centre of an (h, w) map as (r0, r1, c0, c1), clipped to the map (the whole map when it is
    smaller than one window).  The bottom-right window holds the ragged Winograd tiles."""
    sh, sw = min(size, h), min(size, w)
    ch, cw = (h - sh) // 2, (w - sw) // 2
    out = []
    for r0, c0 in ((0, 0), (0, w - sw), (h - sh, 0), (h - sh, w - sw), (ch, cw)):
        if (r0, r0 + sh, c0, c0 + sw) not in out:
            out.append((r0, r0 + sh, c0, c0 + sw))
    return out


def check_conv_layers(case, img, ys, weights, bar, full=False, size=16):
    """Every conv layer of ONE image against fp64 from the GPU's own input: img (3,H,W), ys the 13 GPU pre-activations
    (C,h,w) of that image (any device), weights name -> array.  On the corner and centre windows (``full``: the whole layer).
    Returns the 13 worst errors, each relative to the layer's max."""
    worst = []
    for l, idx in enumerate(orc.CONV_IDX):
        y = ys[l]
        x = layer_input(l, img, ys[l - 1] if l else None)
        scale = float(y.abs().max())
        _, h, w = y.shape
        wins = [(0, h, 0, w)] if full else windows(h, w, size)
        e = 0.0
        for r0, r1, c0, c1 in wins:
            ref = conv3x3_fp64(x, weights[f'backbone.{idx}.weight'], weights[f'backbone.{idx}.bias'], r0, r1, c0, c1)
            e = max(e, float((y[:, r0:r1, c0:c1].double() - ref).abs().max()) / scale)
        worst.append(e)
        assert _tol.within(case, 'conv pre-activation vs fp64 conv of the GPU\'s own input (per layer)', e, bar,
                           ('whole layer' if full else f'corner and centre windows of {size}x{size} outputs') +
                           '; max |y - y64| / max |y| of the layer, y64 = fp64 3x3 conv of ReLU (+ 2x2 max-pool) of the GPU\'s '
                           'pre-activation below'), (case, l, e)
    return worst


def decision_diffs(ys, ys_ref, fc, fc_ref, tie_tol=2e-5):
    """Discrete decisions of ONE image that a run (ys: 13 conv pre-activations (C,h,w); fc: the three fc outputs after
    their ReLU, (n, width)) takes differently from a yardstick run of the same image (ys_ref, fc_ref): ReLU sign of every
    conv and fc unit, arg-max of every 2x2 pooling window (first maximum, _gradcheck._windows order).  A differing unit
    is a near-tie when both runs put it within tie_tol x the layer's max of zero (ReLU), resp. when the yardstick's two
    candidates are within tie_tol x the layer's max of each other or the window passes nothing (its max <= 0).
    Returns (count, list of (kind, layer, index) of the differing units that are NOT near-ties, at most 16)."""
    count, bad = 0, []

    def note(kind, layer, diff, near):
        nonlocal count
        count += int(diff.sum())
        far = diff & ~near
        if bool(far.any()) and len(bad) < 16:
            bad.extend((kind, layer, tuple(i)) for i in far.nonzero()[:16 - len(bad)].tolist())

    for l in range(13):
        y, r = ys[l], ys_ref[l].to(ys[l].device)
        scale = float(r.abs().max())
        note('relu', l, (y > 0) != (r > 0), torch.maximum(y.abs(), r.abs()) <= tie_tol * scale)
        if l in _gradcheck.POOLED:
            wy, wr = _gradcheck._windows(y[None]), _gradcheck._windows(r[None])
            pick, own = wy.argmax(dim=-1, keepdim=True), wr.argmax(dim=-1, keepdim=True)
            gap = (wr.gather(-1, pick) - wr.gather(-1, own)).abs()
            dead = wr.max(dim=-1, keepdim=True).values <= 0
            note('pool', l, pick != own, dead | (gap <= tie_tol * scale))
    for k, (h, r) in enumerate(zip(fc, fc_ref)):
        r = r.to(h.device)
        scale = float(r.abs().max())
        note('fc-relu', k, (h > 0) != (r > 0), torch.maximum(h.abs(), r.abs()) <= tie_tol * scale)
    return count, bad


def near_tie_rows(feats, sp_labels, threshold=0.8, tol=1e-5):
    """Unlabelled rows whose propagation is decided within rounding (the definition of test_fullsize_gpu): best
    similarity within tol of the threshold or of the runner-up.  feats (n, D) of one image, sp_labels (n_l, C)."""
    feats = torch.as_tensor(feats).detach().float().cpu()
    _, W_ul, max_sim, src = orc.label_propagate(feats, torch.as_tensor(sp_labels).float().cpu(), threshold, return_aux=True)
    top2 = W_ul.topk(min(2, W_ul.shape[1]), dim=1).values
    return ((max_sim - threshold).abs() < tol) | ((top2[:, 0] - top2[:, -1]).abs() < tol)
