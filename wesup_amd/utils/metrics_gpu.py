"""The GlaS challenge metrics of ``utils/metrics.py`` with the image processing on the device (csrc/regions.hip).

Only integer tables come back from the GPU -- the component counts, the contingency table of the two labelled maps and the
squared directed Hausdorff distances of the object pairs the metric asks for; the float formulas run on the host in float64
through the same helpers as the CPU path (``detection_f1_from_table``, ``object_dice_from_table``,
``object_hausdorff_from_table``), so the values are equal to the CPU functions', not just close.

Inputs are CUDA tensors or arrays of any integer / bool / float dtype; a pixel is foreground when it is non-zero (GlaS ground
truth is an object-id map).  Function names match the CPU module: ``BaseTrainer.evaluate`` writes the same tracker columns."""
import logging

import numpy as np
import torch

from . import metrics as M
from .. import ops

_log = logging.getLogger(__name__)
_said = set()


def _say_once(key, msg):
    if key not in _said:
        _said.add(key)
        _log.warning(msg)


def _device(*xs):
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    return torch.device('cuda', torch.cuda.current_device())


def _fg(x, device):
    """(H,W) uint8 {0,1} on the device: the non-zero pixels of a tensor / array."""
    t = x if torch.is_tensor(x) else torch.tensor(np.asarray(x))
    t = t.detach().to(device)
    if t.dim() != 2:
        t = t.squeeze()
    if t.dim() != 2:
        raise ValueError(f'expected one (H,W) map, got {tuple(t.shape)}')
    return (t != 0).to(torch.uint8).contiguous()


def label(mask, device=None):
    """8-connected components of the non-zero pixels, numbered 1..n in raster order of the first pixel: (H,W) int32 tensor on
    the device (``utils.metrics.label`` on the host)."""
    return ops.cc_label(_fg(mask, device or _device(mask)), 8, 1)[0]


class _Labelled:
    """Two maps labelled once: label maps, component counts and, when it fits, the contingency table on the host."""

    def __init__(self, S, G):
        dev = _device(S, G)
        self.fS, self.fG = _fg(S, dev), _fg(G, dev)
        if self.fS.shape != self.fG.shape:
            raise ValueError(f'maps of different shapes: {tuple(self.fS.shape)} and {tuple(self.fG.shape)}')
        both, n = ops.cc_label(torch.stack([self.fS, self.fG]), 8, 1)
        self.S, self.G = both[0], both[1]
        self.nS, self.nG = (int(v) for v in n.cpu())
        self.C = None
        if (self.nS + 1) * (self.nG + 1) <= ops.CONTINGENCY_MAX_CELLS:
            table, status = ops.contingency(self.S, self.G, self.nS, self.nG)
            assert int(status.cpu()[0]) == 0
            self.C = table.cpu().numpy().astype(np.int64)
        else:
            _say_once('table', f'a contingency table of {self.nS + 1} x {self.nG + 1} cells is not built on the device: such '
                               'images are scored on the host')

    def host(self):
        return self.fS.cpu().numpy(), self.fG.cpu().numpy()

    def hausdorff_sq(self, pairs):
        """{(s, g): d2} in both directions for the (s, g) pairs."""
        L = ops.LABEL_SORT_MAX_LABELS
        if max(self.nS, self.nG) >= L or len(pairs) > (1 << 22):
            return None
        X, Y = ops.label_sort(self.S, self.nS), ops.label_sort(self.G, self.nG)
        p = torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2)
        sg = p.to(self.S.device).contiguous()
        gs = sg.flip(1).contiguous()
        d_sg = ops.directed_hausdorff_sq(sg, X, Y).cpu().numpy()
        d_gs = ops.directed_hausdorff_sq(gs, Y, X).cpu().numpy()
        assert (d_sg >= 0).all() and (d_gs >= 0).all()
        return ({k: int(v) for k, v in zip(pairs, d_sg)}, {k: int(v) for k, v in zip(pairs, d_gs)})

    def object_hausdorff(self):
        if self.C is not None:
            pairs = M.hausdorff_pairs(self.C)
            d = self.hausdorff_sq(pairs) if pairs else ({}, {})
            if d is not None:
                return M.object_hausdorff_from_table(self.C, *d)
            _say_once('pairs', 'too many objects for the device pixel lists: such images are scored on the host')
        return M.object_hausdorff(*self.host())


def detection_f1(S, G, overlap_threshold=0.5, epsilon=1e-7):
    lab = _Labelled(S, G)
    if lab.C is None:
        return M.detection_f1(*lab.host(), overlap_threshold, epsilon)
    return M.detection_f1_from_table(lab.C, overlap_threshold, epsilon)


def object_dice(S, G):
    lab = _Labelled(S, G)
    return M.object_dice(*lab.host()) if lab.C is None else M.object_dice_from_table(lab.C)


def object_hausdorff(S, G):
    """Object-level Hausdorff distance; ``nan`` when either map is empty (the guard of ``evaluate.score``)."""
    lab = _Labelled(S, G)
    if lab.nS == 0 or lab.nG == 0:
        return float('nan')
    return lab.object_hausdorff()


def hausdorff(S, G):
    """Symmetric Hausdorff distance between the non-zero pixels of two masks: 0 when both are empty, inf when one is."""
    dev = _device(S, G)
    fS, fG = _fg(S, dev), _fg(G, dev)
    X, Y = ops.label_sort(fS.to(torch.int32), 1), ops.label_sort(fG.to(torch.int32), 1)
    nS, nG = int(X.start[2] - X.start[1]), int(Y.start[2] - Y.start[1])
    if nS == 0 and nG == 0:
        return 0
    if nS == 0 or nG == 0:
        return np.inf
    one = torch.ones(1, 2, dtype=torch.int32, device=dev)
    return M.hausdorff_from_sq(int(ops.directed_hausdorff_sq(one, X, Y)[0]), int(ops.directed_hausdorff_sq(one, Y, X)[0]))


def _pixel_sums(S, G, device):
    """#(S == G), sum(S * G), sum(S), sum(G) and the pixel count of the maps AS GIVEN (``utils.metrics.accuracy`` / ``dice`` see
    an object-id ground truth as it is), as exact Python numbers."""
    def dev(x):
        t = x if torch.is_tensor(x) else torch.tensor(np.asarray(x))
        t = t.detach().to(device)
        return t.double() if t.is_floating_point() else t.long()
    s, g = dev(S), dev(G)
    if s.dtype != g.dtype:
        s, g = s.double(), g.double()
    v = torch.stack([(s == g).sum().to(s.dtype), (s * g).sum(), s.sum(), g.sum()]).cpu().tolist()
    return v[0], v[1], v[2], v[3], s.numel()


def challenge_scores(S, G, epsilon=1e-7):
    """Both maps labelled once, one table, one pair list: accuracy, dice and the three object-level metrics of
    ``evaluate.score`` for one image (``object_hausdorff`` is ``nan`` when either map is empty)."""
    lab = _Labelled(S, G)
    eq, inter, sum_s, sum_g, n = _pixel_sums(S, G, lab.S.device)
    out = {'accuracy': eq / n, 'dice': 2 * inter / (sum_g + sum_s + epsilon)}
    if lab.C is None:
        hS, hG = lab.host()
        out['detection_f1'], out['object_dice'] = float(M.detection_f1(hS, hG)), float(M.object_dice(hS, hG))
    else:
        out['detection_f1'] = float(M.detection_f1_from_table(lab.C))
        out['object_dice'] = float(M.object_dice_from_table(lab.C))
    out['object_hausdorff'] = float(lab.object_hausdorff()) if lab.nS and lab.nG else float('nan')
    return out
