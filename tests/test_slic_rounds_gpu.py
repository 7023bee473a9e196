"""Every assignment round of wesup_slic against the teacher-forced fp64 reference of tests/_slicref.py, and the connectivity
pass bit for bit on inputs that load its union-find, absorb chains and scan.

``ops.slic(..., max_iter=i, enforce_connectivity=False)`` is deterministic and returns the labels of assignment round i.  The
reference follows the device's trajectory (its centres move to the fp64 mean of the device's members) and performs the exact
assignment of the next round; every label must then be the reference's, unless the pixel is a near tie by the rule of
_slicref.compare (bar _slicref.TAU, derived in tests/test_slicref_cpu.py), and at most _slicref.CAP of the pixels may be."""
import numpy as np
import pytest
import torch

import _slicref as sr

pytestmark = pytest.mark.gpu

ROUNDS = sr.ROUNDS
check_rounds, _device_rounds = sr.check_rounds, sr.device_rounds


@pytest.mark.parametrize('case', sr.CASES, ids=sr.case_id)
def test_every_round_matches_the_forced_reference(case):
    kind, H, W, n_seg, m = case
    img = sr.image(kind, H, W)
    rounds = _device_rounds(img[None], n_seg, m)
    check_rounds(sr.case_id(case), img, n_seg, m, [r[0] for r in rounds])


@pytest.mark.parametrize('case', sr.BATCHES, ids=sr.case_id)
def test_every_round_of_a_mixed_batch(case):
    """Three different images in one call, each against its own reference."""
    kinds, H, W, n_seg, m = case
    imgs = np.stack([sr.image(k, H, W) for k in kinds])
    rounds = _device_rounds(imgs, n_seg, m)
    for b, kind in enumerate(kinds):
        check_rounds(f'{sr.case_id(case)}[{b}:{kind}]', imgs[b], n_seg, m, [r[b] for r in rounds])


def _images(kinds, H, W):
    if kinds == 'const':
        return np.full((1, 3, H, W), 0.5, dtype=np.float32)
    return np.stack([sr.image(k, H, W) for k in ((kinds,) if isinstance(kinds, str) else kinds)])


@pytest.mark.parametrize('kinds,H,W,n_seg,m', [
    ('noise', 96, 128, 1400, 1.0),                      # step 3: thousands of fragments, long left-neighbour absorb chains
    ('noise', 96, 128, 300, 1.0),                       # step 6
    ('const', 128, 128, 1, 40.0),                       # one component of 16384 pixels: every union meets at one root; n == 1
    (('synth', 'region', 'noise'), 96, 128, 60, 10.0),  # per-image offsets of parent, size, target and the block sums
    (('noise', 'dark', 'region'), 96, 128, 1400, 1.0),
    ('synth', 5, 7, 100, 40.0),                         # HW < 1024: one scan block
    ('noise', 5, 7, 1, 40.0),
    ('noise', 50, 21, 30, 20.0),                        # HW just over one scan block
    ('dark', 50, 21, 30, 20.0),
], ids=lambda v: '+'.join(v) if isinstance(v, tuple) else str(v))
def test_connectivity_is_the_restated_pass_exactly(kinds, H, W, n_seg, m):
    from oracle import slic_oracle as so
    from wesup_amd import ops
    t = torch.from_numpy(_images(kinds, H, W)).to('cuda:0')
    km, _ = ops.slic(t, n_seg, m, ROUNDS, enforce_connectivity=False)
    lab, n = ops.slic(t, n_seg, m, ROUNDS)
    lab2, n2 = ops.slic(t, n_seg, m, ROUNDS)
    assert torch.equal(lab, lab2) and torch.equal(n, n2)
    for b in range(t.shape[0]):
        k = km[b].cpu().numpy().astype(np.int64)
        ref_lab, ref_n = so.enforce_connectivity(k, n_seg, 0.5)
        ncomp = int((np.diff(k, axis=0) != 0).sum() + (np.diff(k, axis=1) != 0).sum())
        print(f'image {b}: {len(np.unique(k))} centres used, {ncomp} label edges, {ref_n} superpixels')
        assert int(n[b]) == ref_n, b
        assert np.array_equal(lab[b].cpu().numpy(), ref_lab), b
    if kinds == 'const':
        assert int(n[0]) == 1 and int(lab.max()) == 0
