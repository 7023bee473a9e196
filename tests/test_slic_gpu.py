"""GPU SLIC against the numpy restatement in oracle/slic_oracle.py and through
size-independent properties.  Parity with skimage is unpinned (third-party, absent); what is pinned here is the
algorithm as restated, the integer connectivity pass bit-exactly, and segmentation quality on synthetic regions."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _region_image(seed, H, W, g):
    """Piecewise-constant colour image over a Voronoi tessellation + mild noise; returns (img (3,H,W), regions)."""
    from wesup_amd import synth
    reg = synth.voronoi_labels(seed, H, W, g)
    rs = np.random.RandomState(seed)
    cols = rs.rand(g * g, 3).astype(np.float32) * 0.8 + 0.1
    img = cols[reg].transpose(2, 0, 1) + rs.randn(3, H, W).astype(np.float32) * 0.01
    return np.clip(img, 0, 1).astype(np.float32), reg


@pytest.mark.parametrize('H,W,n_seg', [(96, 128, 60), (120, 120, 72), (64, 200, 40)])
def test_slic_matches_restatement(H, W, n_seg):
    from oracle import slic_oracle as so
    from wesup_amd import ops, synth
    d = torch.device('cuda:0')
    img = synth.synth_image(5, H, W)
    t = torch.from_numpy(img)[None].to(d)
    km_gpu, _ = ops.slic(t, n_seg, 40.0, 10, enforce_connectivity=False)
    km_ref = so.kmeans_labels(img, n_seg, 40.0, 10)
    # every round against the fp64 reference forced onto the device's trajectory: only near ties may differ (_slicref.compare)
    import _slicref as sr
    rounds = [r[0] for r in sr.device_rounds(img[None], n_seg, 40.0)]
    n_diff = sr.check_rounds(f'restatement-{H}x{W}-n{n_seg}', img, n_seg, 40.0, rounds)
    assert np.array_equal(rounds[-1].reshape(H, W), km_gpu[0].cpu().numpy())
    # ten unforced rounds: float32 and fp64 agree everywhere on these cases (test_slicref_cpu.test_restatement_cases_have_no_
    # near_tie), so a device that differed from the forced reference in no round is on the oracle's trajectory exactly
    agree = float((km_gpu[0].cpu().numpy() == km_ref).mean())
    print(f'unforced agreement after ten rounds {agree:.6f}, {n_diff} pixels differed from the forced reference')
    assert agree > 0.995, agree
    if n_diff == 0:
        assert agree == 1.0, agree
    lab_gpu, n_gpu = ops.slic(t, n_seg, 40.0, 10)
    # the connectivity pass is integer-exact: apply the restated pass to the GPU's own k-means labels
    ref_lab, ref_n = so.enforce_connectivity(km_gpu[0].cpu().numpy().astype(np.int64), n_seg, 0.5)
    assert int(n_gpu[0]) == ref_n
    assert np.array_equal(lab_gpu[0].cpu().numpy(), ref_lab)
    lab2, n2 = ops.slic(t, n_seg, 40.0, 10)
    assert torch.equal(lab_gpu, lab2) and torch.equal(n_gpu, n2)       # run-to-run identical


def test_slic_connectivity_batch_of_two_over_several_scan_blocks():
    """The renumbering scan (csrc/scan.hpp through slic.hip's own wrappers) with B = 2 and three scan blocks of 1024 per image
    (80 x 32 = 2560 pixels), two different images: a wrong image offset or block offset renumbers one of them wrongly.  The
    integer pass is exact: the restated pass on the GPU's own k-means labels, image by image."""
    from oracle import slic_oracle as so
    from wesup_amd import ops, synth
    H, W, n_seg = 80, 32, 20
    imgs = np.stack([synth.synth_image(5 + b, H, W) for b in range(2)])
    assert not np.array_equal(imgs[0], imgs[1])
    t = torch.from_numpy(imgs).to('cuda:0')
    km, _ = ops.slic(t, n_seg, 40.0, 10, enforce_connectivity=False)
    lab, n = ops.slic(t, n_seg, 40.0, 10)
    for b in range(2):
        ref_lab, ref_n = so.enforce_connectivity(km[b].cpu().numpy().astype(np.int64), n_seg, 0.5)
        first = np.full(ref_n, H * W); np.minimum.at(first, ref_lab.ravel(), np.arange(H * W))
        assert (first >= 1024).any() and (first >= 2048).any(), first      # ids begin in every scan block: all offsets are used
        assert int(n[b]) == ref_n, (b, int(n[b]), ref_n)
        assert np.array_equal(lab[b].cpu().numpy(), ref_lab), b


@pytest.mark.parametrize('H,W,sp_area', [(480, 480, 200), (200, 300, 150)])
def test_slic_properties_and_quality(H, W, sp_area):
    from scipy import ndimage
    from wesup_amd import ops
    d = torch.device('cuda:0')
    B = 2
    imgs, regs = zip(*[_region_image(11 + b, H, W, 6) for b in range(B)])
    t = torch.from_numpy(np.stack(imgs)).to(d)
    n_seg = int(H * W / sp_area)                                      # models/wesup.py:473-474
    labels, n = ops.slic(t, n_seg, 40.0, 10)
    for b in range(B):
        lab = labels[b].cpu().numpy()
        K = int(n[b])
        assert lab.min() == 0 and lab.max() == K - 1 and len(np.unique(lab)) == K      # contiguous 0-based ids
        assert 0.6 * n_seg < K < 1.3 * n_seg
        # every superpixel is one 4-connected component
        ncomp = sum(ndimage.label(lab == v)[1] for v in range(K))
        assert ncomp == K
        areas = np.bincount(lab.ravel())
        min_size = int(0.5 * H * W / n_seg)
        assert (areas < min_size).sum() <= 1                                            # only pixel 0's component may stay small
        # ids are numbered in raster order of first pixel
        first = np.full(K, H * W); np.minimum.at(first, lab.ravel(), np.arange(H * W))
        assert np.all(np.diff(first) > 0)
        # quality: superpixels respect the region boundaries (undersegmentation: pixels outside the majority region)
        reg = regs[b].ravel()
        leak = 0
        for v in range(K):
            r = reg[lab.ravel() == v]
            leak += len(r) - np.bincount(r).max()
        assert leak / (H * W) < 0.03, leak / (H * W)


def test_trainer_uses_gpu_slic_when_no_label_map_is_given():
    from oracle import wesup_oracle as orc
    from wesup_amd import synth
    from wesup_amd.models import initialize_trainer
    from wesup_amd.utils.metrics import accuracy, dice
    d = torch.device('cuda:0')
    trainer = initialize_trainer('wesup', device='cuda:0', sp_area=64)
    trainer.model.load_state_dict({k: torch.from_numpy(v) for k, v in orc.make_weights(1, feat_scale=0.05).items()})
    trainer.optimizer, _ = trainer.get_default_optimizer()
    trainer.metric_funcs = [accuracy, dice]
    trainer.tracker.train()
    H = W = 64
    imgs = np.stack([_region_image(3 + b, H, W, 3)[0] for b in range(2)])
    pix = np.stack([synth.pixel_mask(b, H, W) for b in range(2)])
    pts = np.zeros((2, 2, H, W), dtype=np.int64)
    pts[:, 0, 10::16, 10::16] = 1
    pts[:, 1, 4::16, 6::16] = 1
    # the reference's own call signature: (img, pixel_mask, point_mask) and nothing else
    trainer.train_one_iteration('train', torch.from_numpy(imgs).to(d), torch.from_numpy(pix).long().to(d),
                                torch.from_numpy(pts).to(d))
    h = trainer.tracker.history
    assert np.isfinite(h['loss'][0]) and h['loss'][0] > 0 and 0 < h['labeled_sp_ratio'][0] < 1
    meta = trainer.model._last_meta
    meta.check()
    assert int(meta.n_sp.min()) > 20
