"""tests/_poolref.py -- the fp64 reference tests/test_pooling_branches_gpu.py holds the pooling and upsampling kernels to -- against
independent statements of the same map (no GPU), the label maps of tests/_poolcases.py against the kernel branch each is built
to force, and the honest-fp32 figures of the whole case list: every figure is recorded (tests/_tol.py) and must lie below the
cap of its class -- a case whose plain fp32 evaluation already breaks the cap has unsuitable inputs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _poolcases as pc
import _poolref as pr
from _tol import within


def _case(name, h, w, C, seed=0):
    m = pc.label_map(name)
    _, H, W = m['labels'].shape
    new_row, area, K = pc.rows(name)[0]
    s = pr.relu_like(seed, (h, w, C)).double().numpy()
    return m, H, W, new_row, area, K, s


# one odd and one 2-mod-4 shape of SHAPES in tests/test_multiscale_gpu.py, a non-integer ratio and the native grid of each
@pytest.mark.parametrize('name,h,w', [('ms197', 49, 73), ('ms197', 197, 293), ('ms182', 45, 67), ('ms182', 182, 271), ('ms182', 1, 5)])
def test_forward_is_interpolate_then_the_oracles_pooling_in_float64(name, h, w):
    from oracle import wesup_oracle as orc
    m, H, W, new_row, area, K, s = _case(name, h, w, 8, seed=1)
    assert (H % 2 == 1) if name == 'ms197' else (H % 4 == 2)
    up = F.interpolate(torch.from_numpy(s).permute(2, 0, 1)[None], (H, W), mode='bilinear', align_corners=True)[0]
    # (pool_labelmap rounds 1 / area to float32 whatever it is given: it is handed unit areas -- 1 / 1 is exact -- and the float64
    # division is done here)
    ref = orc.pool_labelmap(up.reshape(8, H * W), torch.from_numpy(new_row), torch.ones(K), K) / torch.from_numpy(area).double()[:, None]
    assert ref.dtype == torch.float64
    got, scale = pr.forward(s, new_row, area, H, W)
    assert np.abs(got - ref.numpy()).max() <= 1e-12 * np.abs(ref.numpy()).max()
    assert np.abs(pr.upsample(s, H, W) - up.permute(1, 2, 0).numpy()).max() <= 1e-12 * np.abs(s).max()
    assert np.all(scale >= np.abs(got).max(axis=1) * (1 - 1e-12))            # sum of |terms| bounds |sum of terms|


@pytest.mark.parametrize('name,h,w', [('ms197', 24, 36), ('ms182', 45, 67), ('vor32', 32, 32), ('vor96', 1, 1), ('lens', 13, 19)])
def test_adjoint_and_matrix_form(name, h, w):
    m, H, W, new_row, area, K, s = _case(name, h, w, 6, seed=2)
    g = pr.relu_like(3, (K, 6), zero_mean=True).double().numpy()
    fwd = pr.forward(s, new_row, area, H, W, with_scale=False)
    ds, dscale = pr.adjoint(g, new_row, area, H, W, h, w)
    lhs, rhs = float((fwd * g).sum()), float((s * ds).sum())                     # <Wm s, g> = <s, Wm^T g>
    assert abs(lhs - rhs) <= 1e-12 * float((np.abs(fwd) * np.abs(g)).sum())
    Wm = pr.dense_wm(new_row, area, H, W, h, w)
    assert np.abs(Wm.sum(axis=1) - 1.0).max() <= 1e-12 and Wm.min() >= 0.0      # every row is a mean
    assert np.abs(Wm @ s.reshape(h * w, 6) - fwd).max() <= 1e-12 * np.abs(fwd).max()
    assert np.abs(Wm.T @ g - ds.reshape(h * w, 6)).max() <= 1e-12 * np.abs(ds).max()
    assert np.abs((Wm.T @ np.abs(g)).max(axis=1) - dscale.reshape(-1)).max() <= 1e-12 * dscale.max()


def test_native_resolution_is_the_plain_segment_mean():
    m, H, W, new_row, area, K, s = _case('lens', 128, 128, 5, seed=4)
    got, scale = pr.forward(s, new_row, area, H, W)
    flat = s.reshape(H * W, 5)
    for r in list(range(0, K, 7)) + [int(new_row[p]) for p in m['probe'].values()]:
        assert np.abs(got[r] - flat[new_row == r].mean(axis=0)).max() <= 1e-12
        assert abs(scale[r] - np.abs(flat[new_row == r]).mean(axis=0).max()) <= 1e-12
    A = pr.axis_weights(128, 128)
    assert np.array_equal(A, np.eye(128))
    assert np.array_equal(pr.axis_weights(7, 1), np.ones((7, 1))) and np.array_equal(pr.axis_weights(1, 1), np.ones((1, 1)))
    i0, i1, l0, l1 = pr.axis_taps(9, 3)                          # source positions 0, .25, ... 2: the upper index clamps at the end
    assert i0.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2] and i1.tolist() == [1, 1, 1, 1, 2, 2, 2, 2, 2] and l1[8] == 0.0 and l1[1] == 0.25


def test_both_measures_see_a_dropped_pixel_in_the_largest_row():
    """One pixel dropped from the 7396-pixel row of the skewed map, zero-mean and offset data: both measures land an order of
    magnitude above the cap of the fused forms (the bars derived from the fp32 figures are lower still)."""
    name = 'skew'
    m = pc.label_map(name)
    _, H, W = m['labels'].shape
    new_row, area, K = pc.rows(name)[0]
    s = pr.relu_like(5, (H, W, 4), zero_mean=True).double().numpy()
    ref, scale = pr.forward(s, new_row, area, H, W)
    r = int(np.argmax(area))
    assert area[r] > 5000
    bad = ref.copy()
    p = np.flatnonzero(new_row == r)[-1]
    bad[r] -= s.reshape(H * W, 4)[p] / area[r]
    whole, per_row = pr.measures(bad, ref, scale)
    assert per_row > 1e-4 and whole > 1e-4 and 1e-4 >= 10 * pr.CAP_FUSED
    assert pr.measures(ref, ref, scale) == (0.0, 0.0)
    off = pr.relu_like(5, (H, W, 4)).double().numpy()             # offset data: a dropped pixel shifts the mean by ~1/area
    ref, scale = pr.forward(off, new_row, area, H, W)
    bad = ref.copy()
    bad[r] -= off.reshape(H * W, 4)[p] / area[r]
    assert pr.measures(bad, ref, scale)[1] > 0.5 / area[r] > 5 * pr.CAP_FUSED
    with pytest.raises(AssertionError):
        pr.measures(ref[:, :2], ref, scale)
    assert pr.bar_from(1e-6, pr.CAP_FUSED) == 4e-6 and pr.bar_from(5e-6, pr.CAP_FUSED) == pr.CAP_FUSED


# ---------------------------------------------------------------- the maps take the branch they are built for
def _pixel_lists(name):
    m = pc.label_map(name)
    new_row, area, K = pc.rows(name)[0]
    order = np.argsort(new_row, kind='stable')
    starts = np.concatenate([[0], np.cumsum(area)])
    return m, new_row, area, [order[starts[r]:starts[r + 1]] for r in range(K)]


def test_lengths_map_has_the_rows_it_promises():
    m, new_row, area, lists = _pixel_lists('lens')
    assert m['Kmax'] == m['n'] and pc.label_map('lensP')['Kmax'] == m['n'] + 7
    for n, p in m['probe'].items():
        r = int(new_row[p])
        assert area[r] == n == len(lists[r])
        segs = pr.segments(n)
        assert len(segs) == (n + 511) // 512 and segs[-1][1] == n
        assert (segs[-1][1] - segs[-1][0]) % 64 == n % 64 if n % 512 else True
    assert {n: len(pr.segments(n)) for n in pr.LENGTHS} == {1: 1, 63: 1, 64: 1, 65: 1, 511: 1, 512: 1, 513: 2, 1025: 3}
    assert pr.segments(513)[1] == (512, 513) and pr.segments(1025)[2] == (1024, 1025)       # a second / third segment of one pixel


def test_box_and_diagonal_maps_lie_on_the_side_of_the_cell_capacity_they_claim():
    for name, rows_cells in (('box32', 32), ('box33', 33)):
        m, new_row, area, lists = _pixel_lists(name)
        r = int(new_row[m['probe']['box']])
        boxes = pr.segment_boxes(lists[r], 128, 128, 64, 64)
        assert boxes == [(rows_cells, 32)] and area[r] <= 512
    assert 32 * 32 == pr.SP_CELL_CAP < 33 * 32
    m, new_row, area, lists = _pixel_lists('diag')
    r = int(new_row[m['probe']['diag']])
    assert area[r] == 100
    (bh, bw), = pr.segment_boxes(lists[r], 128, 128, 64, 64)
    assert bh * bw > 2 * pr.SP_CELL_CAP
    # every other row of these maps fits: the fallback is taken by the constructed superpixel alone
    for rr, lst in enumerate(lists):
        if rr != r:
            assert all(a * b <= pr.SP_CELL_CAP for a, b in pr.segment_boxes(lst, 128, 128, 64, 64))
    m, new_row, area, lists = _pixel_lists('skew')
    assert area.max() == 7396 and sorted(len(pr.segments(a)) for a in area)[-1] == 15


def test_lerp_f32_is_the_float32_rule():
    i0, i1 = pr.lerp_f32(np.arange(480), 480, 120)
    j0, j1, _, _ = pr.axis_taps(480, 120)
    assert np.abs(i0 - j0).max() <= 1 and i0[0] == 0 and i1[-1] == 119 and i0[-1] in (118, 119)
    i0, i1 = pr.lerp_f32(np.arange(5), 5, 1)
    assert i0.tolist() == [0] * 5 == i1.tolist()


# ---------------------------------------------------------------- the honest fp32 figures of the case list
@pytest.mark.parametrize('i', range(len(pc.FWD)), ids=[pc.fwd_id(c) for c in pc.FWD])
def test_fp32_cpu_figure_of_every_forward_case_is_below_the_cap(i):
    c = pc.FWD[i]
    for b, (ref, scale, f_whole, f_row) in enumerate(pc.fwd_reference(i, c)):
        cls = pc.map_class(c[0])
        assert within(f'{pc.fwd_id(c)}[{b}]', f'pooling fwd, fp32 on the CPU vs fp64, whole tensor ({cls})', f_whole, pr.CAP_FUSED)
        assert within(f'{pc.fwd_id(c)}[{b}]', f'pooling fwd, fp32 on the CPU vs fp64, per row ({cls})', f_row, pr.CAP_FUSED)


@pytest.mark.parametrize('i', range(len(pc.BWD)), ids=[pc.bwd_id(c) for c in pc.BWD])
def test_fp32_cpu_figure_of_every_backward_case_is_below_the_cap(i):
    c = pc.BWD[i]
    for b, (ref, scale, f_whole, f_row) in enumerate(pc.bwd_reference(i, c)):
        assert within(f'{pc.bwd_id(c)}[{b}]', f'pooling bwd, fp32 on the CPU vs fp64, whole tensor ({c[0]})', f_whole, pc.bwd_cap(c))
        assert within(f'{pc.bwd_id(c)}[{b}]', f'pooling bwd, fp32 on the CPU vs fp64, per cell ({c[0]})', f_row, pc.bwd_cap(c))


def test_wide_and_strided_cases_share_their_data():
    iw, i_s = [i for i, c in enumerate(pc.BWD) if c[0] in ('wide', 'strided') and c[4] == 512]
    assert torch.equal(pc.bwd_input(iw, pc.BWD[iw]), pc.bwd_input(i_s, pc.BWD[i_s]))
