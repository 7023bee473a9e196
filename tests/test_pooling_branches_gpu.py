"""Every branch of the superpixel pooling / upsampling kernels against an fp64 reference of the same linear map (tests/_poolref.py),
never against another kernel.  The case list is tests/_poolcases.py (FWD, BWD); tests/test_poolref_cpu.py holds the reference and
the label maps to independent statements without a GPU.

Measure and bar.  Per case and image two figures, both recorded through tests/_tol.within: the suite's whole-tensor norm
max |gpu - ref64| / max |ref64|, and the per-row figure max_{r,c} |gpu - ref64|[r, c] / scale_r with scale_r = max_c (1 / area_r)
sum_p |up(s)[p, c]| (per coarse cell for the backward): every row is held to the size of the terms it sums, whatever its area.  The
bar is 4 x the same figure of a plain fp32 evaluation on the CPU of exactly these inputs (F.interpolate in float32, index_add_, one
divide; torch's float32 autograd for the backward), and never above the suite's existing bars: 1e-5 for the fused forms and the
upsample backward, 1e-4 (TOL) for sp_pool_bwd.  The factor 4 covers another legitimate summation order (lane-group tree, 512-pixel
partial sums, per-cell regrouping) and the 2^-40 fixed-point weights; a dropped pixel shifts a mean of offset data by ~1 / area
>= 1e-4.  On the skewed maps (rows of up to 7396 pixels) the sequential fp32 sum on the CPU is itself the noisy part: 4 x its
figure (1.7e-6 ... 4.1e-6) exceeds 1e-5 in most of those cases, and the 1e-5 cap is their bar; it is the bar as well for the
per-cell figure of most coarse-grid backward cases (CPU 1.7e-6 ... 6.7e-6).  Nothing is skipped or masked; every element of every
output is compared, the padded rows and the sentinel regions for their exact content.

Measured on the MI355X (profiles/tolerances_pooling_branches.json has every case, HIP beside fp32-CPU): forward 0.2e-6 ... 1.1e-6 on
the Voronoi, lengths and cell-box maps (CPU 0.5e-6 ... 2.6e-6), <= 2.2e-6 on the skewed maps (CPU <= 4.1e-6: the 512-pixel partial
sums beat the sequential sum); Wm <= 2.3e-6; coarse-grid backward <= 2.4e-6 whole, <= 6.8e-6 per cell; native-resolution backward and
sp_pool_bwd <= 1.1e-7 (a reciprocal and a product, two roundings, against the CPU's one division: 5.6e-8).

Which case covers which branch (ids as pytest prints them; "native" is h == H, the ``ident`` branch):

  sp_pool_up_fwd_kernel<8>  (C = 32)   ident: vor96-native-C32, lens-native-C32 | coarse: vor96-48x48-C32, lensP-64x64-C32, skew-60x50-C32
  sp_pool_up_fwd_kernel<16> (C = 64)   ident: vor96-native-C64, lensP-native-C64, vor480-native-C64 | coarse: vor96-24x24-C64, lens-32x32-C64
  sp_pool_up_fwd_kernel<32> (C = 128)  ident: vor96-native-C128, lens-native-C128, skew-native-C128, ms197-native-C128 | coarse: vor96-12x12-C128,
                                       lensP-16x16-C128, vor480-120x120-C128
  sp_pool_up_fwd_kernel<64> (C = 256)  ident: vor96-native-C256, lensP-native-C256, skew-native-C256, vor240-native-C256 | coarse: vor96-6x6-C256,
                                       lens-8x8-C256, vor480-60x60-C256
  256-channel slab loop     (C = 512)  ident: vor96-native-C512, lens-native-C512 | coarse: vor96-48x48-C512, lensP-64x64-C512, skew-30x25-C512,
                                       vor480-30x30-C512 (H/16), vor240-15x15-C512
  ragged last pass of 64 list entries  lens / lensP native at every width: rows of 1, 63, 65, 511 pixels; 64 and 512 are the full passes
                                       (asserted from area_new / seg_start in test_maps_take_their_branch)
  1-pixel row, 512 / 513 / 1025 pixels lens / lensP: one segment of 512, part + sp_pool_combine_kernel with a last segment of ONE pixel
  rows of many segments (up to 15)     skew-native-C128, skew-native-C256, skew-30x25-C512, skew-120x100-C64-zeromean
  by_cell at its capacity (32x32)      box32-64x64-C64, box32-64x64-C512;  one cell row beyond it (33x32, per-pixel loop): box33-64x64-C64 / -C512
  per-pixel fallback far beyond it     diag-64x64-C128, diag-64x64-C512 (a 100-pixel diagonal: box of 51 x 51 cells)
  an axis of one cell (scale 0)        vor96-1x1-C128, vor96-1x48-C32, vor96-48x1-C64;  non-integer ratios: ms197-*, ms156-39x58-C128
  Kmax == count / padded, batch 2      lens / vor480 / vor240 (equal), lensP / vor96 / ms197 / skew (padded); vor96 is a batch of two images
  channel offset 0 / 32 / 256          the -off suffix; the output is 32 channels wider than coff + C and filled with a sentinel
  sp_interp_matrix                     test_interp_matrix: 60^2 and 30^2 under 480^2, 39x58 under 156x232, 13x19 and 64x128 (= 8192 cells) under
                                       128^2, 24^2 under a batch of two; 8193 and 8320 cells refused
  upsample_bwd_ident_kernel            ident-* (C = 32, 64, 256 strided, 512)
  upsample_bwd_cell_kernel (C <= 256)  cell-*: ratios 2, 4, 16 (vor96-6x6, vor480-30x30), 32 (vor96-3x3, vor480-15x15: windows of > 64 candidates,
                                       several ballot rounds), h = 1 (vor32-1x1, vor96-1x48), non-integer (ms156-39x58, ms156-9x14), strided rows
  wide dense route -> group kernel     wide-vor96-24x24-C512 (NPASS 2), wide-vor96-12x12-C768 (NPASS 3, the limit), wide-vor96-6x6-C320 (half-filled pass)
  upsample_bwd_kernel<true>            strided-vor96-24x24-C512 (the data of the wide case), generic-*-C1024 (C > 768), one of them with h = w = 1
  upsample_bwd_kernel<false>           unfused-*: ratio 2 strided, 16, h = w = 1, non-integer, native
  upsample_bwd_cell_group_kernel<1|2|3>  group-*: (64,) | (128,128), (32,256) | (256,256,256); ratio 32, h = 1, non-integer; 772 channels refused
  sp_pool_bwd_kernel                   pool-*
  maxpool_fwd / maxpool_bwd            test_maxpool_odd_sizes_and_ties
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _poolcases as pc
import _poolref as pr
from _tol import within

pytestmark = pytest.mark.gpu

SENTINEL = -777.25        # fill of the pooled output outside [coff, coff + C): must survive bit for bit


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from wesup_amd import ops as o
    return o


_META = {}


def meta_of(ops, name):
    """sp_preprocess of a map of the case list (its integer outputs are held bit-exact by test_sp_preprocess); the kernels' row
    order must be the reference's, or no row below could be compared."""
    if name not in _META:
        m = pc.label_map(name)
        d = dev()
        meta = ops.sp_preprocess(torch.from_numpy(m['labels']).to(d), torch.from_numpy(m['masks']).to(d), m['Kmax'])
        meta.check()
        for b, (new_row, area, K) in enumerate(pc.rows(name)):
            assert int(meta.n_sp[b]) == K == m['n']
            assert np.array_equal(meta.new_row[b].cpu().numpy(), new_row) and np.array_equal(meta.area_new[b, :K].cpu().numpy(), area)
            assert int(meta.area_new[b, K:].abs().sum()) == 0
        _META[name] = meta
    return _META[name]


def host_lists(meta, b=0):
    """(area_new, segments per row, pixel list per row) of image b, read back from the device tables the kernels walk."""
    K = int(meta.n_sp[b])
    area = meta.area_new[b].cpu().numpy()
    rs = meta.row_start[b].cpu().numpy()
    ss = meta.seg_start[b].cpu().numpy()
    pix = meta.pix_sorted[b].cpu().numpy()
    assert np.array_equal(np.diff(rs)[:K], area[:K])
    return area, np.diff(ss), [pix[rs[r]:rs[r + 1]] for r in range(K)]


def test_maps_take_their_branch(ops):
    """The data-dependent branches, asserted on the host from area_new, seg_start and the pixel lists of the device."""
    # constructed lengths: single against multi segment, ragged last pass of the native-resolution loop
    for name in ('lens', 'lensP'):
        meta = meta_of(ops, name)
        m = pc.label_map(name)
        assert meta.Kmax == m['n'] + (7 if name == 'lensP' else 0)
        area, nseg, lists = host_lists(meta)
        new_row = meta.new_row[0].cpu().numpy()
        seen = {}
        for n, p in m['probe'].items():
            r = int(new_row[p])
            assert area[r] == n == len(lists[r]) and nseg[r] == (n + 511) // 512
            last = n - 512 * (nseg[r] - 1)
            seen[n] = (int(nseg[r]), last, (last + 63) >> 6, last % 64)            # segments, last segment, its passes, ragged entries
        assert seen == {1: (1, 1, 1, 1), 63: (1, 63, 1, 63), 64: (1, 64, 1, 0), 65: (1, 65, 2, 1), 511: (1, 511, 8, 63),
                        512: (1, 512, 8, 0), 513: (2, 1, 1, 1), 1025: (3, 1, 1, 1)}
        assert np.all(nseg[meta.Kmax - 7:] == 1) if name == 'lensP' else True      # a padded row is one empty segment
    # skewed: rows of up to 15 segments
    area, nseg, lists = host_lists(meta_of(ops, 'skew'))
    assert area.max() == 7396 and nseg.max() == 15 and int((nseg > 1).sum()) >= 3
    # by_cell at its capacity, one cell row beyond it, far beyond it -- the box with the kernels' own float32 clamp rule
    for name, cells in (('box32', (32, 32)), ('box33', (33, 32))):
        meta = meta_of(ops, name)
        area, nseg, lists = host_lists(meta)
        r = int(meta.new_row[0, pc.label_map(name)['probe']['box']])
        assert nseg[r] == 1 and pr.segment_boxes(lists[r], 128, 128, 64, 64) == [cells]
        assert (cells[0] * cells[1] <= pr.SP_CELL_CAP) == (name == 'box32') and 32 * 32 == pr.SP_CELL_CAP
    meta = meta_of(ops, 'diag')
    area, nseg, lists = host_lists(meta)
    r = int(meta.new_row[0, pc.label_map('diag')['probe']['diag']])
    (bh, bw), = pr.segment_boxes(lists[r], 128, 128, 64, 64)
    assert area[r] == 100 and bh * bw > 2 * pr.SP_CELL_CAP
    for name in ('box32', 'box33', 'diag'):                                        # the rest of those maps goes cell by cell
        meta = meta_of(ops, name)
        area, nseg, lists = host_lists(meta)
        r = int(meta.new_row[0, list(pc.label_map(name)['probe'].values())[0]])
        assert all(a * b <= pr.SP_CELL_CAP for rr, lst in enumerate(lists) if rr != r for a, b in pr.segment_boxes(lst, 128, 128, 64, 64))
    # the step's real geometry: 576 superpixels, some rows of two segments
    area, nseg, lists = host_lists(meta_of(ops, 'vor480'))
    assert len(lists) == 576 and nseg.max() >= 2


def _record(case, what, cls, got, ref, scale, f_whole, f_row, cap, unit='per row'):
    """The two measures of one image against fp64, printed beside the fp32-CPU figures and the bars before anything is asserted."""
    whole, per_row = pr.measures(got, ref, scale)
    bw, br = pr.bar_from(f_whole, cap), pr.bar_from(f_row, cap)
    print(f'{case}: whole {whole:.3e} (fp32 CPU {f_whole:.3e}, bar {bw:.3e})  {unit} {per_row:.3e} (fp32 CPU {f_row:.3e}, bar {br:.3e})')
    within(case, f'{what}, fp32 on the CPU vs fp64, whole tensor ({cls})', f_whole, cap)
    within(case, f'{what}, fp32 on the CPU vs fp64, {unit} ({cls})', f_row, cap)
    ok_w = within(case, f'{what}, HIP vs fp64, whole tensor ({cls})', whole, bw, 'bar = min(4 x the fp32-CPU figure of the case, cap)')
    ok_r = within(case, f'{what}, HIP vs fp64, {unit} ({cls})', per_row, br, 'bar = min(4 x the fp32-CPU figure of the case, cap)')
    return ok_w, ok_r, (whole, bw, per_row, br)


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize('i', range(len(pc.FWD)), ids=[pc.fwd_id(c) for c in pc.FWD])
def test_sp_pool_upsample_fwd_against_fp64(ops, i):
    c = pc.FWD[i]
    name, _, _, C, coff, _ = c
    meta = meta_of(ops, name)
    B, H, W, h, w = pc.geometry(c)
    d = dev()
    s = pc.fwd_input(i, c)
    ldo = coff + C + 32
    out = torch.full((B, meta.Kmax, ldo), SENTINEL, device=d)
    ops.sp_pool_upsample_fwd(s.to(d), meta, out, coff)
    again = torch.full((B, meta.Kmax, ldo), SENTINEL, device=d)
    ops.sp_pool_upsample_fwd(s.to(d), meta, again, coff)
    assert torch.equal(out, again)                                                  # two calls, bit-equal
    out = out.cpu()
    fails = []
    for b, (ref, scale, f_whole, f_row) in enumerate(pc.fwd_reference(i, c)):
        K = ref.shape[0]
        ok_w, ok_r, fig = _record(f'{pc.fwd_id(c)}[{b}]', 'pooling fwd', pc.map_class(name), out[b, :K, coff:coff + C].numpy(), ref, scale,
                                  f_whole, f_row, pr.CAP_FUSED)
        if not (ok_w and ok_r):
            fails.append((b, fig))
        # outside the slice the sentinel survives bit for bit; the padded rows of the slice are zero (what test_sp_pool demands of them)
        assert torch.equal(out[b, :, :coff], torch.full((meta.Kmax, coff), SENTINEL))
        assert torch.equal(out[b, :, coff + C:], torch.full((meta.Kmax, 32), SENTINEL))
        assert torch.equal(out[b, K:, coff:coff + C], torch.zeros(meta.Kmax - K, C))
    assert not fails, fails


# ---------------------------------------------------------------- matrix form
def _fp32_wm(new_row, area, H, W, h, w):
    """The matrix by the honest fp32 evaluation: fp32_forward of the unit vectors of the coarse grid, 256 at a time."""
    out = np.empty((len(area), h * w), dtype=np.float32)
    for q0 in range(0, h * w, 256):
        n = min(256, h * w - q0)
        e = np.zeros((h * w, n), dtype=np.float32)
        e[np.arange(q0, q0 + n), np.arange(n)] = 1.0
        out[:, q0:q0 + n] = pr.fp32_forward(e.reshape(h, w, n), new_row, area, H, W)
    return out


@pytest.mark.parametrize('name,h,w', [('vor480', 60, 60), ('vor480', 30, 30), ('ms156', 39, 58), ('lensP', 13, 19), ('lens', 64, 128),
                                      ('vor96', 24, 24)])
def test_interp_matrix_against_the_fp64_matrix(ops, name, h, w):
    """Entry by entry; a row's scale is its largest entry (a row of a 1025-pixel superpixel is held to ITS entries); the bar is
    4 x the fp32-CPU matrix' figure, at most 1e-5 (what test_sp_interp_matrix_equals_fused_upsample_pool demands of Wm's products)."""
    meta = meta_of(ops, name)
    H, W = meta.H, meta.W
    Wm = ops.sp_interp_matrix(meta, h, w)
    assert torch.equal(Wm, ops.sp_interp_matrix(meta, h, w))
    Wm = Wm.cpu()
    for b, (new_row, area, K) in enumerate(pc.rows(name)):
        ref = pr.dense_wm(new_row, area, H, W, h, w)
        scale = ref.max(axis=1)
        f_whole, f_row = pr.measures(_fp32_wm(new_row, area, H, W, h, w), ref, scale)
        ok_w, ok_r, fig = _record(f'Wm-{name}-{h}x{w}[{b}]', 'interp matrix', 'all', Wm[b, :K].numpy(), ref, scale, f_whole, f_row, pr.CAP_FUSED)
        assert ok_w and ok_r, fig
        assert torch.equal(Wm[b, K:], torch.zeros(meta.Kmax - K, h * w))            # rows beyond n_sp exactly zero
        assert abs(float(Wm[b, :K].double().sum(1).sub(1).abs().max())) < 1e-5


def test_interp_matrix_accepts_8192_cells_and_refuses_more(ops):
    meta = meta_of(ops, 'lens')                                                     # 128 x 128
    assert ops.sp_interp_matrix(meta, 64, 128).shape == (1, meta.Kmax, 8192)
    with pytest.raises(AssertionError):
        ops.sp_interp_matrix(meta, 65, 128)                                          # 8320
    lab = (np.arange(3 * 2731) // 1000).reshape(1, 3, 2731).astype(np.int32)         # 8193 = 3 x 2731 needs a map that wide
    thin = ops.sp_preprocess(torch.from_numpy(lab).to(dev()), None, 9)
    thin.check()
    with pytest.raises(AssertionError):
        ops.sp_interp_matrix(thin, 3, 2731)
    assert ops.sp_interp_matrix(thin, 3, 2730).shape == (1, 9, 8190)


# ---------------------------------------------------------------- backward
def _padded_g(x, K_of, coff, C, ldf, d):
    """g (B, Kmax, ldf): the case's rows in [coff, coff + C), 1e30 in the rows beyond n_sp and in every other column."""
    B, Kmax = x.shape[:2]
    g = torch.full((B, Kmax, ldf), pc.SENTINEL_G)
    g[:, :, coff:coff + C] = x
    for b in range(B):
        g[b, K_of[b]:] = pc.SENTINEL_G
    return g.to(d)


@pytest.mark.parametrize('i', range(len(pc.BWD)), ids=[pc.bwd_id(c) for c in pc.BWD])
def test_backward_routes_against_the_fp64_adjoint(ops, i):
    c = pc.BWD[i]
    route, name, _, _, C, coff = c
    meta = meta_of(ops, name)
    B, H, W, h, w = pc.geometry((name, c[2], c[3]))
    d = dev()
    x = pc.bwd_input(i, c)
    K_of = [r[2] for r in pc.rows(name)]
    Ct = sum(C) if isinstance(C, tuple) else C
    ldf = Ct if coff == 0 else coff + Ct + 32
    # the shape reaches the route it is listed under (dispatch of wesup_upsample_bwd, csrc/spatial.hip)
    native = (h, w) == (H, W)
    assert {'ident': native, 'cell': not native and Ct <= 256, 'wide': not native and 256 < Ct <= 768 and ldf == Ct and coff == 0,
            'strided': not native and 256 < Ct and ldf != Ct, 'generic': not native and Ct > 768, 'group': not native and Ct <= 768,
            'unfused': True, 'pool': native}[route]
    if route == 'group':
        assert {(64,): 1, (128, 128): 1, (32, 256): 2, (256, 256, 256): 3}[C] == (Ct // 4 + 63) // 64          # NPASS
        gs = [_padded_g(xi.contiguous(), K_of, 0, xi.shape[2], xi.shape[2], d) for xi in torch.split(x, list(C), dim=2)]
        outs = [torch.full((B, h, w, ci), 7.0, device=d) for ci in C]
        ops.upsample_bwd_fused_group(gs, meta.new_row, meta.area_new, H, W, h, w, outs)
        got = torch.cat(outs, dim=3)
        outs2 = [torch.full((B, h, w, ci), 7.0, device=d) for ci in C]
        ops.upsample_bwd_fused_group(gs, meta.new_row, meta.area_new, H, W, h, w, outs2)
        assert torch.equal(got, torch.cat(outs2, dim=3))
    elif route == 'unfused':
        dfm = torch.full((B, H, W, ldf), pc.SENTINEL_G)
        dfm[..., coff:coff + Ct] = x
        got = ops.upsample_bwd(dfm.to(d), coff, h, w, Ct)
        assert torch.equal(got, ops.upsample_bwd(dfm.to(d), coff, h, w, Ct))
    elif route == 'pool':
        g = _padded_g(x, K_of, 0, Ct, Ct, d)
        got = ops.sp_pool_bwd(g, meta).view(B, H * W, Ct)
        assert torch.equal(got, ops.sp_pool_bwd(g, meta).view(B, H * W, Ct))
    else:
        g = _padded_g(x, K_of, coff, Ct, ldf, d)
        got = ops.upsample_bwd_fused(g, meta.new_row, meta.area_new, H, W, coff, h, w, Ct)
        assert torch.equal(got, ops.upsample_bwd_fused(g, meta.new_row, meta.area_new, H, W, coff, h, w, Ct))
    got = got.cpu()
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) < 1e6          # nothing of the 1e30 rows / columns arrived
    fails = []
    for b, (ref, scale, f_whole, f_row) in enumerate(pc.bwd_reference(i, c)):
        ok_w, ok_r, fig = _record(f'{pc.bwd_id(c)}[{b}]', 'pooling bwd', route, got[b].numpy(), ref, scale, f_whole, f_row, pc.bwd_cap(c),
                                  unit='per cell')
        if not (ok_w and ok_r):
            fails.append((b, fig))
    assert not fails, fails


def test_wide_and_strided_routes_get_the_same_data():
    iw, i_s = [i for i, c in enumerate(pc.BWD) if c[0] in ('wide', 'strided') and c[4] == 512]
    assert torch.equal(pc.bwd_input(iw, pc.BWD[iw]), pc.bwd_input(i_s, pc.BWD[i_s]))


def test_group_refuses_772_channels(ops):
    meta = meta_of(ops, 'vor96')
    d = dev()
    gs = [torch.zeros(2, meta.Kmax, c, device=d) for c in (256, 256, 260)]
    outs = [torch.zeros(2, 24, 24, c, device=d) for c in (256, 256, 260)]
    with pytest.raises(AssertionError):
        ops.upsample_bwd_fused_group(gs, meta.new_row, meta.area_new, 96, 96, 24, 24, outs)
    ops.upsample_bwd_fused_group([g[..., :256].contiguous() for g in gs], meta.new_row, meta.area_new, 96, 96, 24, 24,
                                 [o[..., :256].contiguous() for o in outs])          # 768 is the limit and is taken


# ---------------------------------------------------------------- max-pool
def _window_kinds(y):
    """y (B, H, W, C): counts of the window contents the test must contain, over the 2 x 2 windows of the even part."""
    B, H, W, C = y.shape
    v = y[:, :H // 2 * 2, :W // 2 * 2].reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(-1, 4)
    mx = v.max(dim=1).values
    return dict(four_way=int(((v == mx[:, None]).sum(1) == 4).sum()), all_negative=int((mx < 0).sum()), max_zero=int((mx == 0).sum()),
                tie_1_2=int(((v[:, 1] == mx) & (v[:, 2] == mx) & (v[:, 0] < mx)).sum()),
                tie_2_3=int(((v[:, 2] == mx) & (v[:, 3] == mx) & (v[:, 0] < mx) & (v[:, 1] < mx)).sum()))


@pytest.mark.parametrize('B,H,W,C', [(2, 7, 10, 8), (2, 10, 7, 8), (1, 9, 11, 12), (3, 2, 2, 8), (3, 3, 3, 8), (1, 33, 18, 64)])
def test_maxpool_odd_sizes_and_ties(ops, B, H, W, C):
    """Small-integer data (ties everywhere) plus written-in windows: four-way ties, all-negative windows, a maximum of exactly 0.0,
    ties between positions 1 and 2 (the first of them takes the gradient).  Every value is a copy or one fp32 add: torch.equal."""
    d = dev()
    gen = torch.Generator().manual_seed(H * 100 + W)
    y = torch.randint(-2, 3, (B, H, W, C), generator=gen).float()
    y[0, :2, :2, 0] = 1.5                                                            # four-way tie, positive
    y[0, :2, :2, 1] = -3.0                                                           # four-way tie, all negative
    y[0, :2, :2, 2] = torch.tensor([[-1.0, 0.0], [-2.0, -0.5]])                      # maximum exactly 0.0
    y[0, :2, :2, 3] = torch.tensor([[0.5, 2.0], [2.0, 1.0]])                         # tie between positions 1 and 2
    y[0, :2, :2, 4] = torch.tensor([[0.5, 1.0], [2.0, 2.0]])                         # tie between positions 2 and 3
    y[0, :2, :2, 5] = torch.tensor([[-4.0, -1.0], [-1.0, -2.0]])                     # tie between 1 and 2, negative
    kinds = _window_kinds(y)
    assert all(v > 0 for v in kinds.values()), kinds
    yr = y.permute(0, 3, 1, 2).clone().requires_grad_(True)
    p = F.max_pool2d(F.relu(yr), 2, 2)
    dyp = torch.randn(p.shape, generator=gen)
    p.backward(dyp)
    want_p = p.detach().permute(0, 2, 3, 1).contiguous()
    want_g = yr.grad.permute(0, 2, 3, 1).contiguous()
    yd, dypd = y.to(d), dyp.permute(0, 2, 3, 1).contiguous().to(d)
    assert torch.equal(ops.maxpool2_fwd(yd, relu=True).cpu(), want_p)
    raw = ops.maxpool2_fwd(yd).cpu()                                                 # pre-ReLU maxima
    assert torch.equal(raw, F.max_pool2d(y.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)) and torch.equal(F.relu(raw), want_p)
    got = ops.maxpool2_bwd(yd, dypd).cpu()
    assert torch.equal(got, want_g)
    base = torch.randn(B, H, W, C, generator=gen)
    acc = base.clone().to(d)
    ops.maxpool2_bwd(yd, dypd, acc, accumulate=True)
    assert torch.equal(acc.cpu(), base + want_g)                                     # the same single fp32 add
    # the trailing row / column of an odd size belongs to no window: zero gradient, or ``base`` untouched
    if H % 2:
        assert float(got[:, H - 1].abs().max()) == 0.0 and torch.equal(acc.cpu()[:, H - 1], base[:, H - 1])
    if W % 2:
        assert float(got[:, :, W - 1].abs().max()) == 0.0 and torch.equal(acc.cpu()[:, :, W - 1], base[:, :, W - 1])
