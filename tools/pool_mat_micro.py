"""The two products of the interpolation-pooling matrix alone on the GPU, on both routes (dense batched TN GEMM / walk over Wm's
non-zeros), forward (sp slice = Wm . s) and backward (ds = Wm^T . gsp slice): the benchmark's two resolutions, the 800 x 800
shard's, batch 1, and small sizes around the crossover.  Wm is a real one (Voronoi label maps through sp_preprocess and
sp_interp_matrix).  The size rule of csrc/pool_mat_route.hpp comes from this table.   python3 tools/pool_mat_micro.py > profiles/pool_mat_micro.txt"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from wesup_amd import ops, synth

d = torch.device('cuda:0')
ENV = 'WESUP_POOL_MAT_SPARSE_MIN'
LD = 2112


def timed(fn, n=10):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / n)
    return sorted(ts)[len(ts) // 2]


_metas = {}


def meta_of(B, H, W, g):
    key = (B, H, W, g)
    if key not in _metas:
        labs = np.stack([synth.voronoi_labels(50 + b, H, W, g) for b in range(B)]).astype(np.int32)
        _metas[key] = ops.sp_preprocess(torch.from_numpy(labs).to(d), None, (g * g + 63) // 64 * 64)
    return _metas[key]


# (B, H, W, grid, h, w, C)
CASES = [(4, 480, 480, 24, 60, 60, 768), (4, 480, 480, 24, 30, 30, 768), (4, 800, 800, 39, 50, 50, 768),
         (1, 480, 480, 24, 60, 60, 768), (1, 480, 480, 24, 30, 30, 768),
         (3, 64, 48, 6, 8, 6, 768), (3, 64, 48, 6, 16, 12, 384), (3, 64, 48, 6, 32, 24, 128), (2, 96, 96, 8, 24, 24, 384),
         (2, 128, 128, 8, 32, 32, 384), (2, 96, 96, 6, 48, 48, 128), (2, 160, 160, 10, 40, 40, 384), (2, 240, 240, 12, 30, 30, 768),
         (2, 240, 240, 12, 60, 60, 384)]
print(f'# us per call alone, median of 5 x 10; entries = Kmax * h * w per image; nnz = non-zeros of Wm per row (mean / max)')
print(f'# {"B":>2} {"image":>9} {"Kmax":>5} {"cells":>7} {"C":>4} {"entries":>9} {"nnz/row":>11} | {"fwd gemm":>9} {"fwd sparse":>10} | '
      f'{"bwd gemm":>9} {"bwd sparse":>10}')
for B, H, W, g, h, w, C in CASES:
    meta = meta_of(B, H, W, g)
    Kmax, hw = meta.Kmax, h * w
    Wm = ops.sp_interp_matrix(meta, h, w)
    WmT = Wm.transpose(1, 2).contiguous()
    nnz = (Wm != 0).sum(dim=2).float()
    s = torch.randn(B, hw, C, device=d)
    sp = torch.zeros(B, Kmax, LD, device=d)
    gsp = torch.randn(B, Kmax, LD, device=d)
    ds = torch.empty(B, hw, C, device=d)
    t = {}
    for kind, val in (('gemm', '0'), ('sparse', '1')):
        os.environ[ENV] = val
        t[kind, 'f'] = timed(lambda: ops.sp_pool_mat_fwd(Wm, WmT, s, sp, 576, ws_tag='side')) * 1e3
        t[kind, 'b'] = timed(lambda: ops.sp_pool_mat_bwd(Wm, WmT, gsp, 576, ds, ws_tag='side')) * 1e3
    del os.environ[ENV]
    print(f'  {B:2d} {H:4d}x{W:<4d} {Kmax:5d} {h:3d}x{w:<3d} {C:4d} {Kmax * hw:9d} {float(nnz[nnz > 0].mean()):5.1f}/{int(nnz.max()):<5d} | '
          f'{t["gemm", "f"]:9.1f} {t["sparse", "f"]:10.1f} | {t["gemm", "b"]:9.1f} {t["sparse", "b"]:10.1f}   '
          f'default rule: {"sparse" if ops.sp_pool_mat_sparse(Kmax, hw) else "gemm"}', flush=True)
