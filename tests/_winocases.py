"""The host decisions of the Winograd family (wesup_amd/csrc/winograd.hpp, winograd.hip, wino_fused.hip and the Winograd composites
of gemm.hip) restated in plain Python, and the tables of cases that tests/test_wino_routes_cpu.py (does every row reach the kernel,
the size and the edge it names?) and tests/test_wino_routes_gpu.py (is every row right, element by element?) share.

Only the default settings are restated (WESUP_WINO_FUSED*, WESUP_NT_MB and the WESUP_TN_* knobs are read once per process and are
not covered).  A change that moves wino_shape_ok, wino4_block_colsum_ok, the 200-block rule, the narrow / vector rule of
wino_filter_grad_launch or a streaming-store byte formula has to update the restatement below AND the rows it moves.

ROUNDINGS: n of the per-element bound gamma(n) * absref of the Gaussian pass, counted from the kernels' code -- the number of
fp32 roundings on the longest path from an operand to the result (a coefficient that is no fp32 number counts as one more):

  in4      4   wino4_bt: every output is an fma of an fma (t[0] = fma(81/64, d0, fma(-45/16, d2, d4)); t[1] = fma(3/4, b, a) with a
               and b one fma each): 2 per 1-D pass, two passes.  Every coefficient and every product of two (-9/4 * 3/4) is dyadic.
  in2      2   one add or subtract per pass
  og4      4   wino4_a: e1 = fma(9/16, y2, y0), t[1] = fma(3/4, o1, e1): 2 per pass
  og2      2   one add or subtract per pass (0 - y is exact)
  out4    10   wino4_at: o[3] = (fma(27/8, d34, (27/64) d12)) + m5 with d12 a subtraction: 4 per pass, 8; + bias; + old content
  out2     6   s0 = m0 + (m1 + m2): 2 per pass, 4; + bias; + old content
  fused   K + 2 + 12   the GEMM family's K + 2 for the MFMA sum over K; Z[jj] = fma(A^T[jj][nu], M, Z[jj]) over at most five
               non-zero nu, Y[i][jj] = fma(A^T[i][xi], Z[jj], Y[i][jj]) over at most five non-zero xi: 10; + bias; + old content
               (a gathered row: reciprocal, product, add = 3 roundings of |old| alone, below the 12 counted for every term)
  pack4    8   wino4_g: a = fma(-128/243, g0, (-8/27) g2): coefficient, product, fma = 3 for g2, u[1] = a - b: 4 per pass
  pack2    4   hs = (g0 + g2) / 2, hs + hm: 2 per pass (exact on integers: quarters)
  reduce4  S + 10   at most S - 1 adds over the S slabs (two chains and their sum), then wino_gt<6>: s12, coefficient, product,
               subtract, add = 5 per pass
  reduce2  S + 4    ... wino_gt<4>: u1 + u2, u0 + hs: 2 per pass (exact on integers)
  colsum   the number of summands (any order): 16 T for db / a bias row's tiles, the rows for the fold of bias_part
"""
from collections import namedtuple

import _gemmcases as g
from _gemmcases import align_up, cdiv

NT_STREAM_BYTES = 16 * 1048576           # wino_nt_stores' default (WESUP_NT_MB)
FUSED_MIN_BLOCKS = 200                   # g_fused_min_blocks
ROUNDINGS = {'in4': 4, 'in2': 2, 'og4': 4, 'og2': 2, 'out4': 10, 'out2': 6, 'fused': 12, 'pack4': 8, 'pack2': 4, 'reduce4': 10,
             'reduce2': 4}


# ---------------------------------------------------------------- winograd.hpp
def wino_positions(m):
    return (m + 2) ** 2


def wino_tiles(B, H, W, m):
    return B * cdiv(H, m) * cdiv(W, m)


def wino_shape_ok(B, H, W, Ci, Cout, m):
    if m not in (2, 4) or B <= 0 or H <= 0 or W <= 0 or Ci < 32 or Cout < 32 or Ci % 4 or Cout % 4:
        return False
    T, q = wino_tiles(B, H, W, m), max(Ci, Cout) // 4
    return T < 2 ** 24 and T * q < 2 ** 31 and T * q * q < 2 ** 40


# ---------------------------------------------------------------- winograd.hip
def transform_blocks(B, H, W, C, m):
    """the grid of every transform kernel: a thread per (tile, channel quad), 256 a block"""
    return cdiv(wino_tiles(B, H, W, m) * (C // 4), 256)


def block_colsum_ok(C):
    return C // 4 <= 256 and 256 % (C // 4) == 0


def bias_rows(B, H, W, C):
    return transform_blocks(B, H, W, C, 4) if wino_shape_ok(B, H, W, C, C, 4) and block_colsum_ok(C) else 0


def xcd_remap(bid, nwg):
    """common.hpp: hardware block bid of nwg -> the logical block it works on (XCD x takes a contiguous range)"""
    q, r = nwg >> 3, nwg & 7
    xcd, idx = bid & 7, bid >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


def streams(nbytes):
    return nbytes > NT_STREAM_BYTES


def nt_single(B, H, W, C, m=4):
    """wesup_winograd_input_transform[_bits] / _outgrad_transform: one transformed tensor (F(2x2) never streams)"""
    return m == 4 and streams(4 * 36 * wino_tiles(B, H, W, 4) * C)


def nt_dual(B, H, W, C):
    return streams(2 * 4 * 36 * wino_tiles(B, H, W, 4) * C)


def nt_fused(B, H, W, N, unpool=False):
    return streams(4 * B * (4 if unpool else 1) * H * W * N)


def outgrad_workspace_bytes(B, H, W, C, m):
    if m != 4 or not wino_shape_ok(B, H, W, C, C, m):
        return 0
    if not block_colsum_ok(C):
        return g.colsum_workspace_bytes(B * H * W, C)
    blocks = transform_blocks(B, H, W, C, m)
    return align_up(blocks * C * 4, 256) + g.colsum_workspace_bytes(blocks, C)


REDUCE_VARIANTS = ('f2', 'f4-16v', 'f4-64v', 'f4-16', 'f4-64')      # wino_wgrad_reduce_kernel<4,64>, <6,16,true>, <6,64,true>, <6,16>, <6,64>


def reduce_variant(Cout, Cin, m, slab_stride, batch_stride, addr=0):
    tot = Cout * Cin
    narrow = m == 4 and tot // 64 < 512
    vec = m == 4 and tot % 4 == 0 and slab_stride % 4 == 0 and batch_stride % 4 == 0 and addr % 16 == 0
    if m == 2:
        return 'f2'
    return 'f4-' + ('16' if narrow else '64') + ('v' if vec else '')


def reduce_grid(Cout, Cin, m, variant, db=False, bias_part=False):
    per = {'f2': 64, 'f4-16v': 64, 'f4-64v': 256, 'f4-16': 16, 'f4-64': 64}[variant]
    return cdiv(Cout * Cin, per), (0 if not db else cdiv(Cout, 16) if bias_part else cdiv(Cout, 256))


# ---------------------------------------------------------------- wino_fused.hip
def fused_supported(K, N, m):
    return 2 if m == 4 and K in (64, 128, 256) and N >= 64 and N % 64 == 0 else 0


def fused_grid(tiles, N):
    """(tile_blocks, n_blocks): a block owns 32 tiles x 64 channels"""
    return cdiv(tiles, 32), N // 64


def fused_route(K, N, m, tiles, min_blocks=FUSED_MIN_BLOCKS):
    cap = fused_supported(K, N, m)
    if not cap or tiles <= 0:
        return cap
    tb, nb = fused_grid(tiles, N)
    return cap if tb * nb >= min_blocks else 0


FUSED_FORMS = ('plain', 'batched', 'ubatched', 'general')


def fused_form(o):
    """the epilogue form of wino4_gemm_out_kernel for a set of option names (FUSED_OPTIONS below)"""
    unpool = 'unpool_src' in o or 'unpool_code' in o
    gather, area = 'side' in o, 'area' in o
    mask, bits, accum = 'mask' in o, 'bits' in o, 'accum' in o
    if not unpool and not mask and not (gather and area) and (bits or accum or gather):
        return 'batched'
    if unpool and 'unpool_code' in o and not mask and not bits and not (gather and area):
        return 'ubatched'
    if not mask and not unpool and not gather and not accum:
        return 'plain'
    return 'general'


# ---------------------------------------------------------------- gemm.hip: the Winograd composites
def conv_workspace_bytes(B, H, W, Cin, Cout, m):
    if not wino_shape_ok(B, H, W, Cin, Cout, m) or Cin % 32:
        return 0
    P, T = wino_positions(m), wino_tiles(B, H, W, m)
    return align_up(P * T * Cin * 4, 256) + align_up(P * T * Cout * 4, 256)


def wgrad_plan(B, H, W, Ci, Cout, m):
    """plan_tn(Cout, Ci, T, 1, P): the P products ride in the grid as a batch and count as tiles"""
    return g.plan_tn(Cout, Ci, wino_tiles(B, H, W, m), wino_positions(m))


def wgrad_workspace_bytes(B, H, W, Ci, Cout, m):
    if not wino_shape_ok(B, H, W, Ci, Cout, m):
        return 0
    P, T = wino_positions(m), wino_tiles(B, H, W, m)
    S = wgrad_plan(B, H, W, Ci, Cout, m).S
    return (align_up(P * T * Ci * 4, 256) + align_up(P * T * Cout * 4, 256) + align_up(P * S * (Cout * Ci + Cout) * 4, 256) +
            outgrad_workspace_bytes(B, H, W, Cout, m))


def composite_route(B, H, W, K, N, m, min_blocks=FUSED_MIN_BLOCKS, y_relu=False):
    """wino_conv: 'f2', 'two' (transform, batched NT, output transform) or 'one' (transform, wino4_gemm_out_kernel)"""
    if m == 2:
        return 'f2'
    return 'one' if not y_relu and fused_route(K, N, m, wino_tiles(B, H, W, m), min_blocks) == 2 else 'two'


# ---------------------------------------------------------------- the cases
# 1. activation transforms.  entries: which of ACT_ENTRIES the row runs (None: all its channel count admits)
ACT_ENTRIES = ('in2', 'in2-relu', 'in4', 'in4-relu', 'bits', 'bits-relu', 'og2', 'og4', 'og4-db', 'dual', 'dual-bias')
ActCase = namedtuple('ActCase', 'id B H W C edge entries', defaults=(None,))
_BAR1, _BAR2 = ('in4', 'bits', 'og4'), ('dual-bias',)
ACT_CASES = [
    ActCase('act-1x1x1x32', 1, 1, 1, 32, 'one pixel, one tile'),
    ActCase('act-2x5x7x32', 2, 5, 7, 32, 'H, W odd and = 1, 3 mod 4: the last tile row and column hang over'),
    ActCase('act-2x6x10x64', 2, 6, 10, 64, '192 threads at m = 4: one partial block, idle threads in the block column sum'),
    ActCase('act-3x13x9x128', 3, 13, 9, 128, '4.5 blocks at m = 4: the grid is no multiple of 8 and its last block is partial'),
    ActCase('act-5x13x18x128', 5, 13, 18, 128, '12.5 blocks at m = 4: above 8 blocks the XCD remap is no identity, so the order of the '
            'colsum_part rows shows (at 4.5 blocks it is one)', ('in4', 'og4-db', 'dual-bias')),
    ActCase('act-3x9x8x36', 3, 9, 8, 36, 'C/4 = 9: fast division by a non-power of two; no block column sum: db from wesup_colsum'),
    ActCase('act-1x4x4x1024', 1, 4, 4, 1024, 'C/4 = 256: the widest block column sum', ('in4', 'og4-db', 'dual-bias')),
    ActCase('act-1x4x4x1028', 1, 4, 4, 1028, 'C/4 = 257: the other side', ('in4', 'og4-db', 'dual')),
    ActCase('act-1x120x120x128', 1, 120, 120, 128, '16 588 800 bytes: below the streaming-store bar of a single transform', _BAR1),
    ActCase('act-1x121x121x128', 1, 121, 121, 128, '17 713 152 bytes: above it', _BAR1),
    ActCase('act-1x84x84x128', 1, 84, 84, 128, '16 257 024 bytes in two tensors: below the bar of the dual transform', _BAR2),
    ActCase('act-1x88x88x128', 1, 88, 88, 128, '17 842 176 bytes: above it', _BAR2),
]


def act_entries(r):
    """the entries a row runs: the block column sum (dual-bias) needs C/4 | 256"""
    e = ACT_ENTRIES if r.entries is None else r.entries
    return tuple(x for x in e if x != 'dual-bias' or block_colsum_ok(r.C))


# 2. output transform.  pool: whether the row has pooling windows at all
OutCase = namedtuple('OutCase', 'id B H W C edge')
OUT_CASES = [
    OutCase('out-1x1x1x32', 1, 1, 1, 32, 'one pixel: no pooling window'),
    OutCase('out-1x2x2x32', 1, 2, 2, 32, 'one pooling window'),
    OutCase('out-2x5x7x32', 2, 5, 7, 32, 'odd H, W: clamped columns; the trailing row and column belong to no window'),
    OutCase('out-3x9x8x36', 3, 9, 8, 36, 'C/4 = 9'),
    OutCase('out-3x13x9x128', 3, 13, 9, 128, '4.5 blocks at m = 4'),
]
OUT_COMBOS = [(b, mk, ac, yr, pool) for b in (0, 1) for mk in (0, 1) for ac in (0, 1) for yr in (0, 1) for pool in (None, 0, 1)]
UNPOOL_COMBOS = [(b, mk, odd) for b in (0, 1) for mk in (0, 1) for odd in (1, 0)]        # odd: Hu = 2 H + 1, Wu = 2 W + 1

# 3. the one-kernel route.  An option set names what the call is given: bias, mask (float), bits (mask_bits), accum, pool, pool_relu,
# code (pool_code out), unpool_src, unpool_code, side (gather; pre-scaled rows unless 'area')
FUSED_OPTIONS = [
    ('plain', ()), ('plain', ('bias',)), ('plain', ('bias', 'pool')), ('plain', ('pool', 'pool_relu', 'code')),
    ('plain', ('bias', 'pool', 'pool_relu', 'code')),
    ('batched', ('bias', 'bits')), ('batched', ('bias', 'accum')), ('batched', ('bias', 'bits', 'accum')), ('batched', ('side',)),
    ('batched', ('side', 'bits')),
    ('ubatched', ('bias', 'unpool_code')), ('ubatched', ('unpool_code', 'side')),
    ('general', ('bias', 'mask')), ('general', ('bias', 'mask', 'accum')), ('general', ('bias', 'unpool_src')),
    ('general', ('side', 'area')), ('general', ('mask', 'side', 'area')), ('general', ('unpool_src', 'side', 'area')),
]
FusedCase = namedtuple('FusedCase', 'id B H W K N edge only', defaults=(None,))
_KN = [(64, 64), (64, 192), (128, 128), (256, 64), (256, 192)]
FUSED_CASES = (
    [FusedCase(f'fu-1x2x2-{K}x{N}', 1, 2, 2, K, N, 'one tile of 32') for K, N in _KN] +
    [FusedCase(f'fu-3x9x8-{K}x{N}', 3, 9, 8, K, N, '18 tiles, three images in one partial block') for K, N in _KN + [(128, 64)]] +
    [FusedCase(f'fu-2x13x21-{K}x{N}', 2, 13, 21, K, N, '48 tiles: an image boundary inside the first block, 16 valid rows in the '
               'second, a last tile row with one image row, a last tile column with one image column') for K, N in _KN + [(64, 128)]] +
    [FusedCase('fu-4x13x21-64x192', 4, 13, 21, 64, 192, '9 blocks: dNb divides by three, the grid is no multiple of 8'),
     FusedCase('fu-1x128x128-64x256', 1, 128, 128, 64, 256, '16 777 216 bytes: at the streaming-store bar, not above', ((), ('bias',))),
     FusedCase('fu-1x129x128-64x256', 1, 129, 128, 64, 256, '16 908 288 bytes: above the bar', ((), ('bias',))),
     FusedCase('fu-1x64x64-64x256', 1, 64, 64, 64, 256, 'unpooling, 16 777 216 bytes: at the bar', (('unpool_code', 'side'), ('unpool_src', 'side', 'area'))),
     FusedCase('fu-1x66x64-64x256', 1, 66, 64, 64, 256, 'unpooling, 17 301 504 bytes: above the bar (so is H = 65; 64 is the last below)',
               (('unpool_code', 'side'), ('unpool_src', 'side', 'area')))])


def fused_options(r):
    return [(f, o) for f, o in FUSED_OPTIONS if r.only is None or o in r.only]


# 4. filter transforms (Cout, Cin): Cout != Cin so that a transposed index shows; any channel count is admitted
PACK_CASES = [(5, 7), (36, 32), (64, 100)]

# 5. filter-gradient reduce.  pad: floats a slab is longer than Cout Cin + Cout; gap: floats between two positions' stacks
ReduceCase = namedtuple('ReduceCase', 'id Cout Cin m pad gap S variant edge db', defaults=(False,))
_SALL = (1, 2, 3, 4, 5, 7)
REDUCE_CASES = [
    ReduceCase('red-36x32-f4', 36, 32, 4, 0, 0, _SALL, 'f4-16v', 'every tail of the vector form: S % 4, then S % 2'),
    ReduceCase('red-36x32-f4-gap', 36, 32, 4, 4, 8, (3,), 'f4-16v', 'strides that are multiples of 4 but not the slab size'),
    ReduceCase('red-36x32-f4-odd', 36, 32, 4, 2, 0, _SALL, 'f4-16', 'a slab stride that is no multiple of 4: scalar loads'),
    ReduceCase('red-5x7-f4', 5, 7, 4, 0, 0, (1, 2, 3), 'f4-16', '35 pairs: no multiple of 4; one partial block'),
    ReduceCase('red-128x252-f4', 128, 252, 4, 0, 0, (2,), 'f4-16v', '504 groups of 64 pairs: narrow'),
    ReduceCase('red-128x256-f4', 128, 256, 4, 0, 0, (2, 5), 'f4-64v', '512 groups: the other side of the narrow rule'),
    ReduceCase('red-128x256-f4-odd', 128, 256, 4, 2, 0, (3,), 'f4-64', '... with a stride that is no multiple of 4'),
    ReduceCase('red-260x32-f2', 260, 32, 2, 0, 0, (1, 2, 3), 'f2', 'F(2x2) with db: two bias blocks', True),
    ReduceCase('red-36x32-f2-odd', 36, 32, 2, 3, 5, (2,), 'f2', 'F(2x2), odd strides', True),
]
# the per-block bias rows through wesup_conv3x3_wgrad_winograd_pre (B, H, W, Ci, Cout, rows)
BIASROW_CASES = [(1, 132, 132, 32, 512, 545, 'one trip of the eight-deep loop and a tail'), (1, 8, 8, 32, 64, 1, 'fewer than 64 rows'),
                 (2, 20, 20, 32, 64, 4, 'fewer than 64 rows, more than one')]

# 6. composites (B, H, W, Cin, Cout); the weight gradient's split (B, H, W, Ci, Cout, m, S)
COMP_CASES = [(2, 5, 7, 32, 64), (1, 9, 8, 64, 64), (3, 9, 8, 128, 64)]
COMP_ROUTES = ('f2', 'two', 'one')
# (2,64,64): T = 512 / 2048, whole splits; (2,60,80): T = 600 / 2400, a ragged last split (280 of 320 rows, 96 of 288)
WGRAD_SPLITS = [(2, 5, 7, 32, 64, 4, 1), (2, 5, 7, 32, 64, 2, 1), (2, 64, 64, 64, 64, 4, 2), (2, 64, 64, 64, 64, 2, 8),
                (2, 60, 80, 64, 64, 4, 2), (2, 60, 80, 64, 64, 2, 9)]


# ---------------------------------------------------------------- the rows' data and the absolute-value pipeline
def absolute():
    """Context: oracle/winograd_oracle.py with |B^T|, |G|, |A^T| in place of its matrices -- the same pipeline on absolute
    values, which is the absref of the Gaussian pass and the premise of the integer pass."""
    import contextlib

    import numpy as np
    from oracle import winograd_oracle as wo

    @contextlib.contextmanager
    def swap():
        saved = {k: dict(getattr(wo, k)) for k in ('_BT', '_G', '_AT')}
        try:
            for k, d in saved.items():
                for m in d:
                    getattr(wo, k)[m] = np.abs(d[m])
            yield wo
        finally:
            for k, d in saved.items():
                getattr(wo, k).update(d)
    return swap()


def _data(shape, kind, seed, scale=1.0):
    from test_gemm_routes_gpu import data
    return data(tuple(shape), kind, seed, scale).numpy().copy()


def seed_zeros(a):
    """exact zeros and negative zeros at fixed places (x > 0 and mask > 0 are false for both)"""
    f = a.reshape(-1)
    f[::7] = 0.0
    f[3::11] = -0.0
    return a


def act_data(r, kind):
    """x / dy of an activation row, (B, H, W, C) fp32"""
    return seed_zeros(_data((r.B, r.H, r.W, r.C), kind, 1))


def mask_data(shape, kind, seed):
    import numpy as np
    a = _data(shape, kind, seed)
    return seed_zeros(np.sign(a) if kind == 'int' else a)              # int: {-1, 0, 1}


def out_data(r, kind, m):
    T = wino_tiles(r.B, r.H, r.W, m)
    px = (r.B, r.H, r.W, r.C)
    return dict(Mt=_data((wino_positions(m), T, r.C), kind, 1), bias=_data((r.C,), kind, 3), old=_data(px, kind, 4),
                mask=mask_data(px, kind, 5))


def fused_data(r, kind):
    """V (36, T, K), U (36, N, K): {-1, 0, 0, 1} in the integer pass"""
    import numpy as np
    T = wino_tiles(r.B, r.H, r.W, 4)
    if kind == 'int':
        import torch
        lut = np.array([-1.0, 0.0, 0.0, 1.0], dtype=np.float32)
        draw = lambda shape, seed: lut[torch.randint(0, 4, shape, generator=torch.Generator().manual_seed(seed)).numpy()]      # noqa: E731
        V, U = draw((36, T, r.K), 1), draw((36, r.N, r.K), 2)
    else:
        V, U = _data((36, T, r.K), kind, 1), _data((36, r.N, r.K), kind, 2, r.K ** -0.5)
    px = (r.B, r.H, r.W, r.N)
    return dict(V=V, U=U, bias=_data((r.N,), kind, 3), old=_data(px, kind, 4), mask=mask_data(px, kind, 5))


def reduce_data(r, kind, S):
    """slabs (P, S, Cout Cin + Cout)"""
    return _data((wino_positions(r.m), S, r.Cout * r.Cin + r.Cout), kind, 10 + S)
