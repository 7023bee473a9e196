"""SHA-256 digests of what the two-class head entries of the C ABI write, case by case: the cases and the hashing shared by
tools/make_head_bits_golden.py (which records them from the library of the commit before the two-class kernels were folded onto
the C-class ones) and tests/test_multiclass_gpu.py (which recomputes them from the library under test).

Only ``_lib`` is used, never the ``ops`` wrappers: the same code runs against either library (WESUP_HIP_LIB).  Inputs come from
seeded builders (tests/_headcases.py, numpy's RandomState); every output buffer starts from a sentinel, so a word an entry leaves
unwritten is part of the digest too."""
import hashlib

import numpy as np
import torch

import _headcases as hc

CLS_R = (1, 63, 64, 65, 300)
CLS_D = (32, 7)
WRAP_R = 2048 * 256 + 257            # the streaming forward kernel's capped grid (2048 blocks x 256 rows) takes a second trip
LDS_D = (8191, 8192)                 # Wc | bc fill the 64 KiB of LDS exactly / one row beyond: read from global memory
PROP_CASES = ('D1-C2-K563', 'D32-C2-K553', 'D64-C2-K563')
HEAD_FWD_CASES = ('fused-D32-C2-K576', 'fused-D128-C2-K576')
LOSS_CASES = ('C2-A-w0.5', 'C2-B-w0.25')
S = hc.SENTINEL


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _p(t):
    import ctypes
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


def _full(shape, value=S, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device='cuda:0')


def _cls_inputs(R, D, seed):
    """feat = relu(randn), Wc, bc, a softmax-like pred formed without a transcendental, dpred, extra."""
    rs = np.random.RandomState(seed)
    feat = np.maximum(rs.randn(R, D), 0).astype(np.float32)
    Wc, bc = (rs.randn(2, D) * 0.3).astype(np.float32), rs.randn(2).astype(np.float32)
    u = (rs.rand(R, 2) + 0.05).astype(np.float32)
    pred = u / (u[:, :1] + u[:, 1:])
    return feat, Wc, bc, pred, rs.randn(R, 2).astype(np.float32), rs.randn(R, D).astype(np.float32)


def _classifier_fwd(lib, out):
    def run(key, feat, Wc, bc):
        R, D = feat.shape
        pred = _full((R, 2))
        assert feat.is_contiguous() and lib.wesup_classifier_fwd(_p(feat), _p(Wc), _p(bc), _p(pred), R, D, None) == 0, key
        out['wesup_classifier_fwd/' + key] = {'pred': _sha(pred)}

    for D in CLS_D:
        for R in CLS_R:
            feat, Wc, bc = _cls_inputs(R, D, 100 * D + R)[:3]
            run(f'D{D}-R{R}', _dev(feat), _dev(Wc), _dev(bc))
    feat, Wc, bc = _cls_inputs(300, 32, 11)[:3]          # a view one float into its buffer: no float4 reads
    base = _full((300 * 32 + 4,))
    view = base[1:1 + 300 * 32].view(300, 32)
    view.copy_(_dev(feat))
    assert view.data_ptr() % 16 == 4
    run('D32-R300-offset-by-one-float', view, _dev(Wc), _dev(bc))
    feat, Wc, bc = _cls_inputs(WRAP_R, 32, 12)[:3]
    run(f'D32-R{WRAP_R}', _dev(feat), _dev(Wc), _dev(bc))
    for D in LDS_D:
        feat, Wc, bc = _cls_inputs(65, D, D)[:3]
        run(f'D{D}-R65', _dev(feat), _dev(Wc * np.float32(0.05)), _dev(bc))


def _classifier_bwd(lib, out):
    for D in CLS_D:
        for R in CLS_R:
            feat, Wc, _, pred, dpred, extra = (_dev(a) for a in _cls_inputs(R, D, 200 * D + R))
            nb = lib.wesup_classifier_bwd_workspace_bytes(R, D)
            for ex, tag in ((extra, 'extra'), (None, 'plain')):
                dfeat, dWc, dbc = _full((R, D)), _full((2, D)), _full((2,))
                ws = _full((nb,), 0, torch.uint8)
                assert lib.wesup_classifier_bwd(_p(feat), _p(Wc), _p(pred), _p(dpred), _p(ex), _p(dfeat), _p(dWc), _p(dbc), R, D,
                                                _p(ws), nb, None) == 0
                out[f'wesup_classifier_bwd/D{D}-R{R}-{tag}'] = {'dfeat': _sha(dfeat), 'dWc': _sha(dWc), 'dbc': _sha(dbc)}


def _prop(lib, out):
    ids = [c[0] for c in hc.PROP]
    for name in PROP_CASES + HEAD_FWD_CASES:
        i = ids.index(name)
        c = hc.prop_case(i)
        B, Kmax, C, D = len(c['n_sp']), c['Kmax'], c['C'], c['D']
        assert C == 2
        feat, labels, n_sp, n_l = _dev(c['feat']), _dev(c['labels']), _dev(c['n_sp'].astype(np.int32)), _dev(c['n_l'].astype(np.int32))
        y_all, src, sim = _full((B, Kmax, C)), _full((B, Kmax), -777, torch.int32), _full((B, Kmax))
        tail = (_p(labels), _p(n_sp), _p(n_l), hc.THR, 1, _p(y_all), _p(src), _p(sim), B, Kmax, D, C, None)
        if name in PROP_CASES:
            assert lib.wesup_propagate(_p(feat), *tail) == 0
            out['wesup_propagate/' + name] = {'y_all': _sha(y_all), 'src_idx': _sha(src), 'max_sim': _sha(sim)}
        else:
            rng = np.random.default_rng(i)
            Wc, bc = _dev((rng.standard_normal((C, D)) * 0.3).astype(np.float32)), _dev(rng.standard_normal(C).astype(np.float32))
            pred = _full((B * Kmax, C))
            assert lib.wesup_head_fwd(_p(feat), _p(Wc), _p(bc), _p(pred), *tail) == 0
            out['wesup_head_fwd/' + name] = {'pred': _sha(pred), 'y_all': _sha(y_all), 'src_idx': _sha(src), 'max_sim': _sha(sim)}


def _head_bwd(lib, out):
    ids = [c[0] for c in hc.LOSS]
    for name in LOSS_CASES:
        c = hc.loss_case(ids.index(name))
        B, Kmax, C, D = hc.LOSS_B, hc.LOSS_KMAX, c['C'], hc.LOSS_D
        R = B * Kmax
        assert C == 2
        feat, Wc, pred, y_all = _dev(c['feat']), _dev(c['Wc']), _dev(c['pred']), _dev(c['y_all'])
        n_sp, n_l = _dev(c['n_sp'].astype(np.int32)), _dev(c['n_l'].astype(np.int32))
        dloss = _dev(np.array([c['dloss']], dtype=np.float32))
        terms, dpred, dfeat, dWc, dbc = _full((B, 8)), _full((B, Kmax, C)), _full((R, D)), _full((C, D)), _full((C,))
        nb = lib.wesup_classifier_bwd_workspace_bytes(R, D)
        ws = _full((nb,), 0, torch.uint8)
        assert lib.wesup_head_bwd(_p(feat), _p(Wc), _p(pred), _p(y_all), _p(n_sp), _p(n_l), _p(dloss), hc.EPS, c['pw'], _p(terms),
                                  _p(dpred), _p(dfeat), B, Kmax, D, C, _p(ws), nb, None) == 0
        assert lib.wesup_classifier_bwd_finish(_p(ws), nb, _p(dWc), _p(dbc), R, D, None) == 0
        out['wesup_head_bwd+wesup_classifier_bwd_finish/' + name] = {
            'terms': _sha(terms), 'dpred': _sha(dpred), 'dfeat': _sha(dfeat), 'dWc': _sha(dWc), 'dbc': _sha(dbc)}


def digests(lib):
    """{'<entry>/<case>': {'<output>': sha256 hex}} from the two-class entries of ``lib`` (wesup_amd._lib.load()), on cuda:0."""
    out = {}
    for part in (_classifier_fwd, _classifier_bwd, _prop, _head_bwd):
        part(lib, out)
        torch.cuda.synchronize()
    return out
