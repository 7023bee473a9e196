"""Inputs of the Adam / AdamW kernel tests (tests/test_optim_cpu.py, tests/test_optim_gpu.py) and their references, computed once
per configuration and shared (callers must not write into what they get).

Sizes are those of the SGD kernel's tests, whose shape the Adam kernel has (tests/_headcases.py): n = 1, 2, 3 (tail only), 4 (no
tail), 5, 7, 1023, 1024, 1025, and 2048 * 256 * 4 + 1200 + k, where the capped grid takes a second trip and block 0 a tail of k."""
import functools

import numpy as np

import _adamref as ar
import _headcases as hc

SMALL = hc.SGD_SMALL
WRAP = hc.SGD_WRAP
LARGE = hc.SGD_LARGE
STEPS = 3
# Seed of the wrap cases.  Adam's update m / (sqrt(v) / sqrt(bc2) + eps) is ill-conditioned where g' = g gs + wd p cancels to within
# eps = 1e-8: an absolute rounding error d of g' (6e-8 of the larger term) moves p by lr d / eps there, in ANY float32 evaluation.
# Among the 3 x 2.1 M standard-normal draws of a wrap case such an element turns up about once in four seeds (numpy float32 against
# float64 on the CPU: 3e-5 at seed 77, 6e-6 at 79, <= 2.4e-7 at 80, 81, 82); a draw that holds one measures the formula, not
# the kernel.  tests/test_optim_cpu.py asserts, on the CPU, that no case the GPU tests use does.
WRAP_SEED = 82
BETAS, EPS = (0.9, 0.999), 1e-8
# id -> (lr, betas, eps, weight_decay, grad_scale).  lr is a thousand times the trainer's, for the reason _headcases.sgd_inputs
# gives: at 5e-5 an error in m or v would hide below the rounding of p.
HYPER = {'adam': (5e-2, BETAS, EPS, 1e-3, 0.5), 'adamw': (5e-2, BETAS, EPS, 1e-2, 1.0), 'wd0': (1e-3, BETAS, EPS, 0.0, 0.5)}
# every set under both update rules (decoupled: AdamW)
CONFIGS = [(h, d) for h in HYPER for d in (False, True)]
IDS = [f"{h}-{'adamw' if d else 'adam'}-rule" for h, d in CONFIGS]


def inputs(n, seed):
    """p and the three steps' gradients, float32: standard normal; every 7th gradient scaled by 1e-6 and every 11th zero, so that
    denominators near eps occur (sqrt(v) of 1e-6-sized gradients is ~3e-8 after the first step, of zero gradients 0)."""
    rng = np.random.default_rng(6000 + seed)
    p = rng.standard_normal(n).astype(np.float32)
    gs = []
    for _ in range(STEPS):
        g = rng.standard_normal(n).astype(np.float32)
        g[::7] *= np.float32(1e-6)
        g[::11] = 0.0
        gs.append(g)
    return p, gs


def reference(p0, gs, hyper, decoupled, dtype=np.float64):
    """STEPS steps from p0 with m = v = 0: [(p, m, v) after each step]."""
    p, m, v = np.asarray(p0, dtype=dtype), np.zeros(len(p0), dtype=dtype), np.zeros(len(p0), dtype=dtype)
    out = []
    for step, g in enumerate(gs):
        p, m, v = ar.adam(p, g, m, v, step + 1, hyper, decoupled, dtype)
        out.append((p, m, v))
    assert all(np.isfinite(a).all() for o in out for a in o)
    return out


@functools.lru_cache(maxsize=None)
def case(n, seed, name, decoupled):
    """(p0, gs, fp64 reference, fp32-CPU evaluation) of one size under HYPER[name]'s numbers and the given update rule."""
    hyper = HYPER[name]
    p0, gs = inputs(n, seed)
    return p0, gs, reference(p0, gs, hyper, decoupled), reference(p0, gs, hyper, decoupled, np.float32)
