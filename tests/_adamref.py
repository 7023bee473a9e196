"""What csrc/optim.hip computes, in numpy: one Adam / AdamW step (torch.optim.Adam / AdamW, no amsgrad) with the step's factors
formed the way the tick kernel forms them.  Nothing here calls the library or wesup_amd (tests/test_optim_cpu.py ties the float64
evaluation to torch.optim on float64 tensors).

    per step    step_size = lr / (1 - b1^t);  inv_sqrt_bc2 = 1 / sqrt(1 - b2^t);  decay = 1 - lr wd     -- Python floats (double)
    per element g' = g gs;  Adam: g' += wd p;  AdamW: p *= decay;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g' g';
                p -= step_size m / (sqrt(v) inv_sqrt_bc2 + eps)

``dtype=np.float64`` is the reference; ``np.float32`` the plain evaluation on the CPU whose distance from it sets the bars (4 x,
capped at CAP_ADAM): every constant formed in double and rounded to float32 ONCE (1 - b2 is float32(1 - 0.999), not
float32(1) - float32(0.999), which is wrong in the fifth digit), every product and sum rounded."""
import math

import numpy as np

CAP_ADAM = 1e-6


def factors(t, lr, betas, wd):
    """(step_size, inv_sqrt_bc2, decay) of step t >= 1 as Python floats."""
    b1, b2 = betas
    return lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t), 1.0 - lr * wd


def adam(p, g, m, v, t, hyper, decoupled, dtype=np.float64):
    """One step on copies: (p, m, v) in ``dtype``.  hyper = (lr, (b1, b2), eps, wd, gs) as the host's Python floats; t = the count
    AFTER this step (1 for the first)."""
    lr, (b1, b2), eps, wd, gs = hyper
    step_size, inv_sqrt_bc2, decay = (dtype(x) for x in factors(t, lr, (b1, b2), wd))
    c = {k: dtype(x) for k, x in dict(b1=b1, omb1=1.0 - b1, b2=b2, omb2=1.0 - b2, eps=eps, wd=wd, gs=gs).items()}
    p, g, m, v = (np.asarray(a, dtype=dtype) for a in (p, g, m, v))
    g = g * c['gs']
    if decoupled:
        p = p * decay
    else:
        g = g + c['wd'] * p
    m = c['b1'] * m + c['omb1'] * g
    v = c['b2'] * v + c['omb2'] * g * g
    p = p - step_size * m / (np.sqrt(v) * inv_sqrt_bc2 + c['eps'])
    assert p.dtype == m.dtype == v.dtype == dtype
    return p, m, v
