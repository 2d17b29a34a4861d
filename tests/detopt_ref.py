"""CPU twin of cosy_sgd_step in numpy float32, and the cases its tests share.

The rule, one rounding per operation: the scalars are rounded to float32 first;
    d  = g + wd w          (wd == 0: d = g, no product is formed)
    m' = d on the first step, else mu m + d        (mu == 0: no buffer)
    w' = w - lr m'
numpy's float32 arrays round every elementwise product and sum on its own (no fused multiply-add), which is the rule itself."""
import numpy as np

U = 2.0 ** -24                                   # unit roundoff of float32

# (lr, momentum, weight_decay): the reference's setting, then each scalar at zero
SCALARS = {'reference': (0.02, 0.9, 1e-4), 'momentum=0': (0.02, 0.0, 1e-4), 'wd=0': (0.02, 0.9, 0.0), 'lr=0': (0.0, 0.9, 1e-4)}


def sgd_step(w, g, m, lr, momentum, weight_decay, first_step):
    """float32 arrays w, g, m (m: None when momentum == 0) -> (w', m'); m' is None when momentum == 0"""
    w, g = np.asarray(w, np.float32), np.asarray(g, np.float32)
    lr, mu, wd = np.float32(lr), np.float32(momentum), np.float32(weight_decay)
    with np.errstate(all='ignore'):
        d = g if wd == 0 else g + wd * w
        if mu == 0:
            step, m_new = d, None
        else:
            step = d if first_step else mu * np.asarray(m, np.float32) + d
            m_new = step.astype(np.float32, copy=True)
        w_new = w - lr * step
    assert w_new.dtype == np.float32
    return w_new, m_new


def bound(w, g, m, lr, momentum, weight_decay, first_step):
    """first-order bound of the twin's error against exact arithmetic on the same float32 inputs, times 1.01 for the higher orders:
    |dd| <= u (|wd w| + |d|), |dm'| <= |dd| + u (|mu m| + |m'|), |dw'| <= lr |dm'| + u (|lr m'| + |w'|); a term whose operation is not
    performed (wd == 0; the first step; mu == 0) is absent.  Computed in float64 -> (bound of w', bound of m')"""
    w, g = np.asarray(w, np.float64), np.asarray(g, np.float64)
    lr, mu, wd = (float(np.float32(v)) for v in (lr, momentum, weight_decay))
    d = g + wd * w
    dd = U * (np.abs(wd * w) + np.abs(d)) if wd != 0 else np.zeros_like(d)
    if mu != 0 and not first_step:
        m = np.asarray(m, np.float64)
        step = mu * m + d
        dm = dd + U * (np.abs(mu * m) + np.abs(step))
    else:
        step, dm = d, dd
    w_new = w - lr * step
    dw = lr * dm + U * (np.abs(lr * step) + np.abs(w_new))
    return 1.01 * dw, 1.01 * dm


def data(n, seed, special=True):
    """w, g, m float32 of n elements: values of mixed magnitude and, when special and n allows, +-0, a NaN and an Inf gradient and denormals"""
    rng = np.random.RandomState(seed)
    w = (rng.standard_normal(n) * np.exp(rng.uniform(-6, 2, n))).astype(np.float32)
    g = (rng.standard_normal(n) * np.exp(rng.uniform(-8, 1, n))).astype(np.float32)
    m = (rng.standard_normal(n) * np.exp(rng.uniform(-8, 1, n))).astype(np.float32)
    if special:
        tiny = np.float32(1e-41)                 # a denormal
        plan = [(0, 0.0, -0.0, 0.0), (1, -0.0, 0.0, -0.0), (2, 1.0, np.nan, 0.5), (3, -2.0, np.inf, 0.25), (4, tiny, tiny, -tiny), (5, 3.0, -tiny, tiny),
                (6, np.float32(-1.5e-39), 1e-3, 0.0), (7, 0.5, -np.inf, 1.0)]
        for i, (k, wv, gv, mv) in enumerate(plan):
            j = (k * 37) % n if n > 8 else k     # spread over the vector body and, in a short buffer, over what there is
            if j < n and (n > 8 or k < n):
                w[j], g[j], m[j] = wv, gv, mv
    return w, g, m
