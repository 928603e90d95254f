"""Cases, fp64 restatements and derived bounds for the fused trainer's update rules (flair_amd.optim, csrc/optim.hip).

The restatements are numpy fp64 and start from fp32 inputs: parameters, gradients, state, and -- with ``round_hyper`` -- the
hyper-parameters as the C ABI receives them (fp32).  A device result is compared with ONE restated step from the device's own
pre-step state, so no error is compounded and no tolerance is guessed: each bound is (number of fp32 roundings of the expression as
the kernel writes it) x 2^-24 x (the magnitude those roundings act on).

Roundings, as csrc/optim.hip writes the expressions (contraction into FMAs only removes some):
  g' = g * grad_scale * coef                 2   (left out of the unscaled instances)
  g' += wd * p                               2
  buf = mu * buf + (1 - damp) * g'           3   (a first step copies: 0), + 1 for the constant 1 - damp when damp != 0
  g' = g' + mu * buf   (nesterov)            2
  p -= lr * g'                               2
SGD:  |dp| <= k 2^-24 (|p| + lr (|g'| + |buf|)),  |dbuf| <= k_buf 2^-24 |buf|.  |g'| and |buf| are the sums of the magnitudes of
their terms (|g grad_scale coef| + wd |p|;  mu |buf_old| + (1 - damp) |g'|): that is what the roundings act on, and it is what
keeps the bound true where the terms cancel.
AdamW:
  m = m + (g' - m) * (1 - b1)                4   (sub, the constant, mul, add)  [+ 2 scaled]      on |m_old| + |g'|
  v = b2 * v + (1 - b2) * (g' * g')          5   (square, the constant, two muls, add) [+ 4 scaled: g' enters squared]   on v
  denom = sqrt(v) / sqrt(bc2) + eps          4   (+ half of v's count: the square root halves a relative error)
  step = (lr / bc1) * (m / denom)            3
  p = fma(p, 1 - lr wd, -step)               the constant 1 - lr wd and the fma: 2 on |p| (lr wd itself rounds below 2^-24 lr wd),
                                             and the fma's rounding once more on |step|
  |dp| <= 2^-24 (2 |p| + k |lr / bc1 * m / denom|) with k = k_m + ceil(k_v / 2) + 4 + 3 + 1 and |m| taken as |m_old| + |g'|.
Every bound also allows one fp32 denormal step (2^-149) per rounding for results that underflow.
"""
import math

import numpy as np

from flair_amd import optim as FO

U = 2.0 ** -24
TINY = 2.0 ** -149

SIZES = [1, 3, 4, 7, 1028, 4194304 + 1031]   # the last wraps the grid-stride loop: one sweep of the capped grid covers 4 194 304 floats


def f32r(x):
    return float(np.float32(x))


# the restatements take numpy arrays or torch tensors (fp64 on the device keeps the trainer tests, 24 M parameters, quick)
def _f64(x):
    return np.asarray(x, np.float64) if isinstance(x, np.ndarray) else x.double()


def _sqrt(x):
    return np.sqrt(x) if isinstance(x, np.ndarray) else x.sqrt()


def within(got, want, bound):
    """(every |got - want| <= bound, the worst |got - want| / bound) for numpy arrays or torch tensors"""
    err = abs(_f64(got) - want)
    return bool((err <= bound).all()), float((err / (bound + TINY)).max())


# ---------------------------------------------------------------------------------------------------------------- the rule grid
def sgd_grid():
    out = []
    for momentum in (0.0, 0.9):
        for dampening in ((0.0,) if momentum == 0 else (0.0, 0.1)):
            for nesterov in ((False, True) if momentum != 0 and dampening == 0 else (False,)):
                for wd in (0.0, 1e-2):
                    out.append(dict(momentum=momentum, dampening=dampening, nesterov=nesterov, weight_decay=wd))
    return out


def adamw_grid():
    return [dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=wd) for wd in (0.0, 1e-2)]


def rule_cases():
    """(kind, hyper-parameters, scaled): scaled runs with grad_scale = 0.5 and a clip coefficient read from memory"""
    return ([("sgd", hp, sc) for hp in sgd_grid() for sc in (False, True)]
            + [("adamw", hp, sc) for hp in adamw_grid() for sc in (False, True)])


def spec_of(kind, hp):
    return FO.SGD(**hp) if kind == "sgd" else FO.AdamW(**hp)


def hp_of(spec):
    if spec.name == "sgd":
        return dict(momentum=spec.momentum, dampening=spec.dampening, nesterov=spec.nesterov, weight_decay=spec.weight_decay)
    return dict(betas=spec.betas, eps=spec.eps, weight_decay=spec.weight_decay)


def case_id(case):
    kind, hp, sc = case
    if kind == "sgd":
        s = f"sgd-m{hp['momentum']}-d{hp['dampening']}-{'nest-' if hp['nesterov'] else ''}wd{hp['weight_decay']}"
    else:
        s = f"adamw-wd{hp['weight_decay']}"
    return s + ("-scaled" if sc else "")


# ---------------------------------------------------------------------------------------------------------------- SGD
def sgd_roundings(hp, scaled, first):
    """(k of the parameter bound, k of the buffer bound)"""
    k_g = (2 if scaled else 0) + (2 if hp["weight_decay"] != 0 else 0)
    if hp["momentum"] == 0:
        return k_g + 2, 0
    k_b = k_g if first else k_g + 3 + (1 if hp["dampening"] != 0 else 0)
    return k_b + (2 if hp["nesterov"] else 0) + 2, k_b


def sgd_step64(p, g, buf, lr, hp, first, grad_scale=1.0, coef=None, round_hyper=True):
    """One step in fp64.  Returns (p_new, buf_new or None, bound_p, bound_buf)."""
    r = f32r if round_hyper else float
    p, g = _f64(p), _f64(g)
    lr, mu, wd = r(lr), r(hp["momentum"]), r(hp["weight_decay"])
    omd = 1.0 - r(hp["dampening"])
    scaled = grad_scale != 1.0 or coef is not None
    gs = g * r(grad_scale) * (1.0 if coef is None else float(coef))
    G = abs(gs)
    if wd != 0:
        gs = gs + wd * p
        G = G + wd * abs(p)
    B = p * 0.0
    b_new = None
    if mu != 0:
        if first:
            b_new, B = gs + 0.0, G + 0.0
        else:
            b = _f64(buf)
            b_new = mu * b + omd * gs
            B = mu * abs(b) + omd * G
        gs = gs + mu * b_new if hp["nesterov"] else b_new
    p_new = p - lr * gs
    k, k_b = sgd_roundings(hp, scaled, first)
    bound_p = k * U * (abs(p) + lr * (G + B)) + k * TINY
    bound_b = k_b * U * B + k_b * TINY
    return p_new, b_new, bound_p, bound_b


# ---------------------------------------------------------------------------------------------------------------- AdamW
def bias_corrections(betas, t):
    return 1.0 - float(betas[0]) ** int(t), 1.0 - float(betas[1]) ** int(t)


def adamw_roundings(scaled):
    """(k_m, k_v, k of the step term)"""
    k_m = 4 + (2 if scaled else 0)
    k_v = 5 + (4 if scaled else 0)
    return k_m, k_v, k_m + math.ceil(k_v / 2) + 4 + 3 + 1


def adamw_step64(p, g, m, v, lr, hp, t, first, grad_scale=1.0, coef=None, round_hyper=True):
    """One step in fp64 (t: 1-based step of the bias corrections).  Returns (p_new, m_new, v_new, bound_p, bound_m, bound_v)."""
    r = f32r if round_hyper else float
    p, g = _f64(p), _f64(g)
    b1, b2, eps, wd, lr = r(hp["betas"][0]), r(hp["betas"][1]), r(hp["eps"]), r(hp["weight_decay"]), r(lr)
    bc1, bc2 = (r(c) for c in bias_corrections(hp["betas"], t))
    scaled = grad_scale != 1.0 or coef is not None
    gs = g * r(grad_scale) * (1.0 if coef is None else float(coef))
    m0 = p * 0.0 if first else _f64(m)
    v0 = p * 0.0 if first else _f64(v)
    m_new = m0 + (gs - m0) * (1.0 - b1)
    v_new = b2 * v0 + (1.0 - b2) * gs * gs
    denom = _sqrt(v_new) / math.sqrt(bc2) + eps
    p_new = p * (1.0 - lr * wd) - (lr / bc1) * m_new / denom
    k_m, k_v, k = adamw_roundings(scaled)
    M = abs(m0) + abs(gs)
    bound_m = k_m * U * M + k_m * TINY
    bound_v = k_v * U * v_new + k_v * TINY
    bound_p = U * (2 * abs(p) + k * abs(lr / bc1 * M / denom)) + k * TINY
    return p_new, m_new, v_new, bound_p, bound_m, bound_v


# ---------------------------------------------------------------------------------------------------------------- norm and clip
def sqnorm64(*gs):
    return float(sum(np.sum(np.asarray(g, np.float64) ** 2) for g in gs))


def clip64(sq_sum, max_norm, grad_scale=1.0):
    """clip_grad_norm_'s rule as flair_clip_coef computes it: (norm fp32, coef fp32, bound on |norm - this|, bound on |coef - this|).
    norm: the fp64 square root and product round once to fp32 (2 2^-24 covers a double rounding); coef: that, the + 1e-6 and
    the division: 4 roundings."""
    norm = np.float32(math.sqrt(sq_sum) * f32r(grad_scale))
    c = np.float32(max_norm) / (norm + np.float32(1e-6))
    coef = np.float32(1.0) if c > 1 else c
    return norm, coef, 2 * U * float(norm), 4 * U * float(coef)


def rand_f32(n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * scale).astype(np.float32)
