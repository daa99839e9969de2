"""The yardstick of the optimiser step on the device (sigmaenv_optim_step, sigmarl_amd/csrc/sigmaenv_optim.inc; the arithmetic is stated in
sigmarl_amd/csrc/sigmaenv_optim.h, the contract in include/sigmaenv.h): a plain numpy helper module like ppo_head_check.py, imported by the tests
(tests/test_optim_check.py runs it on the host against the header compiled alone, tests/test_gpu_optim_step.py on the device's tensors).

A ``case`` is a dict: ``nets`` -- a list of networks, each a list of tensors in the optimiser's order (weight, bias, weight, bias, ..: odd positions are biases), each
tensor a dict of flat float32 arrays ``p``, ``g``, ``m``, ``v`` -- and the hyper-parameters ``lr``, ``beta1``, ``beta2``, ``eps``, ``max_grad_norm`` (Python floats,
i.e. doubles) and ``t`` (the count of THIS step, >= 1).

``step(case, np.float64)`` is the reference: torch.nn.utils.clip_grad_norm_ (norm_type 2, one norm over all tensors of all networks) and torch.optim.Adam
(weight_decay 0, no amsgrad) in float64 from the same float32 inputs, with the hyper-parameters as the doubles they are:
    total_norm = sqrt(sum g^2);  coef = min(1, max_grad_norm / (total_norm + 1e-6));  g' = g coef
    m' = m + (g' - m)(1 - beta1);  v' = beta2 v + (1 - beta2) g'^2;  p' = p - lr / (1 - beta1^t) * m' / (sqrt(v') / sqrt(1 - beta2^t) + eps)
``step(case, np.float32)`` is the twin: the header's operations in the header's order in float32, including the order of its sums (``chunk_partials``,
``block_sum``, ``total_sumsq``) and the scalars formed in double and rounded once (``scalars``).  Device and header must equal it bit for bit.

The bounds (``bounds``), derived -- not fitted: counts of roundings times u = 2^-24 (round to nearest: one operation's relative error) times the magnitudes that
enter the element, to first order in u, times SECOND = 1 + 2^-10 for the dropped terms of order u^2 (the largest count below is under 40: 40 u < 2^-18).  The inputs
are exact (the same float32 numbers on both sides); gradients are assumed to be zero or large enough for their squares to be normal numbers (|g| >= 2^-63).
  norm    a chunk's sum of squares passes one rounding of the square, at most 4 additions of the lane's chain, 6 of the butterfly and 3 over the wavefronts: 14.
          The P partials pass ceil(P / 256) additions of the second level's chain, 6 and 3 again.  All terms are positive, so the relative error of the sum is at
          most D u, D = 14 + ceil(P / 256) + 9 -- the bound follows from the partition depth --; the square root halves it and rounds once:
              |total_norm - norm64| <= (D / 2 + 1) u norm64                                                                      = r_n norm64
  coef    c = max_grad_norm / (total_norm + 1e-6): max_grad_norm and 1e-6 are rounded to float32 (u each; the second is absorbed, since r_n >= u and the sum's
          relative error is a mean of r_n and u), one addition, one division: |c - c64| <= (r_n + 3 u) c64 = r_c c64.  min(1, .) does not expand distances, so the
          same bound holds for coef; it is 0 where c64 (1 - r_c) > 1 (both sides are exactly 1).  e_c := that bound.
  g'      e_g = |g| e_c + u |g'|
  m'      d = g' - m, times w1 = fl(1 - beta1) (u), added to m:  e_m = w1 e_g + u (3 w1 (|g'| + |m|) + |m| + w1 (|g'| + |m|))
          (e_g + u |d| through the product; the factor's own rounding and the product's: 2 u w1 |d|; the sum's: u |m'|; |d| <= |g'| + |m|, |m'| <= |m| + w1 |d|)
  v'      fl(beta2) v: 2 u beta2 v; (fl(1 - beta2) g') g': 3 u w2 g'^2 + 2 w2 |g'| e_g; the sum: u v':
              e_v = 2 u beta2 v + 3 u w2 g'^2 + 2 w2 |g'| e_g + u v'
  p'      r = sqrt(v'): e_r = e_v / (2 r) + u r (0 where v' = 0: then e_v = 0);  q = r / fl(sqrt_bc2): e_q = e_r / sb + 2 u q;  den = q + fl(eps):
          e_den = e_q + u eps + u den;  quo = m' / den: e_quo = e_m / den + |m'| e_den / den^2 + u |quo|;  upd = fl(step_size) quo: e_upd = ss e_quo + 2 u |upd|;
              e_p = e_upd + u (|p| + |upd|)
Everything on the right is evaluated in float64 from the reference's values.

Planted defects (``DEFECTS``; ``step(case, np.float32, defect=)``): each must miss a bound on the test inputs (tests/test_optim_check.py).
"""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -10
CHUNK, LANES = 1024, 256
DEFECTS = ("eps_in_sqrt", "no_bias_correction", "sqrt_bc2_on_eps", "beta2_for_first_moment", "no_1e6_in_coef", "coef_not_clamped", "no_biases_in_norm",
           "norm_per_network")
KEYS = ("p", "m", "v")


def scalars(case):
    """the header's optim_scalars: formed in double, each rounded to float32 once"""
    lr, b1, b2, t = float(case["lr"]), float(case["beta1"]), float(case["beta2"]), int(case["t"])
    return dict(beta2=np.float32(b2), w1=np.float32(1.0 - b1), w2=np.float32(1.0 - b2), step_size=np.float32(lr / (1.0 - math.pow(b1, float(t)))),
                sqrt_bc2=np.float32(math.sqrt(1.0 - math.pow(b2, float(t)))), eps=np.float32(case["eps"]), max_grad_norm=np.float32(case["max_grad_norm"]))


def block_sum(lanes):
    """[.., 256] lane values -> the workgroup's sum, in the values' dtype: per wavefront of 64 lanes the butterfly v += v[lane ^ s], s = 32 .. 1, then
    ((w0 + w1) + w2) + w3"""
    v = lanes.reshape(*lanes.shape[:-1], 4, 64)
    lane = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ s]
    w = v[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def chunk_partials(g):
    """one tensor's chunk partials in g's dtype: chunks of 1024 consecutive elements (the last may be short: padded with zeros, whose squares add exactly
    nothing), lane t the chain from 0 over the elements t, t + 256, t + 512, t + 768"""
    g = np.asarray(g).reshape(-1)
    C = -(-g.size // CHUNK)
    x = np.zeros(C * CHUNK, g.dtype)
    x[: g.size] = g
    sq = (x * x).reshape(C, CHUNK // LANES, LANES)
    s = np.zeros((C, LANES), g.dtype)
    for j in range(CHUNK // LANES):
        s = s + sq[:, j, :]
    return block_sum(s)


def total_sumsq(partials):
    """the second level: lane t the chain from 0 over the partials t, t + 256, .., then the same block sum"""
    partials = np.asarray(partials).reshape(-1)
    J = max(1, -(-partials.size // LANES))
    q = np.zeros(J * LANES, partials.dtype)
    q[: partials.size] = partials
    q = q.reshape(J, LANES)
    s = np.zeros(LANES, partials.dtype)
    for j in range(J):
        s = s + q[j]
    return block_sum(s)


def n_partials(case):
    return sum(-(-t["g"].size // CHUNK) for net in case["nets"] for t in net)


def clip(norm, max_grad_norm, dt, defect=None):
    c = dt(max_grad_norm) / (norm if defect == "no_1e6_in_coef" else norm + dt(1e-6))
    return c if defect == "coef_not_clamped" else (dt(1.0) if c > dt(1.0) else c)


def twin_norm(nets, defect=None):
    """float32 total norm of the tensors of ``nets`` in the header's order"""
    parts = [chunk_partials(t["g"].astype(np.float32)) for net in nets for i, t in enumerate(net) if not (defect == "no_biases_in_norm" and i % 2)]
    return np.sqrt(total_sumsq(np.concatenate(parts)))


def step(case, dtype, defect=None):
    """One clip + Adam step of the case in ``dtype``: ``{"total_norm", "coef", "nets": [[{"p", "m", "v"}, ..], ..]}``.  float64: the reference (no defect);
    float32: the twin, optionally with a planted defect."""
    dt = np.dtype(dtype).type
    nets = case["nets"]
    if dt is np.float64:
        assert defect is None
        b1, b2, t = float(case["beta1"]), float(case["beta2"]), int(case["t"])
        sc = dict(beta2=b2, w1=1.0 - b1, w2=1.0 - b2, step_size=float(case["lr"]) / (1.0 - b1 ** t), sqrt_bc2=math.sqrt(1.0 - b2 ** t), eps=float(case["eps"]),
                  max_grad_norm=float(case["max_grad_norm"]))
        norm = math.sqrt(sum(float(np.sum(t_["g"].astype(np.float64) ** 2)) for net in nets for t_ in net))
        coefs = [clip(norm, sc["max_grad_norm"], dt)] * len(nets)
    else:
        sc = scalars(case)
        if defect == "no_bias_correction":
            sc["step_size"], sc["sqrt_bc2"] = np.float32(case["lr"]), np.float32(1.0)
        if defect == "beta2_for_first_moment":
            sc["w1"] = sc["w2"]
        norm = twin_norm(nets, defect)
        coefs = [clip(norm, sc["max_grad_norm"], dt, defect)] * len(nets)
        if defect == "norm_per_network":
            coefs = [clip(twin_norm([net]), sc["max_grad_norm"], dt) for net in nets]
    out = {"total_norm": dt(norm), "coef": dt(coefs[0]), "nets": []}
    with np.errstate(invalid="ignore", divide="ignore"):
        for net, coef in zip(nets, coefs):
            res = []
            for t_ in net:
                g, p, m, v = (t_[k].astype(dt) for k in ("g", "p", "m", "v"))
                gc = g * coef
                m = m + (gc - m) * sc["w1"]
                v = sc["beta2"] * v + (sc["w2"] * gc) * gc
                if defect == "eps_in_sqrt":
                    den = np.sqrt(v + sc["eps"]) / sc["sqrt_bc2"]
                elif defect == "sqrt_bc2_on_eps":
                    den = (np.sqrt(v) + sc["eps"]) / sc["sqrt_bc2"]
                else:
                    den = np.sqrt(v) / sc["sqrt_bc2"] + sc["eps"]
                p = p - sc["step_size"] * (m / den)
                assert p.dtype == dt and m.dtype == dt and v.dtype == dt
                res.append({"p": p, "m": m, "v": v})
            out["nets"].append(res)
    return out


def bounds(case):
    """The derived bounds on |float32 - float64| (module docstring): ``{"total_norm", "coef", "nets": [[{"p", "m", "v"}, ..], ..]}``."""
    b1, b2, t = float(case["beta1"]), float(case["beta2"]), int(case["t"])
    w1, w2, ss, sb, eps, mg = 1.0 - b1, 1.0 - b2, float(case["lr"]) / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t), float(case["eps"]), float(case["max_grad_norm"])
    ref = step(case, np.float64)
    norm = float(ref["total_norm"])
    D = 14 + -(-n_partials(case) // LANES) + 9
    r_n = (D / 2 + 1) * U
    r_c = r_n + 3 * U
    c64 = mg / (norm + 1e-6)
    e_c = 0.0 if c64 * (1.0 - r_c) > 1.0 else r_c * c64
    coef = float(ref["coef"])
    out = {"total_norm": SECOND * r_n * norm, "coef": SECOND * e_c, "nets": []}
    for net, rnet in zip(case["nets"], ref["nets"]):
        res = []
        for t_, r_ in zip(net, rnet):
            g, p, m, v = (np.abs(t_[k].astype(np.float64)) for k in ("g", "p", "m", "v"))
            gc = g * coef
            e_g = g * e_c + U * gc
            m1, v1 = np.abs(r_["m"]), r_["v"]
            e_m = w1 * e_g + U * (3 * w1 * (gc + m) + m + w1 * (gc + m))
            e_v = 2 * U * b2 * v + 3 * U * w2 * gc * gc + 2 * w2 * gc * e_g + U * v1
            r = np.sqrt(v1)
            e_r = np.where(v1 > 0, e_v / (2 * np.where(v1 > 0, r, 1.0)), 0.0) + U * r
            q = r / sb
            e_q = e_r / sb + 2 * U * q
            den = q + eps
            e_den = e_q + U * eps + U * den
            with np.errstate(invalid="ignore", divide="ignore"):
                quo = m1 / den
                e_quo = e_m / den + m1 * e_den / den ** 2 + U * quo
            upd = ss * quo
            e_upd = ss * e_quo + 2 * U * upd
            e_p = e_upd + U * (p + upd)
            res.append({"p": SECOND * e_p, "m": SECOND * e_m, "v": SECOND * e_v})
        out["nets"].append(res)
    return out


def compare(got, case, factor=1.0, ref=None):
    """``got`` (a ``step`` result, or the device's numbers in the same form) against the float64 reference: the worst ratio |got - ref64| / (factor * bound) per
    kind ``{"total_norm", "coef", "p", "m", "v"}`` -- a kind passes when its ratio is <= 1.  An element whose bound is 0 must be exact (ratio inf otherwise); a NaN
    in ``got`` where the reference is finite is a miss.  ``ref``: another result to compare with instead of the reference (two routes that are each within one
    bound of float64 agree within ``factor`` = 2)."""
    ref, bnd = ref if ref is not None else step(case, np.float64), bounds(case)

    def ratio(x, r, b):
        x, r, b = np.asarray(x, np.float64), np.asarray(r, np.float64), np.asarray(b, np.float64) * factor
        err = np.abs(x - r)
        err = np.where(np.isnan(err), np.inf, err)
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(err == 0, 0.0, np.where(b > 0, err / np.where(b > 0, b, 1.0), np.inf))
        return float(np.max(q)) if q.size else 0.0

    worst = {"total_norm": ratio(got["total_norm"], ref["total_norm"], bnd["total_norm"]), "coef": ratio(got["coef"], ref["coef"], bnd["coef"])}
    for k in KEYS:
        worst[k] = max(ratio(a[k], r[k], b[k]) for gn, rn, bn in zip(got["nets"], ref["nets"], bnd["nets"]) for a, r, b in zip(gn, rn, bn))
    return worst


def same_bits(got, want):
    """every number of two ``step`` results as float32 words"""
    def w(x):
        return np.asarray(x, np.float32).reshape(-1).view(np.uint32)

    ok = np.array_equal(w(got["total_norm"]), w(want["total_norm"])) and np.array_equal(w(got["coef"]), w(want["coef"]))
    return ok and all(np.array_equal(w(a[k]), w(b[k])) for gn, wn in zip(got["nets"], want["nets"]) for a, b in zip(gn, wn) for k in KEYS)


def make_case(sizes, seed, t=1, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=1.0, grad_norm=None, zero_grad=False, fresh=False):
    """A synthetic case: ``sizes`` = per network the tensors' element counts (weight, bias, ..).  Parameters ~ 0.1 N(0, 1); gradients N(0, 1) times
    10^U(-6, -1) per element (so that eps matters for some and not for others), scaled to the total norm ``grad_norm`` when given; moments as after earlier steps
    (``fresh``: zeros, as at t = 1).  ``zero_grad``: all gradients zero."""
    rng = np.random.default_rng(seed)
    nets = []
    for net in sizes:
        ts = []
        for n in net:
            g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, -1, n)).astype(np.float32)
            if zero_grad:
                g[:] = 0.0
            m = np.zeros(n, np.float32) if fresh else (0.3 * rng.standard_normal(n) * 10.0 ** rng.uniform(-6, -1, n)).astype(np.float32)
            v = np.zeros(n, np.float32) if fresh else ((rng.standard_normal(n) * 10.0 ** rng.uniform(-6, -1, n)) ** 2 * 0.1).astype(np.float32)
            ts.append({"p": (0.1 * rng.standard_normal(n)).astype(np.float32), "g": g, "m": m, "v": v})
        nets.append(ts)
    case = dict(nets=nets, lr=lr, beta1=beta1, beta2=beta2, eps=eps, max_grad_norm=max_grad_norm, t=t)
    if grad_norm is not None and not zero_grad:
        norm = float(step(case, np.float64)["total_norm"])
        for net in nets:
            for t_ in net:
                t_["g"] = (t_["g"].astype(np.float64) * (grad_norm / norm)).astype(np.float32)
    return case
