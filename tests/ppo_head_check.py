"""The yardstick of the clip-PPO loss head (sigmaenv_ppo_head, sigmarl_amd/csrc/sigmaenv_ppo.inc; the formulas are the contract in include/sigmaenv.h): a plain
helper module like policy_head_check.py, imported by the tests (tests/test_ppo_head_check.py runs it on the host, tests/test_gpu_ppo_update.py on the device's tensors).

``head(case, np.float64)`` is the reference: the formulas in float64 with the gradients taken ANALYTICALLY (``torch_head`` holds the same formulas in torch, whose
float64 autograd the host test cross-checks them against).  ``head(case, np.float32)`` is the twin: the kernel's operations in the kernel's order in float32,
including the order of its sums (``ordered_sum``).  The entropy sample's draws are recomputed from the key with policy_head_check's generator (draw ids 7300 / 7301).

The criterion (``compare``), built like policy_head_check.compare.  Per element,

    |dev - ref64| <= MARGIN * c * 2^-23 * S

with S the sum of the magnitudes of everything that enters the element (``head`` forms it next to the value, float64 only: every added term, every factor's own
rounding seen through the product, the amplification 1 / (1 - y^2) of atanh, 1 / sigma of the standardised residual ...), c MEASURED on the float32 twin against
float64 over the rows of the case -- never on the kernel -- and MARGIN = 4 (the device's expf / logf / log1pf / tanhf / sincosf need not round as numpy's do).  One
constant per output kind: ``dloc``, ``draw`` (the two halves of dout_actor), ``dcritic``, and the four per-row terms the scalars sum (``obj``, ``lps``, ``sl1``,
``lw``), which the device never shows: for a scalar mean the bound is

    |coef| / (M N) * (MARGIN * c_term * 2^-23 * sum_rows S + (count + 3) * 2^-23 * sum_rows |term|)

``count`` = the roundings of the ordered sum an element passes through (``sum_depth``), + 3 for the scalings that follow.  A case of fewer than FULL_ROWS rows also
takes the constants of the calibration case (``calibration``: the twin on a fixed synthetic case of 1536 rows), as policy_head_check does.

Branches.  min(g1, g2) and the smooth-L1 term are continuous, but the gradient through the objective jumps where lw crosses a clip bound.  A row whose float64 lw lies
within its own bound MARGIN * c_lw * 2^-23 * S_lw of log1p(+-eps) may take either side: its dout_actor elements pass if they pass against either branch, and it may
move clip_fraction by 1 / (M N).  (On a tie INSIDE the band clamp(lw) == lw bit for bit, so g1 == g2 exactly and the unclamped branch is taken: no ambiguity.)

sigma = max(softplus(.) + 0.01, 1e-4): softplus >= 0, so the 1e-4 floor never acts on finite input; what "the floor" means for a row is the 0.01 floor of
biased_softplus (raw << 0: sigma = 0.01 to rounding, d sigma / d raw -> 0), which ``populations`` counts.
"""
from __future__ import annotations

import math

import numpy as np

import policy_head_check as phc

MARGIN = 4.0
FULL_ROWS = 1000
U23 = 2.0 ** -23
ENTROPY_DRAWS = (7300, 7301)  # sigmaenv_dist.h: DRAW_ENTROPY, + 1
BIAS, LOG_SQRT_2PI, LOG2 = phc.BIAS, phc.LOG_SQRT_2PI, phc.LOG2
RESULT = ("loss_objective", "loss_entropy", "loss_critic", "entropy", "clip_fraction", "kl_approx")
DEFECTS = ("ratio_clip", "tie_clamped_neg", "no_dsigma_draw", "entropy_no_sigma_grad", "smooth_l1_half", "critic_mean", "index_on_out")
# faults of the final sum (``ordered_sum``): they show only past 64 (first_64: the workgroups from 64 on are never read) or 32 (stride_32: lane k also adds the
# workgroups k + 32, k + 96, .., which belong to lane k + 32) workgroups, so they are planted at sizes of their own (tests/test_ppo_head_check.py)
SUM_DEFECTS = ("first_64", "stride_32")


def clip_bounds(eps):
    """(log1p(-eps), log1p(eps)) of the float32 eps, each rounded to float32 once -- what the library forms on the host"""
    e = float(np.float32(eps))
    return np.float32(math.log1p(-e)), np.float32(math.log1p(e))


def wave_sum(v):
    """the butterfly v += v[lane ^ s], s = 32 .. 1, over the last axis (64 lanes), in v's dtype; every lane ends with the same value: lane 0 is returned"""
    lane = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ s]
    return v[..., 0]


def ordered_sum(t, defect=None):
    """The device's sum of one value per row, in t's dtype: rows padded with zeros to workgroups of 256, per wavefront the butterfly, per workgroup
    ((w0 + w1) + w2) + w3, then one wavefront -- lane k the chain over the workgroups k, k + 64, .. from 0 -- and the butterfly.  ``defect``: one of SUM_DEFECTS."""
    t = np.asarray(t).reshape(-1)
    dt = t.dtype.type
    G = -(-t.size // 256)
    p = np.zeros(G * 256, t.dtype)
    p[: t.size] = t
    w = wave_sum(p.reshape(G, 4, 64))
    g = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    J = -(-G // 64)
    q = np.zeros(J * 64, t.dtype)
    q[:G] = g
    q = q.reshape(J, 64)
    v = np.zeros(64, t.dtype)
    if defect == "stride_32":  # lane k: the workgroups k, k + 32, k + 64, ..
        h = np.zeros(2 * J * 64 + 32, t.dtype)
        h[:G] = g
        for j in range(2 * J):
            v = (v + h[32 * j:32 * j + 64]).astype(dt)
        return dt(wave_sum(v))
    for j in range(1 if defect == "first_64" else J):
        v = (v + q[j]).astype(dt)
    return dt(wave_sum(v))


def sum_depth(rows):
    """the roundings an element passes through in ``ordered_sum``: 6 + 3 + ceil(G / 64) + 6"""
    G = -(-rows // 256)
    return 6 + 3 + -(-G // 64) + 6


def draws(case, dtype=np.float64, magnitude=False):
    """(z [M, N, 2]) of the entropy sample: key (seed, counter, env = frame, agent), draws 7300 / 7301"""
    M, N = case["out"].shape[:2]
    f = np.repeat(np.asarray(case["index"], np.int64), N).astype(np.uint32)
    n = np.tile(np.arange(N), M).astype(np.uint32)
    z = phc.normals(case["seed"], case["counter"], f, n, ENTROPY_DRAWS, dtype, magnitude)
    return np.stack(z, -1).reshape(M, N, 2)


def head(case, dtype=np.float64, defect=None):
    """The head on ``case`` = dict(out [M, N, 4], value [M], index [M], action [F, N, 2], sample_log_prob / advantage / value_target [F, N] (float32 arrays), low,
    high, clip_epsilon, entropy_coeff, critic_coeff, seed, counter).  Returns dict(dout_actor [M, N, 4], dout_critic [M], result {name: scalar}, terms {obj, lps, sl1,
    lw: [M, N]}, and for the branches lw, g1, g2, A, e, sigma, y, dlw_on); float64 also S_* (the magnitudes) and alt_dout_actor (the other side of the clip branch).
    ``defect``: one of DEFECTS, planted (the twin only)."""
    f = dtype
    out = np.asarray(case["out"], np.float32)
    M, N = out.shape[:2]
    idx = np.asarray(case["index"], np.int64)
    o = (out[idx % M] if defect == "index_on_out" else out).astype(f)
    v = np.asarray(case["value"], np.float32).astype(f).reshape(M, 1)
    act = np.asarray(case["action"], np.float32)[idx].astype(f)
    old, A, vt = (np.asarray(case[k], np.float32)[idx].astype(f) for k in ("sample_log_prob", "advantage", "value_target"))
    low, high = np.asarray(case["low"], np.float32).astype(f), np.asarray(case["high"], np.float32).astype(f)
    lo32, hi32 = clip_bounds(case["clip_epsilon"])
    lo, hi = f(lo32), f(hi32)
    R = M * N
    ce, cc = np.float32(case["entropy_coeff"]), np.float32(case["critic_coeff"])
    if f == np.float32:  # 1 / (M N) and its products with the coefficients: rounded once each, as the library's host code forms them
        inv = np.float32(1.0) / np.float32(R)
        ce_inv, cc_inv = ce * inv, cc * inv
    else:                # the reference: the exact mean
        inv = 1.0 / R
        ce_inv, cc_inv = float(ce) / R, float(cc) / R
    z = draws(case, f)
    loc, raw = o[..., :2], o[..., 2:]
    w = raw + f(BIAS)
    s0 = phc.raw_scale_of(raw, f)
    sig = np.maximum(s0, f(1e-4))
    with np.errstate(over="ignore"):
        dsdr = np.where(s0 < f(1e-4), f(0.0), f(1.0) / (f(1.0) + np.exp(-w)))
    h = f(0.5) * (high - low)
    logh, logs = np.log(h), np.log(sig)
    EPS = f(np.float32(1e-6))
    y = np.minimum(np.maximum((act - low) / h - f(1.0), f(-1.0) + EPS), f(1.0) - EPS)
    x = f(0.5) * (np.log1p(y) - np.log1p(-y))
    q = (x - loc) / sig
    lpd, sp = phc.log_density(q, logs, x, f)
    lpd = lpd - logh
    lp = lpd[..., 0] + lpd[..., 1]
    xs = loc + sig * z
    lpsd, sps = phc.log_density(z, logs, xs, f)
    lpsd = lpsd - logh
    lps = lpsd[..., 0] + lpsd[..., 1]
    lw = lp - old
    cl = np.minimum(np.maximum(lw, lo), hi)
    with np.errstate(over="ignore"):
        ratio = np.exp(lw)
        rc = np.minimum(np.maximum(ratio, lo), hi) if defect == "ratio_clip" else np.exp(cl)
    g1, g2 = ratio * A, rc * A
    on = g1 <= g2
    if defect == "tie_clamped_neg":
        on = (g1 < g2) | ((g1 == g2) & (A >= 0))
    dlw = np.where(on, g1, f(0.0))
    e = v - vt
    ae = np.abs(e)
    beta = f(0.5) if defect == "smooth_l1_half" else f(1.0)
    sl1 = np.where(ae < beta, f(0.5) * e * e / beta if defect == "smooth_l1_half" else f(0.5) * e * e, ae - f(0.5) * beta)
    de = np.minimum(np.maximum(e, -beta), beta) / beta if defect == "smooth_l1_half" else np.minimum(np.maximum(e, f(-1.0)), f(1.0))
    clipped = (cl != lw).astype(f)
    th2 = f(2.0) * np.tanh(xs)

    def grads(dlw_):
        wobj = (-inv * dlw_)[..., None]
        dl = wobj * (q / sig) + ce_inv * th2
        ent = f(0.0) if defect == "entropy_no_sigma_grad" else ce_inv * (th2 * z - f(1.0) / sig)
        dsig = wobj * ((q * q - f(1.0)) / sig) + ent
        dr = dsig if defect == "no_dsigma_draw" else dsig * dsdr
        return np.concatenate([dl, dr], -1), dsig

    dout_a, dsig = grads(dlw)
    if f == np.float32:
        s = np.zeros(M, f)
        for n in range(N):
            s = (s + de[:, n]).astype(f)
        dout_c = cc_inv * s
        S = {k: ordered_sum(t.astype(f), defect if defect in SUM_DEFECTS else None) for k, t in (("obj", np.minimum(g1, g2)), ("lps", lps), ("sl1", sl1), ("clip", clipped), ("kl", -lw))}
    else:
        dout_c = cc_inv * de.sum(1)
        S = {k: float(t.sum()) for k, t in (("obj", np.minimum(g1, g2)), ("lps", lps), ("sl1", sl1), ("clip", clipped), ("kl", -lw))}
    if defect == "critic_mean":
        dout_c = dout_c / f(N)
    entropy = -(f(S["lps"]) * inv)
    result = dict(loss_objective=-(f(S["obj"]) * inv), loss_entropy=-(f(ce) * entropy), loss_critic=f(cc) * (f(S["sl1"]) * inv), entropy=entropy,
                  clip_fraction=f(S["clip"]) * inv, kl_approx=f(S["kl"]) * inv)
    r = dict(dout_actor=dout_a, dout_critic=dout_c, result=result, terms=dict(obj=np.minimum(g1, g2), lps=lps, sl1=sl1, lw=lw), lw=lw, g1=g1, g2=g2, A=A, e=e,
             sigma=sig, y=y, dlw_on=on, lo=lo, hi=hi, rows=R, inv=float(inv), ce=float(ce), cc=float(cc), clipped=int((cl != lw).sum()))
    if f != np.float64:
        return r
    # ---- the magnitudes (float64 reference only), in units of one float32 rounding
    a = np.abs
    zm = draws(case, magnitude=True)
    dx = (a(act - low) / h + 1.0 + a(y)) / (1.0 - y * y) + a(x)                 # atanh(y): the roundings of y seen through 1 / (1 - y^2), and its own
    qm = (dx + a(loc) + a(x)) / sig + 3.0 * a(q)                                # q = (x - loc) / sigma (sigma carries a relative rounding or two of its own)
    S_lp = (a(q) * qm + 0.5 * q * q + a(logs) + 1.0 + LOG_SQRT_2PI + 2 * LOG2 + 2 * a(x) + 2 * a(sp) + 2 * dx + a(logh)).sum(-1)
    S_lw = S_lp + a(lp) + a(old)
    gm = np.maximum(a(g1), a(g2))
    S_obj = gm * (S_lw + 3.0)
    dxs = a(loc) + 2 * sig * zm + a(xs)                                          # x' = loc + sigma z
    S_lps = (0.5 * z * z + a(z) * zm + a(logs) + 1.0 + LOG_SQRT_2PI + 2 * LOG2 + 2 * a(xs) + 2 * a(sps) + 2 * dxs + a(logh)).sum(-1)
    S_sl1 = np.minimum(ae, 1.0) * (a(v) + a(vt)) + 2 * sl1 + 0.5 * (ae >= 1.0)
    r["S_terms"] = dict(obj=S_obj, lps=S_lps, sl1=S_sl1, lw=S_lw)
    sech2 = 1.0 - np.tanh(xs) ** 2

    def mags(dlw_):
        g = a(dlw_)[..., None]
        Sg = (a(dlw_) * (S_lw + 3.0))[..., None]  # the magnitude of g1 = exp(lw) A
        t1 = float(inv) * (Sg * a(q) / sig + g * (qm / sig + 3 * a(q) / sig))
        t2 = a(ce_inv) * (3 * a(th2) + 2 * sech2 * dxs)
        S_dl = t1 + t2 + a(-inv * dlw_[..., None] * (q / sig)) + a(ce_inv * th2)
        u1 = float(inv) * (Sg * a(q * q - 1.0) / sig + g * (2 * a(q) * qm + 4 * (q * q + 1.0)) / sig)
        u2 = a(ce_inv) * (4 * a(th2) * a(z) + 2 * sech2 * dxs * a(z) + a(th2) * zm + 4.0 / sig)
        S_ds = u1 + u2 + a(-inv * dlw_[..., None] * ((q * q - 1.0) / sig)) + a(ce_inv * (th2 * z - 1.0 / sig))
        ds = -inv * dlw_[..., None] * ((q * q - 1.0) / sig) + ce_inv * (th2 * z - 1.0 / sig)
        S_dr = S_ds * dsdr + a(ds) * dsdr * (4.0 + a(raw) + BIAS)
        return np.concatenate([S_dl, S_dr], -1)

    r["S_dout_actor"] = mags(dlw)
    alt = np.where(on, 0.0, g1)  # the other side of the clip branch
    r["alt_dout_actor"], r["S_alt_dout_actor"] = grads(alt)[0], mags(alt)
    r["S_dout_critic"] = a(cc_inv) * ((a(v) + a(vt)).sum(1) + (N + 3) * a(de).sum(1))
    return r


def populations(ref):
    """How many rows of a case lie in each branch of the head (from the float64 reference alone)"""
    lw, A, e = ref["lw"], ref["A"], ref["e"]
    lo, hi = float(ref["lo"]), float(ref["hi"])
    inside, above, below = (lw > lo) & (lw < hi), lw >= hi, lw <= lo
    return dict(inside_pos=int((inside & (A > 0)).sum()), inside_neg=int((inside & (A < 0)).sum()), above_pos=int((above & (A > 0)).sum()),
                above_neg=int((above & (A < 0)).sum()), below_pos=int((below & (A > 0)).sum()), below_neg=int((below & (A < 0)).sum()),
                e_small=int((np.abs(e) < 1).sum()), e_large=int((np.abs(e) >= 1).sum()), sigma_floor=int((ref["sigma"] < 0.0101).sum()),
                y_max=float(np.abs(ref["y"]).max()))


def _ratio(got, ref, S):
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(np.asarray(got, np.float64) - ref)
        return np.where(S > 0, err / (U23 * np.where(S > 0, S, 1.0)), np.where(err == 0, 0.0, np.inf))


def constants(case, ref=None):
    """The twin's measured constants over the rows of ``case``: dict(dloc, draw, dcritic, obj, lps, sl1, lw)"""
    ref = ref if ref is not None else head(case)
    twin = head(case, np.float32)
    ra = _ratio(twin["dout_actor"], ref["dout_actor"], ref["S_dout_actor"])
    c = dict(dloc=float(ra[..., :2].max()), draw=float(ra[..., 2:].max()), dcritic=float(_ratio(twin["dout_critic"], ref["dout_critic"], ref["S_dout_critic"]).max()))
    for k in ("obj", "lps", "sl1", "lw"):
        c[k] = float(_ratio(twin["terms"][k], ref["terms"][k], ref["S_terms"][k]).max())
    return c


_CALIBRATION = {}


def calibration():
    """The constants of the calibration case (``synthetic_case()`` at its defaults: 512 slots x 3 agents), for cases of fewer than FULL_ROWS rows"""
    if not _CALIBRATION:
        _CALIBRATION.update(constants(synthetic_case()))
    return _CALIBRATION


def constants_in_force(case, ref):
    """the constants ``compare`` holds ``case`` to: the twin's over its rows, and the calibration case's for fewer than FULL_ROWS rows"""
    c = constants(case, ref)
    if ref["rows"] < FULL_ROWS:
        c = {k: max(v, calibration()[k]) for k, v in c.items()}
    return c


def in_the_band(ref, c):
    """[M, N] bool: the rows whose float64 lw lies within its own bound of a clip bound (module docstring, Branches)"""
    tol = MARGIN * c["lw"] * U23 * ref["S_terms"]["lw"]
    return (np.abs(ref["lw"] - float(ref["lo"])) <= tol) | (np.abs(ref["lw"] - float(ref["hi"])) <= tol)


def clear_of_the_band(case, shift=0.05):
    """``case`` with every row of the branch band moved out of it, away from zero, through its ``sample_log_prob`` (a frame picked twice has one record and the same
    outputs in both slots: its slots move together).  Returns (case, reference, constants, the rows moved); the caller asserts that ``in_the_band`` is empty.  With no
    row in the band a kernel that meets the criterion of ``lw`` clips exactly the rows the float64 reference clips."""
    case = dict(case, sample_log_prob=np.array(case["sample_log_prob"], np.float32))
    moved = 0
    for _ in range(4):
        ref = head(case)
        c = constants_in_force(case, ref)
        amb = in_the_band(ref, c)
        if not amb.any():
            break
        for m, n in np.argwhere(amb):
            case["sample_log_prob"][case["index"][m], n] -= np.float32(math.copysign(shift, ref["lw"][m, n]))
        moved += int(amb.sum())
    return case, ref, c, moved


def compare(dout_actor, dout_critic, result, case, what=""):
    """The criterion of the module docstring: the device's (or a twin's) outputs against ``head(case, float64)``.  ``result``: the six scalars in RESULT order.
    Returns the figures; ``ok`` says whether everything passed."""
    ref = head(case)
    c = constants_in_force(case, ref)
    M, N = ref["lw"].shape
    r = dict(what=what, rows=ref["rows"], c=c)
    da = np.asarray(dout_actor, np.float64).reshape(M, N, 4)
    ck = np.array([c["dloc"], c["dloc"], c["draw"], c["draw"]])
    main, alt = _ratio(da, ref["dout_actor"], ref["S_dout_actor"]) / ck, _ratio(da, ref["alt_dout_actor"], ref["S_alt_dout_actor"]) / ck
    # rows whose lw is within its own bound of a clip bound may take either side of the branch
    amb = in_the_band(ref, c)
    use = np.where(amb[..., None], np.minimum(main, alt), main)
    r["ambiguous_rows"] = int(amb.sum())
    r["dloc"], r["draw"] = float(use[..., :2].max()), float(use[..., 2:].max())
    r["dcritic"] = float((_ratio(np.asarray(dout_critic, np.float64).reshape(M), ref["dout_critic"], ref["S_dout_critic"]) / c["dcritic"]).max())
    ok = bool(np.isfinite(da).all() and max(r["dloc"], r["draw"], r["dcritic"]) <= MARGIN)
    # the scalars
    res = {k: float(v) for k, v in zip(RESULT, np.asarray(result, np.float64).reshape(-1)[:6])}
    cnt, inv, T, S = sum_depth(ref["rows"]) + 3, ref["inv"], ref["terms"], ref["S_terms"]

    def bound(term, coef):
        return abs(coef) * inv * U23 * (MARGIN * c[term] * float(S[term].sum()) + cnt * float(np.abs(T[term]).sum()))

    bounds = dict(loss_objective=bound("obj", 1.0), entropy=bound("lps", 1.0), loss_entropy=bound("lps", ref["ce"]) + abs(float(ref["result"]["loss_entropy"])) * U23,
                  loss_critic=bound("sl1", ref["cc"]), kl_approx=bound("lw", 1.0), clip_fraction=(r["ambiguous_rows"] + cnt * U23 * ref["rows"]) * inv)
    r["scalars"] = {}
    for k in RESULT:
        err = abs(res[k] - float(ref["result"][k]))
        r["scalars"][k] = dict(dev=res[k], ref=float(ref["result"][k]), err=err, bound=bounds[k])
        ok &= bool(np.isfinite(res[k]) and err <= bounds[k])
    r["ok"] = ok
    return r, ref


def check(dout_actor, dout_critic, result, case, what=""):
    r, ref = compare(dout_actor, dout_critic, result, case, what)
    print(what, {k: (round(r[k], 3) if isinstance(r[k], float) else r[k]) for k in ("rows", "ambiguous_rows", "dloc", "draw", "dcritic")},
          {k: (f"{v['err']:.3g}", f"{v['bound']:.3g}") for k, v in r["scalars"].items()})
    assert r["ok"], f"{what}: the PPO head misses its criterion: {r}"
    return r, ref


def twin_outputs(case, defect=None):
    """(dout_actor, dout_critic, result in RESULT order) of the float32 twin, optionally with a planted defect"""
    t = head(case, np.float32, defect)
    return t["dout_actor"], t["dout_critic"], np.array([t["result"][k] for k in RESULT], np.float32)


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
LOW, HIGH = (-1.0, -0.6), (1.0, 0.6)


def records_for(out64, value64, index, F, N, seed, low=LOW, high=HIGH):
    """Records [F, ..] that populate every branch for the minibatch (out64 [M, N, 4], value64 [M]: the float64 outputs the networks will give, or synthetic ones) at
    the frames ``index``: recorded actions with |y| <= 0.999, sample_log_prob = the reference's logp + a log-ratio that is inside the clip band (+-0.2: |lw| < 0.15)
    for half of the rows and outside (0.3 <= |lw| < 0.8) for the rest, advantages of both signs, value targets with |e| on both sides of 1.  Frames that the
    index does not pick hold arbitrary finite values; a frame picked twice takes the values made for its LAST slot."""
    g = np.random.default_rng(seed)
    M = len(index)
    low, high = np.asarray(low, np.float32), np.asarray(high, np.float32)
    h = 0.5 * (high.astype(np.float64) - low)
    act = np.zeros((F, N, 2), np.float32)
    yy = g.uniform(-0.999, 0.999, (F, N, 2))
    act[:] = (low + (yy + 1.0) * h).astype(np.float32)
    adv = (g.standard_normal((F, N)) * 1.5).astype(np.float32)
    adv[np.abs(adv) < 0.05] = 0.5
    old = g.standard_normal((F, N)).astype(np.float32)
    vt = g.standard_normal((F, N)).astype(np.float32)
    case = dict(out=np.asarray(out64, np.float32), value=np.asarray(value64, np.float32), index=np.asarray(index), action=act, sample_log_prob=old, advantage=adv,
                value_target=vt, low=low, high=high, clip_epsilon=0.2, entropy_coeff=0.0, critic_coeff=1.0, seed=0, counter=0)
    lp = head(case)["lw"] + old[np.asarray(index)]  # the reference's logp of the recorded actions
    mag = np.where(g.random((M, N)) < 0.5, g.uniform(0.0, 0.15, (M, N)), g.uniform(0.3, 0.8, (M, N)))
    lw = mag * np.where(g.random((M, N)) < 0.5, -1.0, 1.0)
    e = np.where(g.random((M, N)) < 0.5, g.uniform(0.02, 0.9, (M, N)), g.uniform(1.1, 3.0, (M, N))) * np.where(g.random((M, N)) < 0.5, -1.0, 1.0)
    for m, fr in enumerate(np.asarray(index)):
        old[fr] = (lp[m] - lw[m]).astype(np.float32)
        vt[fr] = (np.asarray(value64, np.float64).reshape(-1)[m] - e[m]).astype(np.float32)
    return dict(action=act, sample_log_prob=old, advantage=adv, value_target=vt)


def synthetic_case(M=512, N=3, F=700, seed=1, entropy_coeff=0.01, critic_coeff=1.0, clip_epsilon=0.2, counter=3, low=LOW, high=HIGH, floor_rows=8, index=None):
    """A case on synthetic network outputs: raw ~ N(0, 1.5) (``floor_rows`` slots at raw = -40: sigma at its 0.01 floor), loc = x - sigma q with q ~ N(0, 1.2) so
    that the standardised residuals are moderate, ``index`` (default) = a sample of the F frames with duplicates."""
    g = np.random.default_rng(seed)
    if index is None:
        index = g.integers(0, F, M).astype(np.int32)
        index[:2] = index[min(2, M - 1)]  # (a frame picked three times for certain)
    index = np.asarray(index, np.int32)
    M = len(index)
    # the outputs are made per FRAME, as a network's are: the slots of a frame picked twice agree
    raw = g.standard_normal((F, N, 2)) * 1.5
    raw[g.choice(index, min(floor_rows, M), replace=False)] = -40.0
    outF = np.zeros((F, N, 4), np.float32)
    outF[..., 2:] = raw
    valueF = g.standard_normal(F).astype(np.float32)
    rec = records_for(outF[index], valueF[index], index, F, N, seed + 1, low, high)
    # loc from the recorded action's x: a second pass, now that the actions exist
    lo_, hi_ = np.asarray(low, np.float64), np.asarray(high, np.float64)
    hh = 0.5 * (hi_ - lo_)
    y = np.clip((rec["action"].astype(np.float64) - lo_) / hh - 1.0, -1 + 1e-6, 1 - 1e-6)
    sig = phc.scale_of(outF[..., 2:], np.float64)
    outF[..., :2] = (np.arctanh(y) - sig * g.standard_normal((F, N, 2)) * 1.2).astype(np.float32)
    out, value = outF[index], valueF[index]
    rec = records_for(out, value, index, F, N, seed + 1, low, high)
    return dict(out=out, value=value, index=index, low=np.asarray(low, np.float32), high=np.asarray(high, np.float32), clip_epsilon=clip_epsilon,
                entropy_coeff=entropy_coeff, critic_coeff=critic_coeff, seed=1234567, counter=counter, **rec)


# ---- past 64 workgroups: the second and third term of a lane's chain in the final sum ---------------------------------------------------------------
BIG_N = 16
BIG_M = {1024: (16384, 64, 1), 1025: (16400, 65, 2), 2049: (32784, 129, 3)}  # M -> (rows, workgroups, the longest chain of a lane: lane 0's)
BIG_PATTERNS = ("duplicates", "permutation")
_BIG = {}


def big_case(M, pattern):
    """The case of M frames x BIG_N agents over F = M + 3 frames, its index a sample with duplicates or a cut of a permutation, cleared of the branch band:
    (case, float64 reference, constants, rows moved out of the band).  Made once per (M, pattern)."""
    if (M, pattern) not in _BIG:
        F = M + 3
        g = np.random.default_rng(1000 * M + BIG_PATTERNS.index(pattern))
        idx = (g.integers(0, F, M) if pattern == "duplicates" else g.permutation(F)[:M]).astype(np.int32)
        if pattern == "duplicates":
            idx[-1] = idx[0]
        _BIG[(M, pattern)] = clear_of_the_band(synthetic_case(N=BIG_N, F=F, seed=40 + M, index=idx, floor_rows=2))
    return _BIG[(M, pattern)]


def exact_clip_fraction(ref):
    """clip_fraction as the device forms it when it clips the rows of the float64 reference: the flags are 0 or 1, their sum is exact in any order, then one product
    with the float32 1 / R"""
    return np.float32(ref["clipped"]) * (np.float32(1.0) / np.float32(ref["rows"]))


# ---- the same formulas in torch (autograd: the host cross-check of the analytical gradients, and the whole-chain reference of the GPU test) --------------
def torch_head(out, value, index, case, z, dtype):
    """(loss_objective, loss_entropy, loss_critic) as torch scalars with a graph over ``out [M, N, 4]`` and ``value [M]`` (tensors of ``dtype``); ``index`` a long
    tensor, ``z [M, N, 2]`` the entropy draws (a constant), the records and constants from ``case``."""
    import torch

    t = lambda k: torch.from_numpy(np.asarray(case[k], np.float32)).to(dtype)[index]  # noqa: E731
    act, old, A, vt = t("action"), t("sample_log_prob"), t("advantage"), t("value_target")
    low, high = (torch.from_numpy(np.asarray(case[k], np.float32)).to(dtype) for k in ("low", "high"))
    lo, hi = (float(b) for b in clip_bounds(case["clip_epsilon"]))
    loc, raw = out[..., :2], out[..., 2:]
    sig = torch.clamp_min(torch.nn.functional.softplus(raw + BIAS) + 0.01, 1e-4)
    h = 0.5 * (high - low)
    eps = float(np.float32(1e-6))
    y = torch.clamp((act - low) / h - 1.0, -1.0 + eps, 1.0 - eps)
    x = 0.5 * (torch.log1p(y) - torch.log1p(-y))
    jac = lambda u: 2.0 * (LOG2 - u - torch.nn.functional.softplus(-2.0 * u))  # noqa: E731
    lp = (-((x - loc) ** 2) / (2 * sig ** 2) - torch.log(sig) - LOG_SQRT_2PI - jac(x) - torch.log(h)).sum(-1)
    lw = lp - old
    g1, g2 = torch.exp(lw) * A, torch.exp(torch.clamp(lw, lo, hi)) * A
    xs = loc + sig * z
    lps = (-(z ** 2) / 2 - torch.log(sig) - LOG_SQRT_2PI - jac(xs) - torch.log(h)).sum(-1)
    e = value.reshape(-1, 1) - vt
    sl1 = torch.where(e.abs() < 1.0, 0.5 * e * e, e.abs() - 0.5)
    return -torch.min(g1, g2).mean(), float(np.float32(case["entropy_coeff"])) * lps.mean(), float(np.float32(case["critic_coeff"])) * sl1.mean()
