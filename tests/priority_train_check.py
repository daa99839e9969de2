"""The yardstick of the priority module's clip-PPO loss head (sigmaenv_ppo_head_1d, sigmarl_amd/csrc/sigmaenv_ppo.inc; the formulas are the contract in
include/sigmaenv.h) and of the padded critic rows: a plain helper module like ppo_head_check.py, imported by the tests (tests/test_priority_train_check.py runs it on
the host, tests/test_gpu_priority_train.py on the device's tensors).

``head(case, np.float64)`` is the reference: ppo_head_check.head's formulas in ONE dimension with the trivial bounds -- no affine map (y = clamp(score)), no - log h --
with the gradients taken analytically (``torch_head``: the same formulas in torch, for the host's autograd cross-check).  ``head(case, np.float32)`` is the twin: the
kernel's operations in the kernel's order in float32, including the order of its sums (ppo_head_check.ordered_sum: the two heads share the reduction).  The entropy
sample is the COSINE branch of the normal pair under the draw ids 7350 / 7351 (sigmaenv_dist.h DRAW_PRIORITY_ENTROPY).

The criterion is ppo_head_check's, restated for one dimension; nothing here is a new number.  Per element |dev - ref64| <= MARGIN * c * 2^-23 * S with S the sum of
the magnitudes of everything that enters the element, c measured on the float32 twin against float64 over the rows of the case (and, below FULL_ROWS rows, on the
calibration case as well) and MARGIN = ppo_head_check.MARGIN, the allowance for the device's expf / logf / log1pf / tanhf / cosf.  What changes against the 2-D
count of roundings is the inverse transform: the recorded score is clamped and nothing else, so y is EXACT and x = atanh(y) = 0.5 (log1p(y) - log1p(-y)) carries
only the roundings of the two log1p (|log1p(y)| + |log1p(-y)| = 2 |x|: the two have opposite signs) halved, and of the subtraction: 2 |x| in all, where the 2-D head
has (|a - low| / h + 1 + |y|) / (1 - y^2) + |x|.  That is what lets the criterion tell ``clamp(score)`` from the affine map with low = -1, high = 1, whose
(score + 1) / 1 - 1 rounds the score to a multiple of 2^-24 or 2^-23.  The scalars' bounds are ppo_head_check.compare's.

An index entry outside [0, F) is part of the contract: its rows give zero gradients and add zeros to every sum, in the reference and in the twin alike.

``padded_rows``: the padded critic rows restated in numpy (element j of agent a's segment is ``j < D ? src[a * D + j] : 0``).
"""
from __future__ import annotations

import numpy as np

import policy_head_check as phc
import ppo_head_check as pc

MARGIN, FULL_ROWS, U23 = pc.MARGIN, pc.FULL_ROWS, pc.U23
ENTROPY_DRAWS = (7350, 7351)  # sigmaenv_dist.h: DRAW_PRIORITY_ENTROPY, + 1
BIAS, LOG_SQRT_2PI, LOG2 = phc.BIAS, phc.LOG_SQRT_2PI, phc.LOG2
RESULT = pc.RESULT
DEFECTS = ("affine", "draw_entropy", "sine", "entropy_clamped", "critic_sum_over_m", "grad_on_clamped", "base_advantage", "no_slope")


def draws(case, dtype=np.float64, magnitude=False, ids=ENTROPY_DRAWS, sine=False):
    """z [M, N] of the entropy sample: key (seed, counter, env = frame, agent), the cosine branch of the pair of ``ids`` (``sine``: the other branch, a defect).
    An index entry outside the records draws with frame 0 (its rows are zeroed by ``head``)."""
    M, N = case["out"].shape[:2]
    idx = _safe_index(case)[0]
    f = np.repeat(idx, N).astype(np.uint32)
    n = np.tile(np.arange(N), M).astype(np.uint32)
    z = phc.normals(case["seed"], case["counter"], f, n, ids, dtype, magnitude)
    return z[1 if sine else 0].reshape(M, N)


def _safe_index(case):
    idx = np.asarray(case["index"], np.int64)
    F = np.asarray(case["scores"]).shape[0]
    ok = (idx >= 0) & (idx < F)
    return np.where(ok, idx, 0), ok


def head(case, dtype=np.float64, defect=None):
    """The 1-D head on ``case`` = dict(out [M, N, 2], value [M], index [M], scores / score_log_prob / advantage / value_target [F, N] (float32 arrays; optionally
    base_advantage [F, N], what the defect of that name feeds the loss), clip_epsilon, entropy_coeff, critic_coeff, seed, counter).  Returns what
    ppo_head_check.head returns, with dout_actor [M, N, 2].  ``defect``: one of DEFECTS, planted (the twin only)."""
    f = dtype
    out = np.asarray(case["out"], np.float32)
    M, N = out.shape[:2]
    idx, valid = _safe_index(case)
    o = out.astype(f)
    v = np.asarray(case["value"], np.float32).astype(f).reshape(M, 1)
    sc, old, A, vt = (np.asarray(case[k], np.float32)[idx].astype(f) for k in ("scores", "score_log_prob", "advantage", "value_target"))
    if defect == "base_advantage":
        A = np.asarray(case["base_advantage"], np.float32)[idx].astype(f)
    lo32, hi32 = pc.clip_bounds(case["clip_epsilon"])
    lo, hi = f(lo32), f(hi32)
    R = M * N
    ce, cc = np.float32(case["entropy_coeff"]), np.float32(case["critic_coeff"])
    if f == np.float32:  # 1 / (M N) and its products with the coefficients: rounded once each, as the library's host code forms them
        inv = np.float32(1.0) / np.float32(R)
        ce_inv, cc_inv = ce * inv, cc * inv
    else:                # the reference: the exact mean
        inv = 1.0 / R
        ce_inv, cc_inv = float(ce) / R, float(cc) / R
    z = draws(case, f, ids=pc.ENTROPY_DRAWS if defect == "draw_entropy" else ENTROPY_DRAWS, sine=defect == "sine")
    loc, raw = o[..., 0], o[..., 1]
    w = raw + f(BIAS)
    s0 = phc.raw_scale_of(raw, f)
    sig = np.maximum(s0, f(1e-4))
    with np.errstate(over="ignore"):
        dsdr = np.where(s0 < f(1e-4), f(0.0), f(1.0) / (f(1.0) + np.exp(-w)))
    logs = np.log(sig)
    EPS = f(np.float32(1e-6))
    pre = (sc - f(-1.0)) / f(1.0) - f(1.0) if defect == "affine" else sc  # (the affine map with low = -1, high = 1: h = 1, and the sum rounds)
    y = np.minimum(np.maximum(pre, f(-1.0) + EPS), f(1.0) - EPS)
    x = f(0.5) * (np.log1p(y) - np.log1p(-y))
    q = (x - loc) / sig
    lp, sp = phc.log_density(q, logs, x, f)
    xs = loc + sig * z
    if defect == "entropy_clamped":  # the sample squashed, clamped and brought back, as a recorded score is
        ys = np.minimum(np.maximum(np.tanh(xs), f(-1.0) + EPS), f(1.0) - EPS)
        xs = f(0.5) * (np.log1p(ys) - np.log1p(-ys))
    lps, sps = phc.log_density(z, logs, xs, f)
    lw = lp - old
    cl = np.minimum(np.maximum(lw, lo), hi)
    with np.errstate(over="ignore"):
        g1, g2 = np.exp(lw) * A, np.exp(cl) * A
    on = g1 <= g2
    dlw = np.where(on, g1, g2 if defect == "grad_on_clamped" else f(0.0))
    e = v - vt
    ae = np.abs(e)
    sl1 = np.where(ae < f(1.0), f(0.5) * e * e, ae - f(0.5))
    de = np.minimum(np.maximum(e, f(-1.0)), f(1.0))
    clipped = (cl != lw).astype(f)
    th2 = f(2.0) * np.tanh(xs)
    vm = valid[:, None]
    zero = lambda t: np.where(vm, t, f(0.0))  # noqa: E731  (an index entry outside the records: zeros, never an address)

    def grads(dlw_):
        wobj = -inv * dlw_
        dl = wobj * (q / sig) + ce_inv * th2
        dsig = wobj * ((q * q - f(1.0)) / sig) + ce_inv * (th2 * z - f(1.0) / sig)
        dr = dsig if defect == "no_slope" else dsig * dsdr
        return np.stack([zero(dl), zero(dr)], -1)

    dout_a = grads(dlw)
    terms = dict(obj=zero(np.minimum(g1, g2)), lps=zero(lps), sl1=zero(sl1), lw=zero(lw))
    sums = (("obj", terms["obj"]), ("lps", terms["lps"]), ("sl1", terms["sl1"]), ("clip", zero(clipped)), ("kl", -terms["lw"]))
    if f == np.float32:
        s = np.zeros(M, f)
        for n in range(N):
            s = (s + de[:, n]).astype(f)
        dout_c = cc_inv * s
        S = {k: pc.ordered_sum(t.astype(f)) for k, t in sums}
    else:
        dout_c = cc_inv * de.sum(1)
        S = {k: float(t.sum()) for k, t in sums}
    if defect == "critic_sum_over_m":  # the sum runs over the minibatch's slots (agent m mod N) instead of the frame's agents
        dout_c = (cc_inv * de.sum(0))[np.arange(M) % N].astype(f)
    dout_c = np.where(valid, dout_c, f(0.0))
    entropy = -(f(S["lps"]) * inv)
    result = dict(loss_objective=-(f(S["obj"]) * inv), loss_entropy=-(f(ce) * entropy), loss_critic=f(cc) * (f(S["sl1"]) * inv), entropy=entropy,
                  clip_fraction=f(S["clip"]) * inv, kl_approx=f(S["kl"]) * inv)
    r = dict(dout_actor=dout_a, dout_critic=dout_c, result=result, terms=terms, lw=lw, lp=lp, g1=g1, g2=g2, A=A, e=e, sigma=sig, y=y, dlw_on=on, lo=lo, hi=hi, rows=R,
             inv=float(inv), ce=float(ce), cc=float(cc), clipped=int(((cl != lw) & vm).sum()), valid=valid)
    if f != np.float64:
        return r
    # ---- the magnitudes (float64 reference only), in units of one float32 rounding: ppo_head_check.head's, one dimension, y exact
    a = np.abs
    zm = draws(case, magnitude=True)
    dx = 2.0 * a(x)                                                              # atanh(y) of an exact y: the two log1p halved, and the subtraction
    qm = (dx + a(loc) + a(x)) / sig + 3.0 * a(q)                                 # q = (x - loc) / sigma (sigma carries a relative rounding or two of its own)
    S_lp = a(q) * qm + 0.5 * q * q + a(logs) + 1.0 + LOG_SQRT_2PI + 2 * LOG2 + 2 * a(x) + 2 * a(sp) + 2 * dx
    S_lw = S_lp + a(lp) + a(old)
    gm = np.maximum(a(g1), a(g2))
    S_obj = gm * (S_lw + 3.0)
    dxs = a(loc) + 2 * sig * zm + a(xs)                                          # x' = loc + sigma z
    S_lps = 0.5 * z * z + a(z) * zm + a(logs) + 1.0 + LOG_SQRT_2PI + 2 * LOG2 + 2 * a(xs) + 2 * a(sps) + 2 * dxs
    S_sl1 = np.minimum(ae, 1.0) * (a(v) + a(vt)) + 2 * sl1 + 0.5 * (ae >= 1.0)
    r["S_terms"] = dict(obj=zero(S_obj), lps=zero(S_lps), sl1=zero(S_sl1), lw=zero(S_lw))
    r["S_lp"] = S_lp
    sech2 = 1.0 - np.tanh(xs) ** 2

    def mags(dlw_):
        g = a(dlw_)
        Sg = a(dlw_) * (S_lw + 3.0)  # the magnitude of g1 = exp(lw) A
        t1 = float(inv) * (Sg * a(q) / sig + g * (qm / sig + 3 * a(q) / sig))
        t2 = a(ce_inv) * (3 * a(th2) + 2 * sech2 * dxs)
        S_dl = t1 + t2 + a(-inv * dlw_ * (q / sig)) + a(ce_inv * th2)
        u1 = float(inv) * (Sg * a(q * q - 1.0) / sig + g * (2 * a(q) * qm + 4 * (q * q + 1.0)) / sig)
        u2 = a(ce_inv) * (4 * a(th2) * a(z) + 2 * sech2 * dxs * a(z) + a(th2) * zm + 4.0 / sig)
        S_ds = u1 + u2 + a(-inv * dlw_ * ((q * q - 1.0) / sig)) + a(ce_inv * (th2 * z - 1.0 / sig))
        ds = -inv * dlw_ * ((q * q - 1.0) / sig) + ce_inv * (th2 * z - 1.0 / sig)
        S_dr = S_ds * dsdr + a(ds) * dsdr * (4.0 + a(raw) + BIAS)
        return np.stack([zero(S_dl), zero(S_dr)], -1)

    r["S_dout_actor"] = mags(dlw)
    alt = np.where(on, 0.0, g1)  # the other side of the clip branch
    r["alt_dout_actor"], r["S_alt_dout_actor"] = grads(alt), mags(alt)
    r["S_dout_critic"] = np.where(valid, a(cc_inv) * ((a(v) + a(vt)).sum(1) + (N + 3) * a(de).sum(1)), 0.0)
    return r


def constants(case, ref=None):
    """The twin's measured constants over the rows of ``case``: dict(dloc, draw, dcritic, obj, lps, sl1, lw)"""
    ref = ref if ref is not None else head(case)
    twin = head(case, np.float32)
    ra = pc._ratio(twin["dout_actor"], ref["dout_actor"], ref["S_dout_actor"])
    c = dict(dloc=float(ra[..., 0].max()), draw=float(ra[..., 1].max()), dcritic=float(pc._ratio(twin["dout_critic"], ref["dout_critic"], ref["S_dout_critic"]).max()))
    for k in ("obj", "lps", "sl1", "lw"):
        c[k] = float(pc._ratio(twin["terms"][k], ref["terms"][k], ref["S_terms"][k]).max())
    return c


_CALIBRATION = {}


def calibration():
    """The constants of the calibration case (``synthetic_case()`` at its defaults: 512 slots x 3 agents), for cases of fewer than FULL_ROWS rows"""
    if not _CALIBRATION:
        _CALIBRATION.update(constants(synthetic_case()))
    return _CALIBRATION


def constants_in_force(case, ref):
    c = constants(case, ref)
    if ref["rows"] < FULL_ROWS:
        c = {k: max(v, calibration()[k]) for k, v in c.items()}
    return c


def in_the_band(ref, c):
    """[M, N] bool: the rows whose float64 lw lies within its own bound of a clip bound (ppo_head_check's Branches); never a row of an entry outside the records"""
    tol = MARGIN * c["lw"] * U23 * ref["S_terms"]["lw"]
    return ((np.abs(ref["lw"] - float(ref["lo"])) <= tol) | (np.abs(ref["lw"] - float(ref["hi"])) <= tol)) & ref["valid"][:, None]


def clear_of_the_band(case, shift=0.05):
    """ppo_head_check.clear_of_the_band for this head: rows of the branch band are moved out of it through ``score_log_prob``"""
    case = dict(case, score_log_prob=np.array(case["score_log_prob"], np.float32))
    moved = 0
    for _ in range(4):
        ref = head(case)
        c = constants_in_force(case, ref)
        amb = in_the_band(ref, c)
        if not amb.any():
            break
        for m, n in np.argwhere(amb):
            case["score_log_prob"][case["index"][m], n] -= np.float32(np.copysign(shift, ref["lw"][m, n]))
        moved += int(amb.sum())
    return case, ref, c, moved


def compare(dout_actor, dout_critic, result, case, what=""):
    """ppo_head_check.compare for this head: the device's (or a twin's) outputs against ``head(case, float64)``"""
    ref = head(case)
    c = constants_in_force(case, ref)
    M, N = ref["lw"].shape
    r = dict(what=what, rows=ref["rows"], c=c)
    da = np.asarray(dout_actor, np.float64).reshape(M, N, 2)
    ck = np.array([c["dloc"], c["draw"]])
    main, alt = pc._ratio(da, ref["dout_actor"], ref["S_dout_actor"]) / ck, pc._ratio(da, ref["alt_dout_actor"], ref["S_alt_dout_actor"]) / ck
    amb = in_the_band(ref, c)
    use = np.where(amb[..., None], np.minimum(main, alt), main)
    r["ambiguous_rows"] = int(amb.sum())
    r["dloc"], r["draw"] = float(use[..., 0].max()), float(use[..., 1].max())
    r["dcritic"] = float((pc._ratio(np.asarray(dout_critic, np.float64).reshape(M), ref["dout_critic"], ref["S_dout_critic"]) / c["dcritic"]).max())
    ok = bool(np.isfinite(da).all() and max(r["dloc"], r["draw"], r["dcritic"]) <= MARGIN)
    res = {k: float(v) for k, v in zip(RESULT, np.asarray(result, np.float64).reshape(-1)[:6])}
    cnt, inv, T, S = pc.sum_depth(ref["rows"]) + 3, ref["inv"], ref["terms"], ref["S_terms"]

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
    assert r["ok"], f"{what}: the priority PPO head misses its criterion: {r}"
    return r, ref


def twin_outputs(case, defect=None):
    """(dout_actor, dout_critic, result in RESULT order) of the float32 twin, optionally with a planted defect"""
    t = head(case, np.float32, defect)
    return t["dout_actor"], t["dout_critic"], np.array([t["result"][k] for k in RESULT], np.float32)


def exact_clip_fraction(ref):
    return pc.exact_clip_fraction(ref)


def log_density_bound(ref, c):
    """[M, N]: the bound of a float32 log-probability of the recorded score against the float64 one -- the criterion's bound of ``lw`` without the terms of the
    subtraction of the recorded value"""
    return MARGIN * c["lw"] * U23 * ref["S_lp"]


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
def records_for(out64, value64, index, F, N, seed, small=()):
    """Records [F, N] that populate every branch for the minibatch (out64 [M, N, 2], value64 [M]) at the frames ``index``, as ppo_head_check.records_for makes them:
    recorded scores with |y| <= 0.999, score_log_prob = the reference's logp + a log-ratio inside the clip band for half of the rows and outside for the rest,
    advantages of both signs (``base_advantage``: a second, unrelated set), value targets with |e| on both sides of 1.  ``small``: frames whose scores are tiny
    (|s| < 1e-3), whose log-ratio lies inside the band and whose advantage is positive -- rows through which the gradient flows and where a rounding of the score shows."""
    g = np.random.default_rng(seed)
    index = np.asarray(index)
    M = len(index)
    sc = g.uniform(-0.999, 0.999, (F, N)).astype(np.float32)
    adv = (g.standard_normal((F, N)) * 1.5).astype(np.float32)
    adv[np.abs(adv) < 0.05] = 0.5
    base_adv = (g.standard_normal((F, N)) * 1.5).astype(np.float32)
    old = g.standard_normal((F, N)).astype(np.float32)
    vt = g.standard_normal((F, N)).astype(np.float32)
    small = np.asarray(small, np.int64)
    if small.size:
        sc[small] = g.uniform(-1e-3, 1e-3, (small.size, N)).astype(np.float32)
        adv[small] = np.abs(adv[small]) + np.float32(0.5)
    case = dict(out=np.asarray(out64, np.float32), value=np.asarray(value64, np.float32), index=index, scores=sc, score_log_prob=old, advantage=adv, value_target=vt,
                clip_epsilon=0.2, entropy_coeff=0.0, critic_coeff=1.0, seed=0, counter=0)
    ok = _safe_index(case)[1]
    lp = head(case)["lp"]  # the reference's logp of the recorded scores
    mag = np.where(g.random((M, N)) < 0.5, g.uniform(0.0, 0.15, (M, N)), g.uniform(0.3, 0.8, (M, N)))
    mag[np.isin(index, small)] = g.uniform(0.0, 0.15, (int(np.isin(index, small).sum()), N))
    lw = mag * np.where(g.random((M, N)) < 0.5, -1.0, 1.0)
    e = np.where(g.random((M, N)) < 0.5, g.uniform(0.02, 0.9, (M, N)), g.uniform(1.1, 3.0, (M, N))) * np.where(g.random((M, N)) < 0.5, -1.0, 1.0)
    for m, fr in enumerate(index):
        if ok[m]:
            old[fr] = (lp[m] - lw[m]).astype(np.float32)
            vt[fr] = (np.asarray(value64, np.float64).reshape(-1)[m] - e[m]).astype(np.float32)
    return dict(scores=sc, score_log_prob=old, advantage=adv, base_advantage=base_adv, value_target=vt)


def synthetic_case(M=512, N=3, F=700, seed=1, entropy_coeff=0.01, critic_coeff=1.0, clip_epsilon=0.2, counter=3, floor_rows=8, small_rows=8, index=None):
    """A case on synthetic network outputs, made per FRAME as a network's are (the slots of a frame picked twice agree): raw ~ N(0, 1.5), ``floor_rows`` frames at
    raw = -40 (sigma at its 0.01 floor), loc = x - sigma q with q ~ N(0, 1.2); ``small_rows`` further frames have sigma at the floor, tiny scores and q ~ N(0, 0.02)
    (``records_for``'s ``small``).  ``index`` (default) = a sample of the F frames with duplicates; entries outside [0, F) are legal and take no rows."""
    g = np.random.default_rng(seed)
    if index is None:
        index = g.integers(0, F, M).astype(np.int32)
        index[:2] = index[min(2, M - 1)]  # (a frame picked three times for certain)
    index = np.asarray(index, np.int32)
    M = len(index)
    inside = np.unique(index[(index >= 0) & (index < F)])
    picked = g.permutation(inside)
    floor, small = picked[: min(floor_rows, len(picked))], picked[floor_rows: floor_rows + small_rows]
    raw = g.standard_normal((F, N)) * 1.5
    raw[floor] = -40.0
    raw[small] = -40.0
    outF = np.zeros((F, N, 2), np.float32)
    outF[..., 1] = raw
    valueF = g.standard_normal(F).astype(np.float32)
    safe = np.where((index >= 0) & (index < F), index, 0)
    rec = records_for(outF[safe], valueF[safe], index, F, N, seed + 1, small)
    # loc from the recorded score's x: a second pass, now that the scores exist
    y = np.clip(rec["scores"].astype(np.float64), -1 + 1e-6, 1 - 1e-6)
    sig = phc.scale_of(outF[..., 1], np.float64)
    qs = g.standard_normal((F, N)) * 1.2
    qs[small] = g.standard_normal((len(small), N)) * 0.02
    outF[..., 0] = (np.arctanh(y) - sig * qs).astype(np.float32)
    out, value = outF[safe], valueF[safe]
    rec = records_for(out, value, index, F, N, seed + 1, small)
    return dict(out=out, value=value, index=index, clip_epsilon=clip_epsilon, entropy_coeff=entropy_coeff, critic_coeff=critic_coeff, seed=1234567, counter=counter,
                small=small, **rec)


# the (M, N) of the device test: one row; 255 and 258 rows, either side of a workgroup boundary; full wavefronts; 16 agents; 129 workgroups with a ragged last one
# and 130 (33020 and 33028 rows), where lane 0 (and lane 1) of the final sum takes its third pass
DEVICE_CASES = ((1, 1), (85, 3), (86, 3), (64, 4), (16, 16), (8255, 4), (8257, 4))
_CASES = {}


def device_case(M, N, out_of_range=False):
    """The case of M slots x N agents over F = M + 3 frames (an index with duplicates), cleared of the branch band: (case, float64 reference, constants, rows
    moved).  ``out_of_range``: one entry of the index (the middle one) lies outside the records.  Made once per key."""
    key = (M, N, out_of_range)
    if key not in _CASES:
        F = M + 3
        g = np.random.default_rng(7000 + 31 * M + N)
        idx = g.integers(0, F, M).astype(np.int32)
        if M > 1:
            idx[-1] = idx[0]
        if out_of_range:
            idx[M // 2] = F if M % 2 else -1
        k = min(8, max(1, M // 8))
        _CASES[key] = clear_of_the_band(synthetic_case(N=N, F=F, seed=60 + M + N, index=idx, floor_rows=k if M > 2 else 0, small_rows=k if M > 2 else 0))
    return _CASES[key]


# ---- the same formulas in torch (autograd: the host cross-check of the analytical gradients) ------------------------------------------------
def torch_head(out, value, index, case, z, dtype):
    """(loss_objective, loss_entropy, loss_critic) as torch scalars with a graph over ``out [M, N, 2]`` and ``value [M]``; every index entry inside the records"""
    import torch

    t = lambda k: torch.from_numpy(np.asarray(case[k], np.float32)).to(dtype)[index]  # noqa: E731
    sc, old, A, vt = t("scores"), t("score_log_prob"), t("advantage"), t("value_target")
    lo, hi = (float(b) for b in pc.clip_bounds(case["clip_epsilon"]))
    loc, raw = out[..., 0], out[..., 1]
    sig = torch.clamp_min(torch.nn.functional.softplus(raw + BIAS) + 0.01, 1e-4)
    eps = float(np.float32(1e-6))
    x = torch.atanh(torch.clamp(sc, -1.0 + eps, 1.0 - eps))
    jac = lambda u: 2.0 * (LOG2 - u - torch.nn.functional.softplus(-2.0 * u))  # noqa: E731
    lp = -((x - loc) ** 2) / (2 * sig ** 2) - torch.log(sig) - LOG_SQRT_2PI - jac(x)
    lw = lp - old
    g1, g2 = torch.exp(lw) * A, torch.exp(torch.clamp(lw, lo, hi)) * A
    xs = loc + sig * z
    lps = -(z ** 2) / 2 - torch.log(sig) - LOG_SQRT_2PI - jac(xs)
    e = value.reshape(-1, 1) - vt
    sl1 = torch.where(e.abs() < 1.0, 0.5 * e * e, e.abs() - 0.5)
    return -torch.min(g1, g2).mean(), float(np.float32(case["entropy_coeff"])) * lps.mean(), float(np.float32(case["critic_coeff"])) * sl1.mean()


# ---- the padded critic rows ---------------------------------------------------------------------------------------------------------------------
def padded_rows(src, N, D, Dc):
    """[rows, N * Dc] from rows whose first N * D floats are N segments of D: element j of agent a's segment is ``j < D ? src[a * D + j] : 0`` -- the env's own next
    observation with the 2 K placeholder columns of the base observation zero (sigmaenv_mlp32_forward_rows_pad's rows, include/sigmaenv.h)"""
    src = np.asarray(src)
    rows = src.shape[0]
    out = np.zeros((rows, N * Dc), src.dtype)
    for k in range(N * Dc):
        a, j = divmod(k, Dc)
        if j < D:
            out[:, k] = src[:, a * D + j]
    return out
