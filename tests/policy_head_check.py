"""The yardstick of the policy heads (actor_distribution in sigmaenv_actor.inc, sigmaenv_priority_head_kernel and sigmaenv_priority_random_kernel in
sigmaenv_wrappers.inc): a plain helper module, imported by the tests.  The generator, the head and the criterion are numpy only; ``calibration`` and the
``regime_*`` case builders at the end need torch (imported inside them).

The generator is a pure integer function of (seed, counter, env, agent, draw), so the draw every row made is recomputed here exactly (``rng_u32``, held to the
oracle's C function by tests/test_policy_head_check.py; ``uniform``; ``normals``).  With z known, the action and the log-probability of a row follow from the
head's inputs (loc, scale) in closed form: ``head(..., np.float64)`` is the reference, ``head(..., np.float32)`` the calibration twin, the same formulas in
the kernels' operation order in float32.

The criterion (``compare``).  Per row,

    |lp_dev - lp_64|  <= MARGIN * c   * 2^-23 * S(row)        S: the sum of the magnitudes of everything that is added up to form the log-probability,
                                                               plus 2 |x| + 2 scale m + |z| m per dimension (the rounding of x = loc + scale z enters
                                                               through the Jacobian term, whose slope is at most 2; m: the magnitude at which the
                                                               float32 draw rounds, |z| + angle * |the other branch|, see ``normals``)
    |a_dev  - a_64|   <= MARGIN * c_a * 2^-23 * A(row, dim)   A = max(1, |low|, |high|) + h (1 - y^2) (|loc| + 2 scale m): the affine map's own rounding
                                                               plus the rounding of x seen through d tanh / dx = 1 - y^2

with c and c_a MEASURED on the float32 twin against float64 over the very rows of the case, never on the kernel, and MARGIN = 4.  A case of fewer than
``FULL_ROWS`` = 1000 rows can be lucky (one row may round exactly): it is given the larger of its own constants and those of its calibration case, the twin
on 257 x 16 rows of the same network with the same key and bounds (``calibration``).  No constant is typed in.  The margin is not a measurement: the device's logf / expf / log1pf / tanhf / sincosf
need not round as numpy's do.  Rows with |x| >= ``SATURATED`` = 10 have tanh(x) within 4.2e-9 of +-1, far inside the clamp at 1 - 1e-6 (float32: 1 - 17 * 2^-24):
their action is the clamp's image under the affine map, three float32 operations that the build evaluates without contraction, and is compared EXACTLY.
"""
from __future__ import annotations

import math
import weakref

import numpy as np

MARGIN = 4.0      # times the twin's measured constant
FULL_ROWS = 1000  # a case of fewer rows also takes the constants of its calibration case
SATURATED = 10.0  # |x| from which the clamped tanh is exactly the clamp
U23 = 2.0 ** -23

BIAS = 0.5254587192925021                      # ln(e^0.99 - 1): biased_softplus_1.0 with min_val 0.01
LOG_SQRT_2PI, LOG2 = 0.91893853320467274, 0.69314718055994531
EPS32 = np.float32(1e-6)                       # SafeTanhTransform: finfo(float32).resolution
CLAMP_HI = np.float32(1.0) - EPS32             # 1 - 17 * 2^-24
CLAMP_LO = np.float32(-1.0) + EPS32
TWO_PI32 = np.float32(6.283185307179586)

ACTOR_DRAWS, PRIORITY_DRAWS, SHUFFLE_DRAW = (7000, 7001), (7100, 7101), 7200  # sigmaenv_dist.h: DRAW_ACTOR, DRAW_PRIORITY (+ 1 each), DRAW_SHUFFLE
_M = 0xFFFFFFFF


# ---- the generator ------------------------------------------------------------------------------------------------------------------
def _u32(v):
    """the low 32 bits of python ints / integer arrays, as a uint32 array"""
    if isinstance(v, np.ndarray):
        return (v.astype(np.uint64) & np.uint64(_M)).astype(np.uint32) if v.dtype != np.uint32 else v
    return np.asarray(int(v) & _M, np.uint32)


def _hi32(v):
    if isinstance(v, np.ndarray):
        return (v.astype(np.uint64) >> np.uint64(32)).astype(np.uint32)
    return np.asarray((int(v) >> 32) & _M, np.uint32)


def _fmix(h):
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def stream_key(env, agent):
    """What (env, agent) contribute to the generator's pre-mix: two streams draw the same numbers at every seed, counter and draw id exactly when these
    coincide (the pre-mix is an XOR of per-field terms, everything after it a bijection of 32 bits)."""
    with np.errstate(over="ignore"):
        return ((_u32(env) + np.uint32(0x165667B1)) * np.uint32(0xC2B2AE35)) ^ ((_u32(agent) + np.uint32(0x27D4EB2F)) * np.uint32(0x9E3779B1))


def rng_u32(seed, counter, env, agent, draw):
    """sigmaenv_dist.h rng_u32, vectorised (arguments broadcast): ``seed`` enters with both 32-bit words, ``counter`` with its low 32 bits only."""
    with np.errstate(over="ignore"):
        h = _u32(seed) ^ (_hi32(seed) * np.uint32(0x9E3779B9))
        h = h ^ ((_u32(counter) + np.uint32(0x7F4A7C15)) * np.uint32(0x85EBCA6B))
        h = h ^ stream_key(env, agent)
        h = h ^ ((_u32(draw) + np.uint32(0x61C88647)) * np.uint32(0x85EBCA77))
        h = _fmix(h)
        h = h + np.uint32(0x9E3779B9)
        return _fmix(h)


def uniform(k):
    """((k >> 8) + 0.5f) * 2^-24 in float32, as the kernels form it: from k >> 8 = 2^23 on the + 0.5f rounds to even, so u = 1.0f is reachable (log u = 0: z = 0)."""
    return ((np.asarray(k, np.uint32) >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def normals(seed, counter, env, agent, draws=ACTOR_DRAWS, dtype=np.float64, magnitude=False):
    """Box-Muller from the two float32 uniforms of ``draws``: (z0, z1) = r (cos, sin)(a), r = sqrt(-2 ln u1), a = 2 pi u2.  float64: the reference; float32: the
    kernels' operations (the angle is the float32 product 6.2831855f * u2).  The priority head takes z0 of draws (7100, 7101).
    ``magnitude``: (m0, m1) instead, the magnitudes at which the float32 draws round: m0 = |z0| + a |z1|, m1 = |z1| + a |z0| -- the angle carries a relative
    rounding, and d z0 / d a = -z1, d z1 / d a = z0."""
    u1, u2 = uniform(rng_u32(seed, counter, env, agent, draws[0])), uniform(rng_u32(seed, counter, env, agent, draws[1]))
    if dtype == np.float32 and not magnitude:
        r = np.sqrt(np.float32(-2.0) * np.log(u1))
        a = TWO_PI32 * u2
        return r * np.cos(a), r * np.sin(a)
    r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    a = 2.0 * math.pi * u2.astype(np.float64)
    z0, z1 = r * np.cos(a), r * np.sin(a)
    return (np.abs(z0) + a * np.abs(z1), np.abs(z1) + a * np.abs(z0)) if magnitude else (z0, z1)


def row_keys(B, N, env_index_base=0):
    """(env, agent) of the agent rows of a [B, N] batch whose first env has index ``env_index_base`` in the whole batch"""
    r = np.arange(B * N)
    return (env_index_base + r // N).astype(np.uint32), (r % N).astype(np.uint32)


def random_ranks(seed, counter, env, N):
    """sigmaenv_priority_random_kernel: the inside-out Fisher-Yates shuffle, position i draws j = umulhi(rng(.., agent = i, 7200), i + 1) in [0, i];
    ``env``: the env indices [B]; returns [B, N] int32."""
    env = np.asarray(env, np.uint32).reshape(-1)
    r = np.zeros((env.size, N), np.int32)
    rows = np.arange(env.size)
    for i in range(N):
        j = ((rng_u32(seed, counter, env, i, SHUFFLE_DRAW).astype(np.uint64) * np.uint64(i + 1)) >> np.uint64(32)).astype(np.int64)
        r[rows, i] = r[rows, j]
        r[rows, j] = i
    return r


# ---- the head -----------------------------------------------------------------------------------------------------------------------
def softplus(v, dtype, shortcut=True):
    """float32: the kernels' v > 20 ? v : log1p(exp(v)); float64: exact at either side of the switch"""
    v = np.asarray(v, dtype)
    with np.errstate(over="ignore"):
        s = np.log1p(np.exp(np.minimum(v, dtype(80.0))))
    if dtype == np.float32:
        return np.where(v > dtype(20.0), v, s) if shortcut else s
    return np.where(v > 30.0, v + np.log1p(np.exp(-np.maximum(v, 30.0))), s)  # (exact in float64 at either side)


def raw_scale_of(raw, dtype=np.float64):
    """softplus(raw + ln(e^0.99 - 1)) + 0.01: the scale before its 1e-4 floor"""
    return softplus(np.asarray(raw, dtype) + dtype(BIAS), dtype) + dtype(0.01)


def scale_of(raw, dtype=np.float64):
    """NormalParamExtractor "biased_softplus_1.0": max(softplus(raw + ln(e^0.99 - 1)) + 0.01, 1e-4)"""
    return np.maximum(raw_scale_of(raw, dtype), dtype(1e-4))


def log_density(q, log_scale, x, dtype):
    """(-q^2 / 2 - log scale - log sqrt(2 pi) - 2 (log 2 - x - softplus(-2 x)), softplus(-2 x)) per dimension, q = (x - loc) / scale (a sample's own x: q = z):
    the TanhNormal log-density without the - log h of the affine map, in the kernels' operation order"""
    f = dtype
    sp = softplus(f(-2.0) * x, f)
    return f(-0.5) * q * q - log_scale - f(LOG_SQRT_2PI) - f(2.0) * (f(LOG2) - x - sp), sp


def head(loc, scale, z, low=None, high=None, dtype=np.float64, zmag=None):
    """TanhNormal(loc, scale) between ``low`` and ``high`` at the draw ``z`` (all [rows, d]; the log-probability sums over d).  ``low is None``: the 1-D head
    of the priority actor on [-1, 1], without the affine map (the score is the clamped tanh itself, no - log h).  ``zmag``: the magnitude at which z rounds
    (``normals(magnitude=True)``; default |z|).  Returns dict(x, y, action, log_prob, S, A); float32: every operation in the kernels' order in float32."""
    f = dtype
    loc, scale, z = (np.asarray(v).astype(f) for v in (loc, scale, z))
    x = loc + scale * z
    y = np.minimum(np.maximum(np.tanh(x), f(CLAMP_LO)), f(CLAMP_HI))
    affine = low is not None
    if affine:
        low, high = np.asarray(low, np.float32).astype(f), np.asarray(high, np.float32).astype(f)
        h = f(0.5) * (high - low)
        action = low + (y + f(1.0)) * h
        log_h = np.log(h)
    else:
        h, action, log_h = f(1.0), y, f(0.0)
    lp_d, sp = log_density(z, np.log(scale), x, f)
    if affine:
        lp_d = lp_d - log_h
    lp = lp_d[:, 0] + lp_d[:, 1] if lp_d.shape[-1] == 2 else lp_d[:, 0]
    a64 = lambda v: np.abs(np.asarray(v, np.float64))  # noqa: E731
    zm = a64(z) if zmag is None else np.asarray(zmag, np.float64)
    S = (0.5 * a64(z) ** 2 + a64(z) * zm + a64(np.log(scale)) + LOG_SQRT_2PI + 2 * LOG2 + 2 * a64(x) + 2 * a64(sp) + a64(log_h) + 2 * a64(x) + 2 * a64(scale) * zm).sum(-1)
    big = np.maximum(1.0, np.maximum(a64(low), a64(high))) if affine else 1.0
    A = big + a64(h) * (1.0 - np.asarray(y, np.float64) ** 2) * (a64(loc) + 2 * a64(scale) * zm)
    return dict(x=x, y=y, action=action, log_prob=lp, S=S, A=A)


def saturated_action(x64, low=None, high=None):
    """The action of a saturated row (|x| >= SATURATED) in the kernels' float32 operations: the clamp through the affine map."""
    y = np.where(np.asarray(x64) > 0, CLAMP_HI, CLAMP_LO).astype(np.float32)
    if low is None:
        return y
    low, high = np.asarray(low, np.float32), np.asarray(high, np.float32)
    return low + (y + np.float32(1.0)) * (np.float32(0.5) * (high - low))


def compare(action_dev, log_prob_dev, loc, scale, z, low=None, high=None, z32=None, zmag=None, raw=None, what="", least=(0.0, 0.0)):
    """The criterion of the module docstring for one case: the device's actions [rows, d] and log-probabilities [rows] (None: not compared) against
    ``head(loc, scale, z, float64)``, every row.  ``z32``: the twin's float32 draws (default: ``z`` rounded -- a deterministic case has z = 0).  ``raw``
    instead of ``scale`` (the priority head, whose input is the network's raw output): the reference takes ``scale_of(raw)`` in float64, the twin in float32.
    ``least``: (c, c_a) of the calibration case, for a case of few rows.  Returns the figures; ``ok`` says whether every row passed."""
    loc = np.asarray(loc, np.float32)
    z = np.asarray(z, np.float64)
    s64, s32 = (scale_of(np.asarray(raw, np.float32), np.float64), scale_of(np.asarray(raw, np.float32), np.float32)) if raw is not None else (np.asarray(scale, np.float32),) * 2
    ref = head(loc, s64, z, low, high, np.float64, zmag)
    twin = head(loc, s32, z.astype(np.float32) if z32 is None else z32, low, high, np.float32)
    r = dict(what=what, rows=int(loc.shape[0]))
    a_dev = np.asarray(action_dev, np.float32).reshape(ref["action"].shape)
    ua = U23 * ref["A"]
    r["c_a"] = max(float((np.abs(twin["action"].astype(np.float64) - ref["action"]) / ua).max()), float(least[1]))
    r["c_a_dev"] = float((np.abs(a_dev.astype(np.float64) - ref["action"]) / ua).max())
    r["a_err_twin"], r["a_err_dev"] = float(np.abs(twin["action"] - ref["action"]).max()), float(np.abs(a_dev - ref["action"]).max())
    ok = bool(np.isfinite(a_dev).all() and r["c_a_dev"] <= MARGIN * r["c_a"])
    sat = np.abs(ref["x"]) >= SATURATED
    want = np.broadcast_to(saturated_action(ref["x"], low, high), a_dev.shape)
    r["saturated"], r["saturated_wrong"] = int(sat.sum()), int((a_dev[sat] != want[sat]).sum())
    ok &= r["saturated_wrong"] == 0
    if log_prob_dev is not None:
        lp_dev = np.asarray(log_prob_dev, np.float32).reshape(ref["log_prob"].shape).astype(np.float64)
        us = U23 * ref["S"]
        r["c"] = max(float((np.abs(twin["log_prob"].astype(np.float64) - ref["log_prob"]) / us).max()), float(least[0]))
        r["c_dev"] = float((np.abs(lp_dev - ref["log_prob"]) / us).max())
        r["lp_err_twin"], r["lp_err_dev"] = float(np.abs(twin["log_prob"] - ref["log_prob"]).max()), float(np.abs(lp_dev - ref["log_prob"]).max())
        r["lp_bound_max"], r["lp_bound_median"] = float((MARGIN * r["c"] * us).max()), float(np.median(MARGIN * r["c"] * us))
        ok &= bool(np.isfinite(lp_dev).all() and r["c_dev"] <= MARGIN * r["c"])
    r["ok"] = bool(ok)
    return r, ref


def compare_scale(scale_dev, raw64, raw_bound):
    """The device's scale against scale_of(raw) in float64, raw from the float64 network: |d scale / d raw| <= 1, so the network's bound on raw (``raw_bound``,
    the criterion of tests/network_check.py) carries over, plus one float32 rounding of the sum raw + bias and of the result; and scale >= 0.01 everywhere."""
    want = scale_of(raw64, np.float64)
    s = np.asarray(scale_dev, np.float64).reshape(want.shape)
    err = np.abs(s - want)
    bound = raw_bound + (np.abs(want) + np.abs(np.asarray(raw64, np.float64)) + BIAS) * 2.0 ** -23
    return dict(ok=bool(np.isfinite(s).all() and (err <= bound).all() and s.min() >= np.float32(0.01)), err_max=float(err.max()), ratio_max=float((err / bound).max()),
                scale_min=float(s.min()))


def check_rows(action_dev, log_prob_dev, loc, scale, seed, counter, B, N, env_index_base=0, low=None, high=None, draws=ACTOR_DRAWS, deterministic=False, raw=None,
               rows=None, what="", net=None):
    """``compare`` for agent rows of a [B, N] batch: the draw of every row is recomputed from its key (seed, counter, env_index_base + env, agent) -- zero when
    ``deterministic``.  ``rows``: the agent rows (env * N + agent) the given arrays hold, default all B * N in order.  The 1-D head (``low is None``) takes
    the cosine branch of ``draws``.  ``net``: the network of the case (torch), required for a case of fewer than FULL_ROWS rows: its calibration case gives the
    least constants.  Returns (figures, reference, z)."""
    env, agent = row_keys(B, N, env_index_base)
    if rows is not None:
        env, agent = env[rows], agent[rows]
    d = np.asarray(loc).shape[1]
    if deterministic:
        z = np.zeros((env.size, d))
        z32 = zmag = None
    else:
        z = np.stack(normals(seed, counter, env, agent, draws), -1)[:, :d]
        z32 = np.stack(normals(seed, counter, env, agent, draws, np.float32), -1)[:, :d]
        zmag = np.stack(normals(seed, counter, env, agent, draws, magnitude=True), -1)[:, :d]
    least = (0.0, 0.0)
    if env.size < FULL_ROWS:
        assert net is not None, "a case of few rows needs its network for the calibration case"
        least = calibration(net, seed, counter, env_index_base, low, high, draws, deterministic)
    r, ref = compare(action_dev, log_prob_dev, loc, scale, z, low, high, z32=z32, zmag=zmag, raw=raw, what=what, least=least)
    return r, ref, z


_CALIBRATION_OUT = weakref.WeakKeyDictionary()  # network -> its float32 outputs on the calibration rows


def calibration(net, seed, counter, env_index_base=0, low=None, high=None, draws=ACTOR_DRAWS, deterministic=False):
    """(c, c_a) of the calibration case of ``net``: the float32 twin against float64 on 257 x 16 rows -- ``regime_input`` through the network in float32 on the
    CPU -- with the key, the bounds and the head (``low is None``: the 1-D head) of the case it stands in for."""
    import torch
    B, N = 257, 16
    out = _CALIBRATION_OUT.get(net)
    if out is None:
        lin = [m for m in net.modules() if isinstance(m, torch.nn.Linear)]
        with torch.no_grad():
            out = _CALIBRATION_OUT[net] = net(torch.from_numpy(regime_input(B * N, obs_dim=lin[0].in_features))).numpy()
    d = 1 if low is None else 2
    loc, raw = out[:, :d], out[:, d:2 * d]
    env, agent = row_keys(B, N, env_index_base)
    if deterministic:
        z, z32, zmag = np.zeros((B * N, d)), None, None
    else:
        z = np.stack(normals(seed, counter, env, agent, draws), -1)[:, :d]
        z32 = np.stack(normals(seed, counter, env, agent, draws, np.float32), -1)[:, :d]
        zmag = np.stack(normals(seed, counter, env, agent, draws, magnitude=True), -1)[:, :d]
    twin = head(loc, scale_of(raw, np.float32), z.astype(np.float32) if z32 is None else z32, low, high, np.float32)
    # (the actor's cases compare at the device's own float32 scale; the priority head's at scale_of(raw), formed in float64 by the reference)
    sc, rw = (None, raw) if low is None else (scale_of(raw, np.float32), None)
    r, _ = compare(twin["action"], twin["log_prob"], loc, sc, z, low, high, z32=z32, zmag=zmag, raw=rw)
    return r["c"], r["c_a"]


# ---- the cases (torch; shared by the host tests, which count the regimes on the CPU, and the GPU tests) -------------------------------------------
LAST_LAYER_SCALES = (1, 8, 30)  # moderate | tanhf = 1, the clamp, the -2 x > 20 shortcut, the scale floor | raw + bias > 20, most rows saturated


def regime_net(last_scale, kind="actor", seed=11, obs_dim=32):
    """The actor (obs_dim -> 256 -> 256 -> 256 -> 4) or the priority network (obs_dim -> 256 -> 256 -> 2) with weights x 1.7, biases U(-0.3, 0.3) and the LAST
    layer's weights x ``last_scale``"""
    import torch
    L, T = torch.nn.Linear, torch.nn.Tanh
    torch.manual_seed(seed)
    if kind == "actor":
        mlp = torch.nn.Sequential(L(obs_dim, 256), T(), L(256, 256), T(), L(256, 256), T(), L(256, 4))
    else:
        mlp = torch.nn.Sequential(L(obs_dim, 256), T(), L(256, 256), T(), L(256, 2))
    with torch.no_grad():
        for m in mlp:
            if isinstance(m, L):
                m.weight.mul_(1.7)
                m.bias.uniform_(-0.3, 0.3)
        mlp[-1].weight.mul_(float(last_scale))
    return mlp


def regime_input(rows, seed=5, obs_dim=32):
    g = np.random.default_rng(seed)
    return ((g.random((rows, obs_dim), dtype=np.float32) * 2 - 1) * 1.5).astype(np.float32)


def regime_counts(x, scale, z):
    """How many values of a case lie in each regime of the head (x, z: float64 [rows, d]; scale: [rows, d])"""
    x, scale = np.asarray(x, np.float64), np.asarray(scale, np.float64)
    return dict(tanh_is_one=int((np.abs(x) >= 9.02).sum()),            # tanhf(x) = +-1 in float32: the clamp acts
                shortcut_jacobian=int((-2.0 * x > 20.0).sum()),        # softplus(-2 x) takes the v > 20 branch
                shortcut_scale=int((scale > 20.0101).sum()),            # softplus(raw + bias) took it: scale = raw + bias + 0.01
                scale_floor=int((scale < 0.0101).sum()),
                inside=int((np.abs(x) < 1.0).sum()),
                tail_draw=int((np.abs(np.asarray(z)) > 4.0).sum()))
