"""The yardstick of the episode return on the device (sigmaenv_episode_return, sigmarl_amd/csrc/sigmaenv_episode.inc; the arithmetic is stated in
sigmarl_amd/csrc/sigmaenv_episode.h, the contract in include/sigmaenv.h): a plain numpy helper module like optim_check.py, imported by the tests
(tests/test_episode_check.py runs it on the host against the header compiled alone, tests/test_gpu_episode.py on the device's tensors).  No test functions.

A ``case`` is a dict: ``T, B, N, D``, ``reward [T, B, N]`` and ``done [T, B]`` (float32; the done flag is 0.0 or 1.0 as the record holds it), ``carry [B, N]`` (the
incoming running returns) and ``slab [T, Bt, W]`` -- the hand-made record rows ``[N*D observation | N reward | 1 done]`` that hold them, ``W = N*(D+1)+1``, the
observation part filled with numbers that are no reward (a read at a wrong offset shows); ``Bt >= B`` and ``env_first`` place the case's envs inside a wider
buffer.  No env is needed to make one.

What is held, and to what.
  The record (RewardSum, sigmarl/mappo_cavs.py:178-183, restated from torchrl's published behaviour): forwards over t, ``E[t,b,i] = c + r[t,b,i]``, then
  ``c = 0 if done[t,b] else E[t,b,i]``; ``carry`` on exit is the last ``c``.  ``twin`` does exactly that in float32, one addition per step: header and device must equal
  it BIT FOR BIT (``E`` and ``carry``) -- the record is defined as the step-by-step fp32 sum, so there is no tolerance to derive.  ``recurrence64`` is the same
  recurrence in float64 with its first-order distance bound ``n u A`` (n = the steps of the open episode so far, A = the sum of |r| over them, u = 2^-24), against
  which the twin itself is checked: it says that the fp32 record is the reference's number up to the rounding any fp32 RewardSum has.
  The reduction (episode_reward[done].mean(), :468-478): ``K`` = the number of done frames (exact); ``S`` = the sum of E over the done frames and all agents in the
  header's order -- per frame the chain over i from 0; per env the chain over its done steps, t ascending, from 0; over the envs lane l of 256 the chain over
  b = l, l + 256, .. from 0, the butterfly per wavefront of 64 (v += v[lane ^ m], m = 32 .. 1) and ((w0 + w1) + w2) + w3 --; ``mean = S / (fl(K) * fl(N))``, NaN at
  K = 0.  ``twin`` reproduces that order in float32: header and device must equal ``S`` and ``mean`` bit for bit (any NaN equals any NaN: the sign of 0 / 0 is the
  one thing IEEE leaves open).  ``reference64`` sums THE RECORDED float32 E over the done frames in float64 (the record is already pinned bit for bit: what is left
  to bound is the reduction's own rounding):
      |S - S64|       <= chain * 2^-24 * sum|E|,  chain = the header's longest chain of additions, N + T + ceil(B / 256) + 9     (``longest_chain``)
      |mean - mean64| <= that / (K N)  +  |S| / (K N) * 2 u / (1 - u)    (one rounding for the product K * N, one for the division)
  The first bound is rigorous, not first-order: three additions of the chain add to 0 and are exact, and (1 + u)^(n-3) - 1 <= n u for every n below 10^4.

Planted defects (``DEFECTS``; ``twin(case, defect=)``): each must miss a bar on the test inputs (tests/test_episode_check.py).
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
LANES = 256  # EPR_LANES
MAX_FRAMES = 1 << 24  # EPR_MAX_FRAMES
DEFECTS = ("reset_before_add", "carry_not_written", "carry_from_t_minus_2", "done_of_next_env", "mean_over_k", "not_done_in_sum", "e_in_float64")
PATTERNS = ("done_t0", "done_last", "consecutive", "none", "all", "mixed")


def longest_chain(T, B, N):
    """epr_longest_chain"""
    return N + T + -(-B // LANES) + 6 + 3


def rewards(rng, T, B, N):
    """mixed sign, magnitudes spread over 2^-20 .. 2^4 with full mantissas: fp32 addition order matters"""
    mag = np.exp2(rng.uniform(-20.0, 4.0, (T, B, N))) * rng.uniform(1.0, 2.0, (T, B, N)) * 0.5
    return (mag * rng.choice([-1.0, 1.0], (T, B, N))).astype(np.float32)


def done_pattern(rng, T, B, pattern):
    d = np.zeros((T, B), np.float32)
    if pattern == "done_t0":
        d[0, :] = 1.0
    elif pattern == "done_last":
        d[T - 1, :] = 1.0
    elif pattern == "consecutive":  # runs of dones on consecutive steps, at an offset that differs from env to env
        for b in range(B):
            t0 = b % T
            d[t0: t0 + 3, b] = 1.0
    elif pattern == "none":
        pass
    elif pattern == "all":
        d[:] = 1.0
    elif pattern == "mixed":
        d[:] = (rng.uniform(size=(T, B)) < 0.3).astype(np.float32)
    else:
        raise ValueError(pattern)
    return d


def make_slab(reward, done, D, Bt=None, env_first=0, seed=0):
    """the record rows that hold ``reward`` / ``done``: [T, Bt, W]; everything else is filled with numbers in [100, 200)"""
    T, B, N = reward.shape
    Bt = B if Bt is None else Bt
    W = N * (D + 1) + 1
    slab = np.random.default_rng(seed + 77).uniform(100.0, 200.0, (T, Bt, W)).astype(np.float32)
    slab[:, env_first: env_first + B, N * D: N * D + N] = reward
    slab[:, env_first: env_first + B, N * D + N] = done
    return slab


def make_case(T, B, N, D, pattern="mixed", seed=0, carry=False, done=None, Bt=None, env_first=0):
    rng = np.random.default_rng(seed)
    r = rewards(rng, T, B, N)
    d = done_pattern(rng, T, B, pattern) if done is None else np.asarray(done, np.float32).reshape(T, B)
    c = rewards(rng, 1, B, N)[0] * np.float32(3.0) if carry else np.zeros((B, N), np.float32)
    return dict(T=T, B=B, N=N, D=D, reward=r, done=d, carry=c.astype(np.float32), slab=make_slab(r, d, D, Bt, env_first, seed), env_first=env_first, pattern=pattern)


def done_count_case(T, B, N, D, per_env, seed=0):
    """``per_env`` done steps in every env (the first ones, so that the env's chain has exactly that many terms)"""
    d = np.zeros((T, B), np.float32)
    d[:per_env, :] = 1.0
    return make_case(T, B, N, D, done=d, seed=seed, carry=True)


def block_sum(lanes):
    """[256] lane values -> the workgroup's sum in the values' dtype: per wavefront of 64 lanes the butterfly v += v[lane ^ m], m = 32 .. 1, then ((w0 + w1) + w2) + w3"""
    v = lanes.reshape(4, 64)
    lane = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ m]
    w = v[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def lane_sums(s):
    """lane l the chain from 0 over s[l], s[l + 256], .."""
    J = max(1, -(-s.size // LANES))
    q = np.zeros(J * LANES, s.dtype)
    q[: s.size] = s
    q = q.reshape(J, LANES)
    v = np.zeros(LANES, s.dtype)
    for j in range(J):
        v = v + q[j]
    return v


def twin(case, defect=None):
    """The header's operations in the header's order in float32: ``{"E" [T,B,N], "carry" [B,N], "S", "mean" (float32), "K" (int)}``; optionally with a planted defect."""
    assert defect is None or defect in DEFECTS
    T, B, N = case["T"], case["B"], case["N"]
    r, done = case["reward"], case["done"]
    f32 = np.float32
    c = case["carry"].astype(np.float64 if defect == "e_in_float64" else f32)
    E = np.zeros((T, B, N), f32)
    s, k = np.zeros(B, f32), np.zeros(B, np.int64)
    carry_out = case["carry"].copy()
    for t in range(T):
        d = done[t] != 0
        if defect == "done_of_next_env":
            d = np.roll(d, -1)
        if defect == "reset_before_add":
            c = np.where(d[:, None], c.dtype.type(0), c)
        Ec = c + r[t].astype(c.dtype)  # one addition per step
        E[t] = Ec.astype(f32)
        if defect != "reset_before_add":
            c = np.where(d[:, None], c.dtype.type(0), Ec)
        else:
            c = Ec
        x = np.zeros(B, f32)
        for i in range(N):  # the frame's agents in order
            x = x + E[t, :, i]
        inc = np.ones(B, bool) if defect == "not_done_in_sum" else d
        s = np.where(inc, s + x, s).astype(f32)
        k = k + d
        if defect == "carry_from_t_minus_2" and t == T - 2:
            carry_out = np.asarray(c, f32).copy()
    if defect is None or defect not in ("carry_not_written", "carry_from_t_minus_2"):
        carry_out = np.asarray(c).astype(f32)
    S = block_sum(lane_sums(s))
    K = int(k.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = S / (f32(K) if defect == "mean_over_k" else f32(K) * f32(N))
    return dict(E=E, carry=carry_out, S=f32(S), mean=f32(mean), K=K)


def recurrence64(case):
    """The recurrence in float64 from the same float32 inputs: ``(E64 [T,B,N], bound [T,B,N])`` with ``bound = n u A`` -- n the steps of the open episode up to t (the
    incoming carry counts as one), A the sum of |r| (and |carry|) over them: every fp32 addition of the chain rounds a partial sum that is at most A in magnitude."""
    T = case["T"]
    r, done = case["reward"].astype(np.float64), case["done"]
    c, A = case["carry"].astype(np.float64), np.abs(case["carry"]).astype(np.float64)
    n = (case["carry"] != 0).astype(np.float64)
    E, bound = np.zeros(r.shape), np.zeros(r.shape)
    for t in range(T):
        E[t] = c + r[t]
        A, n = A + np.abs(r[t]), n + 1.0
        bound[t] = n * U * A * (1.0 + 2.0 ** -10)
        d = (done[t] != 0)[:, None]
        c, A, n = np.where(d, 0.0, E[t]), np.where(d, 0.0, A), np.where(d, 0.0, n)
    return E, bound


def reference64(case, E):
    """``{"S", "mean", "K", "bound_S", "bound_mean"}`` from the RECORDED float32 ``E`` in float64 (module docstring)"""
    T, B, N = case["T"], case["B"], case["N"]
    d = case["done"] != 0
    K = int(d.sum())
    sel = np.asarray(E, np.float64)[d]  # [K, N]
    S, A = float(sel.sum()), float(np.abs(sel).sum())
    bound_S = longest_chain(T, B, N) * U * A
    if K == 0:
        return dict(S=0.0, mean=float("nan"), K=0, bound_S=0.0, bound_mean=float("nan"))
    return dict(S=S, mean=S / (K * N), K=K, bound_S=bound_S, bound_mean=bound_S / (K * N) + (abs(S) + bound_S) / (K * N) * 2.0 * U / (1.0 - U))


def same_bits(a, b):
    """float32 arrays / scalars equal bit for bit; any NaN equals any NaN"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def check(got, case):
    """``got`` (``E`` may be None: not recorded) against the twin and the float64 reference: a dict of named bars, each True when held"""
    tw = twin(case)
    ref = reference64(case, tw["E"])
    bars = {
        "E_bits": got["E"] is None or same_bits(got["E"], tw["E"]),
        "carry_bits": same_bits(got["carry"], tw["carry"]),
        "S_bits": same_bits(got["S"], tw["S"]),
        "mean_bits": same_bits(got["mean"], tw["mean"]),
        "K_exact": int(got["K"]) == ref["K"] == tw["K"],
        "S_fp64": abs(float(got["S"]) - ref["S"]) <= ref["bound_S"],
    }
    if ref["K"] == 0:
        bars["mean_fp64"] = bool(np.isnan(got["mean"]))
    else:
        bars["mean_fp64"] = bool(abs(float(got["mean"]) - ref["mean"]) <= ref["bound_mean"])
    return bars


def twin_holds_the_recurrence64(case):
    """the twin's record lies within the float64 recurrence's bound everywhere"""
    E64, bound = recurrence64(case)
    return bool((np.abs(twin(case)["E"].astype(np.float64) - E64) <= bound).all())
