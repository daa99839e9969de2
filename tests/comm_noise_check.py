"""The yardstick of communication noise on the propagated actions of the prioritized rollout (sigmaenv_turn_gather_noise_kernel in sigmaenv_wrappers.inc,
comm_noise_seen / comm_noise_std in sigmaenv_dist.h): a plain helper module, numpy only, imported by tests/test_comm_noise_check.py (host) and
tests/test_gpu_comm_noise.py (device).

What is restated (prioritized_ap_policy, sigmarl/helper_training.py:1271-1287).  In turn k of env b the acting agent i = ranks[b, k] sees, in the 2 K = 4 last
columns of its base observation, [a(n0).speed, a(n0).steer, a(n1).speed, a(n1).steer] of its observed neighbours n0, n1 -- zeros for a neighbour that has not
acted yet (combined_action) or an index that is no agent -- plus noise = cat([s_v randn(2), s_d randn(2)]): the std goes by the column's POSITION,
[s_v, s_v, s_d, s_d], with s_v = fl32(max_speed * level) and s_d = fl32(max_steering * level) (Python doubles that multiply a float32 tensor).  Every column
gets a draw.  The draws are the project's: column q takes the cosine branch of the normal pair of draws (DRAW + 2 q, DRAW + 2 q + 1) under the key
(seed, counter0 + t, env_index_base + b, i) (``policy_head_check.rng_u32`` / ``normals``).

The criterion (``bar``), per element, for seen = fl32(v + fl32(std z)) against v + std z in float64 with the float64 draw:

    |seen_dev - (v + std z_64)|  <=  std * Z  +  2^-24 (|std z_64| + std Z)  +  2^-24 (|v + std z_64| + std Z (1 + 2^-24))  + 2^-149

 -- the draw's own error Z seen through the product, one rounding of the product, one of the sum (2^-149: a product that underflows).  Z is the bar
``policy_head_check`` carries for a float32 draw against its float64 value: MARGIN * c * 2^-23 * m, m = |z0| + angle |z1| the magnitude at which the cosine
branch rounds (``normals(magnitude=True)``), c measured on the float32 TWIN of the draw (``normals(dtype=float32)``) against float64 over the rows of the case and
over the calibration keys of ``draw_constant`` (257 x 16 rows x 4 columns, so that a case of few rows cannot be lucky) -- never on the code under test -- and
MARGIN = 4 that module's margin for a device whose logf / cosf need not round as numpy's do.  Nothing here is typed in or fitted to the kernel.
"""
from __future__ import annotations

import numpy as np

import policy_head_check as ph

f32 = np.float32
DRAW = 7500          # sigmaenv_dist.h: DRAW_COMM_NOISE
MAX_COLUMNS = 8      # COMM_NOISE_MAX_COLUMNS: 2 * SIGMAENV_MAX_NEARING
K = 2                # the only K the reference's 4-vector of stds fits
U24 = 2.0 ** -24
MAX_SPEED, MAX_STEERING = 1.0, 31 * np.pi / 180  # AGENTS["max_speed"], AGENTS["max_steering"] (sigmarl/constants.py:637-640), Python doubles


def column_stds(level):
    """[s_v, s_v, s_d, s_d] float32: the double products rounded to float32, by position"""
    s_v, s_d = f32(MAX_SPEED * float(level)), f32(MAX_STEERING * float(level))
    return np.array([s_v, s_v, s_d, s_d], f32)


def seen32(v, std, z):
    """the float32 twin of comm_noise_seen: the product rounded, then the sum rounded"""
    p = np.asarray(std, f32) * np.asarray(z, f32)
    return (np.asarray(v, f32) + p).astype(f32)


def draws(seed, counter, env, agent, ids=None, dtype=np.float64, magnitude=False):
    """z [.., 2 K] of the acting agents (env, agent broadcastable [..]): column q from the draws (DRAW + 2 q, + 2 q + 1), cosine branch.  ``ids``: the first draw
    id per column (a planted defect passes others)."""
    ids = [DRAW + 2 * q for q in range(2 * K)] if ids is None else ids
    env, agent = np.asarray(env, np.uint32), np.asarray(agent, np.uint32)
    return np.stack([ph.normals(seed, counter, env, agent, (d, d + 1), dtype=dtype, magnitude=magnitude)[0] for d in ids], -1)


_CONSTANT = {}


def draw_constant(seed, counter):
    """c of the module docstring on the calibration keys: max |z_32 - z_64| / (2^-23 m) of the float32 twin over 257 x 16 (env, agent) keys x 4 columns"""
    key = (int(seed), int(counter))
    if key not in _CONSTANT:
        env, agent = ph.row_keys(257, 16, 0)
        z, z32, m = draws(seed, counter, env, agent), draws(seed, counter, env, agent, dtype=f32), draws(seed, counter, env, agent, magnitude=True)
        _CONSTANT[key] = float((np.abs(z32.astype(np.float64) - z) / (ph.U23 * m)).max())
    return _CONSTANT[key]


def bar(v, std, z, z32, zmag, seed, counter):
    """(the bound per element, c): the criterion of the module docstring; ``v`` the clean value, ``std`` float32 per column, ``z`` / ``z32`` / ``zmag`` of ``draws``"""
    v, std = np.asarray(v, np.float64), np.asarray(std, f32).astype(np.float64)
    c = max(float((np.abs(np.asarray(z32, np.float64) - z) / (ph.U23 * zmag)).max()), draw_constant(seed, counter))
    Z = ph.MARGIN * c * ph.U23 * zmag
    p = std * z
    return std * Z + U24 * (np.abs(p) + std * Z) + U24 * (np.abs(v + p) + std * Z * (1 + U24)) + 2.0 ** -149, c


def positions(ranks):
    """pos[b, i] = the turn in which agent i acts (N for an agent the ranks never name)"""
    ranks = np.asarray(ranks)
    B, N = ranks.shape
    pos = np.full((B, N), N, np.int64)
    for k in range(N - 1, -1, -1):
        ok = (ranks[:, k] >= 0) & (ranks[:, k] < N)
        pos[np.nonzero(ok)[0], ranks[ok, k]] = k
    return pos


def turn_rows(actions, nearing, ranks, stds, seed, counter, env_index_base=0):
    """The float64 restatement of every agent's turn row of one step.  ``actions [B, N, 2]`` float32: the step's CLEAN actions (the record); ``nearing [B, N, K]``;
    ``ranks [B, N]``; ``stds``: ``column_stds(level)`` or ``[B, 4]`` per env.  Returns dict: ``clean [B, N, 2 K]`` float32 -- what agent i gathers in its turn: the
    action of a neighbour that acted in an earlier turn, else zero --, ``undecided [B, N, 2 K]`` bool (the columns that hold such a zero), ``z`` / ``z32`` / ``zmag``,
    ``std [B, 1, 2 K]``, ``seen`` = clean + std z in float64, ``bound`` and ``c`` of ``bar``."""
    actions, nearing = np.asarray(actions, f32), np.asarray(nearing, np.int64)
    B, N, _ = actions.shape
    assert nearing.shape == (B, N, K)
    pos = positions(ranks)
    valid = (nearing >= 0) & (nearing < N)
    nb = np.where(valid, nearing, 0)
    rows = np.arange(B)[:, None, None]
    decided = valid & (pos[rows, nb] < pos[:, :, None])                      # [B, N, K]: the neighbour acted before agent i
    clean = np.where(decided[..., None], actions[rows, nb], f32(0.0)).reshape(B, N, 2 * K).astype(f32)
    env = (env_index_base + np.arange(B))[:, None] + np.zeros((1, N), np.int64)
    agent = np.arange(N)[None, :] + np.zeros((B, 1), np.int64)
    z, z32, zmag = draws(seed, counter, env, agent), draws(seed, counter, env, agent, dtype=f32), draws(seed, counter, env, agent, magnitude=True)
    std = np.broadcast_to(np.asarray(stds, f32).reshape(-1, 1, 2 * K), (B, 1, 2 * K))
    bound, c = bar(clean, std, z, z32, zmag, seed, counter)
    return dict(clean=clean, undecided=np.repeat(~decided, 2, axis=-1), z=z, z32=z32, zmag=zmag, std=std, seen=clean + std.astype(np.float64) * z, bound=bound, c=c,
                acted=pos < N)


def compare(tentative, base_obs, obs, ref, what=""):
    """One step's records against ``turn_rows``'s ``ref``: ``tentative [B, N, K, 2]``, ``base_obs [B, N, D + 2 K]``, ``obs [B, N, D]`` (the root observation record).
    Returns the figures; ``ok`` = every check holds:
      ``tentative_is_base``  tentative equals the last 2 K columns of base_obs bit for bit
      ``obs_is_base``        the first D columns of base_obs equal obs bit for bit
      ``values``             seen - (clean + std z_64) within the bar on every column of every agent that acted -- at an undecided column the clean value is
                             zero: pure noise -- and finite"""
    tentative, base_obs, obs = np.asarray(tentative, f32), np.asarray(base_obs, f32), np.asarray(obs, f32)
    B, N, D = obs.shape
    bits = lambda a: np.ascontiguousarray(a, f32).view(np.uint32)  # noqa: E731
    seen = base_obs[..., D:]
    acted = ref["acted"][..., None]
    err = np.where(acted, np.abs(seen.astype(np.float64) - ref["seen"]), 0.0)
    r = dict(what=what, rows=int(ref["acted"].sum()), c=ref["c"], err_max=float(err.max()), ratio_max=float((err / ref["bound"]).max()), bound_max=float(ref["bound"].max()),
             undecided=int((ref["undecided"] & acted).sum()),
             tentative_is_base=bool(np.array_equal(bits(tentative.reshape(B, N, 2 * K)), bits(seen))),
             obs_is_base=bool(np.array_equal(bits(base_obs[..., :D]), bits(obs))))
    r["values"] = bool(np.isfinite(seen[np.broadcast_to(acted, seen.shape)]).all() and (err <= ref["bound"]).all())
    r["ok"] = r["tentative_is_base"] and r["obs_is_base"] and r["values"]
    return r


# ---- a host model of one step, with the planted defects ---------------------------------------------------------------------------------------------
DEFECTS = ("stds_by_quantity", "one_draw_for_all_columns", "draw_keyed_by_env_only", "counter_ignored", "noise_written_back", "undecided_left_clean", "actor_draw_ids",
           "clean_base_record")


def model_policy(rows):
    """A fixed float32 stand-in for the actor of the host model: [.., D + 2 K] -> an action [.., 2] in (-1, 1) x (-0.6, 0.6) that depends on every column"""
    rows = np.asarray(rows, f32)
    w = (np.arange(rows.shape[-1], dtype=f32) % f32(7.0) - f32(3.0)) * f32(0.37)
    s = (rows * w).sum(-1, dtype=f32)
    return np.stack([np.tanh(s), f32(0.6) * np.tanh(f32(0.5) * s + f32(0.2))], -1).astype(f32)


def model_step(obs, nearing, ranks, stds, seed, counter, env_index_base=0, defect=None):
    """One step of prioritized action propagation with noise in float32 (the kernels' operations: ``seen32`` on the float32 twin's draws), turn after turn, with
    ``model_policy`` as the actor.  ``defect``: one of ``DEFECTS``, planted.  Returns dict(actions [B, N, 2], tentative [B, N, K, 2], base_obs [B, N, D + 2 K])."""
    assert defect is None or defect in DEFECTS
    obs, nearing, ranks = np.asarray(obs, f32), np.asarray(nearing, np.int64), np.asarray(ranks, np.int64)
    B, N, D = obs.shape
    std = np.broadcast_to(np.asarray(stds, f32).reshape(-1, 2 * K), (B, 2 * K)).copy()
    if defect == "stds_by_quantity":
        std = std[:, [0, 2, 0, 2]]
    ids = [DRAW + 2 * q for q in range(2 * K)]
    if defect == "one_draw_for_all_columns":
        ids = [DRAW] * (2 * K)
    if defect == "actor_draw_ids":
        ids = [ph.ACTOR_DRAWS[0]] * (2 * K)
    actions = np.zeros((B, N, 2), f32)
    tentative, base = np.zeros((B, N, K, 2), f32), np.zeros((B, N, D + 2 * K), f32)
    rows = np.arange(B)
    env = env_index_base + rows
    for k in range(N):
        i = ranks[:, k]
        nb = nearing[rows, i]                                             # [B, K]
        valid = (nb >= 0) & (nb < N)
        so_far = np.where(valid[..., None], actions[rows[:, None], np.where(valid, nb, 0)], f32(0.0)).reshape(B, 2 * K)
        z = draws(seed, 0 if defect == "counter_ignored" else counter, env, np.zeros_like(i) if defect == "draw_keyed_by_env_only" else i, ids, dtype=f32)
        seen = seen32(so_far, std, z)
        if defect == "undecided_left_clean":
            seen = np.where(so_far == 0, so_far, seen)
        row = np.concatenate([obs[rows, i], seen], -1)
        actions[rows, i] = model_policy(row)
        tentative[rows, i] = seen.reshape(B, K, 2)
        base[rows, i] = np.concatenate([obs[rows, i], so_far], -1) if defect == "clean_base_record" else row
        if defect == "noise_written_back":
            for j in range(K):
                ok = valid[:, j]
                actions[rows[ok], nb[ok, j]] = seen.reshape(B, K, 2)[ok, j]
    return dict(actions=actions, tentative=tentative, base_obs=base)


def model_case(B=33, N=5, D=6, seed=0x5EED00000007, counter=2 ** 32 + 9, env_index_base=4000, rng_seed=1):
    """inputs of the host model: observations, a neighbour table with an index that is no agent (-1) in it, a permutation per env"""
    g = np.random.default_rng(rng_seed)
    obs = g.standard_normal((B, N, D)).astype(f32)
    nearing = np.stack([np.stack([g.permutation(np.delete(np.arange(N), i))[:K] for i in range(N)]) for _ in range(B)]).astype(np.int32)
    nearing[0, 0, 1] = -1
    ranks = np.stack([g.permutation(N) for _ in range(B)]).astype(np.int32)
    return dict(obs=obs, nearing=nearing, ranks=ranks, seed=seed, counter=counter, env_index_base=env_index_base)
