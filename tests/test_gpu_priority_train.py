"""The device parts of training prioritized action propagation: the priority module's 1-D clip-PPO head (sigmaenv_ppo_head_1d, ``learn.priority_ppo_head``) against
tests/priority_train_check.py -- the float32 twin for what is exact (rows of an index entry outside the records, the clip fraction), the float64 reference within the
criterion --, the base-observation record of the prioritized rollout (``Actor.rollout(base_obs=)``) against the records that already exist, and the base critic's
padded next rows (``Critic.rollout_values(pad=)`` / ``Critic.apply(index=, pad=)``) against the dense calls on rows gathered and padded with torch, bit for bit.

Head shapes (priority_train_check.DEVICE_CASES): one row; 255 and 258 rows, either side of a workgroup boundary; 256 rows of full wavefronts; 16 agents; 129
workgroups with a ragged last one and 130, where the final sum takes its third pass.  Record shapes: B in {1, 3, 65} envs (one row, fewer rows than a wavefront, a
second network tile and several gather workgroups) x N in {1, 3, 4} agents (no neighbour: K = 0, the padded columns are empty; K = 2 with N - 1 = 2 and with more
agents than observed neighbours), T = 2 steps on the CPM map.  Padded rows: 1, 63, 65 and 257 rows (one row, one short of a 64-row tile, one past it, a fifth tile
of one row) of N = 3 agents with K = 2: an odd record row width, so that rows and segments start at every offset of a 16-byte granule.  Loop: B = 8 envs, N = 4,
T = 4 steps (32 frames), minibatches of 8 frames, 2 epochs -- ``learn.collect`` / ``update`` / ``train`` with a priority module against their parts written out."""
import copy
import ctypes as C

import numpy as np
import pytest

import ppo_head_check as pc
import priority_train_check as pt

pytestmark = pytest.mark.gpu

LOW, HIGH = [-1.0, -0.6], [1.0, 0.6]
_envs = {}


def make_env(N, B, **pkw):
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters

    kw = dict(n_agents=N, scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False)
    kw.update(pkw)
    e = SigmaEnv(Parameters(**kw), n_envs=B, device="cuda:0")
    e.reset_random(seed=3)
    return e


@pytest.fixture(scope="module")
def env_of():
    """an env of N agents (the head's rows per frame are the handle's agents), made once per N"""
    def get(N):
        if N not in _envs:
            _envs[N] = make_env(N, 4, max_steps=6)
        return _envs[N]

    yield get
    for e in _envs.values():
        e.close()
    _envs.clear()


def c_head(env, case):
    """sigmaenv_ppo_head_1d on ``case`` (tests/priority_train_check.py): (dout_actor, dout_critic, result[8]) as numpy arrays; every output starts as NaN"""
    import torch
    from sigmarl_amd import capi

    M, N = case["out"].shape[:2]
    assert env.N == N
    dev = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()  # noqa: E731
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")  # noqa: E731
    t = dict(index=dev(case["index"], np.int32), out=dev(case["out"]), value=dev(case["value"]), scores=dev(case["scores"]), score_log_prob=dev(case["score_log_prob"]),
             advantage=dev(case["advantage"]), value_target=dev(case["value_target"]), dout_actor=nan(M, N, 2), dout_critic=nan(M), result=nan(8),
             workspace=nan(capi.PPO_SUMS * ((M * N + 255) // 256)))
    a = capi.PpoHead1dArgs()
    a.n_index, a.n_frames = M, case["scores"].shape[0]
    for k, v in t.items():
        setattr(a, k, v.data_ptr())
    a.clip_epsilon, a.entropy_coeff, a.critic_coeff = float(case["clip_epsilon"]), float(case["entropy_coeff"]), float(case["critic_coeff"])
    a.seed, a.counter = int(case["seed"]), int(case["counter"])
    torch.cuda.synchronize()
    rc = env.lib.ppo_head_1d(env.h, C.byref(a))
    assert rc == 0, env.lib.last_error(env.h)
    env.sync()
    return t["dout_actor"].cpu().numpy(), t["dout_critic"].cpu().numpy(), t["result"].cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize("out_of_range", [False, True])
@pytest.mark.parametrize("M,N", pt.DEVICE_CASES)
def test_head_against_the_twin_and_the_float64_reference(env_of, M, N, out_of_range):
    """Duplicate index entries everywhere (M > 1); ``out_of_range``: one entry outside [0, F), whose rows must come back as exact zeros and add nothing to the sums.
    Against float64: the criterion.  Against the twin, bit for bit: the zeros of that entry and the clip fraction (the flags are 0 or 1: their sum is exact in any
    order; no row of the case lies in the branch band, asserted).  A second launch gives the same bits."""
    env = env_of(N)
    case, ref, c, moved = pt.device_case(M, N, out_of_range)
    assert not pt.in_the_band(ref, c).any()
    idx, F = case["index"], case["scores"].shape[0]
    outside = (idx < 0) | (idx >= F)
    assert int(outside.sum()) == int(out_of_range) and (M == 1 or len(np.unique(idx)) < M)
    da, dc, res = c_head(env, case)
    r, _ = pt.check(da, dc, res, case, what=f"1-D head M={M} N={N} out_of_range={out_of_range}")
    assert r["ambiguous_rows"] == 0 and res[6] == 0 and res[7] == 0
    ta, tc, tres = pt.twin_outputs(case)
    assert np.array_equal(bits(da[outside]), bits(ta[outside])) and not da[outside].any() and not dc[outside].any()
    print(f"clip_fraction {res[4]!r}: {ref['clipped']} of {M * N} rows clipped in float64")
    assert res[4].tobytes() == tres[4].tobytes() == pt.exact_clip_fraction(ref).tobytes()
    da2, dc2, res2 = c_head(env, case)
    assert np.array_equal(bits(da), bits(da2)) and np.array_equal(bits(dc), bits(dc2)) and np.array_equal(bits(res), bits(res2))


def test_head_draws_are_those_of_the_new_id_and_not_the_base_heads(env_of):
    """entropy_coeff = 1 and zero advantages: dout_actor is the entropy sample's gradient alone, 2 tanh(loc + sigma z) / (M N) in its loc half -- a function of the draw
    of every row.  It passes the criterion with the cosine branch of the draws 7350 / 7351 and misses it with the base head's id, with the sine branch and with
    another counter.  Then both heads on the same (seed, counter), index and (loc, raw scale): their loc gradients, each a function of its own z alone, differ."""
    import torch
    from sigmarl_amd import capi

    N, M = 4, 64
    env = env_of(N)
    case = dict(pt.device_case(M, N)[0], entropy_coeff=1.0, counter=11)
    case["advantage"] = np.zeros_like(case["advantage"])
    da, dc, res = c_head(env, case)
    pt.check(da, dc, res, case, what="entropy draws")
    for defect in ("draw_entropy", "sine"):
        want = pt.twin_outputs(case, defect)[0]
        assert np.abs(da[..., 0] - want[..., 0]).max() > 1e3 * np.abs(da[..., 0] - pt.twin_outputs(case)[0][..., 0]).max()
    r, _ = pt.compare(da, dc, res, dict(case, counter=12))
    assert not r["ok"] and r["dloc"] > 1e3
    # the base head on (loc, loc, raw, raw) of the same rows: dimension 0 draws the cosine branch under DRAW_ENTROPY
    F = case["scores"].shape[0]
    dev = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()  # noqa: E731
    out4 = np.concatenate([case["out"][..., :1], case["out"][..., :1], case["out"][..., 1:], case["out"][..., 1:]], -1)
    t = dict(index=dev(case["index"], np.int32), out=dev(out4), value=dev(case["value"]), action=dev(np.zeros((F, N, 2))), sample_log_prob=dev(case["score_log_prob"]),
             advantage=dev(case["advantage"]), value_target=dev(case["value_target"]), dout_actor=dev(np.zeros((M, N, 4))), dout_critic=dev(np.zeros(M)),
             result=dev(np.zeros(8)), workspace=dev(np.zeros(capi.PPO_SUMS)))
    a = capi.PpoHeadArgs()
    a.n_index, a.n_frames = M, F
    for k, v in t.items():
        setattr(a, k, v.data_ptr())
    a.low[0], a.low[1], a.high[0], a.high[1] = -1.0, -1.0, 1.0, 1.0
    a.clip_epsilon, a.entropy_coeff, a.critic_coeff, a.seed, a.counter = 0.2, 1.0, 1.0, int(case["seed"]), 11
    torch.cuda.synchronize()
    assert env.lib.ppo_head(env.h, C.byref(a)) == 0, env.lib.last_error(env.h)
    env.sync()
    base = t["dout_actor"].cpu().numpy()[..., 0]
    zb = pc.draws(dict(case, out=out4), np.float64)[..., 0]  # what the base head drew for dimension 0
    assert np.abs(zb - pt.draws(case)).min() > 0 and np.mean(np.abs(zb - pt.draws(case)) > 0.1) > 0.8
    # (same loc and sigma: the two gradients differ exactly where the draws do -- outside the tanh's saturation)
    assert np.mean(np.abs(base - da[..., 0]) > 1e-3 / (M * N)) > 0.5


def _priority_setup(N, B, seed=1):
    """an env pair (reset alike), an actor on the base observation and a priority network with small weights (scores far from the clamp)"""
    import torch
    from sigmarl_amd.actor import Actor, PriorityNet, make_mlp, make_priority_mlp

    envs = [make_env(N, B, is_using_prioritized_marl=True) for _ in range(2)]
    D, K = envs[0].D, envs[0].K
    assert K == min(2, N - 1)
    torch.manual_seed(seed)
    mlp = make_mlp(D + 2 * K)
    with torch.no_grad():
        for m in mlp:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(1.7)
                m.bias.uniform_(-0.3, 0.3)
    pmlp = make_priority_mlp(D).cuda()
    return torch, envs, Actor(mlp, low=LOW, high=HIGH), pmlp, PriorityNet(pmlp)


def _records(torch, env, T, fill=0.0):
    from sigmarl_amd.shard import slab_width

    B, N, K, D = env.B, env.N, env.K, env.D
    z = lambda *s: torch.full(s, fill, device="cuda")  # noqa: E731
    return dict(slab=z(T, B, slab_width(N, D)), log_prob=z(T, B, N), actions=z(T, B, N, 2), obs_rec=z(T, B, N, D), tentative=z(T, B, N, K, 2))


@pytest.mark.parametrize("N", [1, 3, 4])
@pytest.mark.parametrize("B", [1, 3, 65])
def test_base_observation_record(B, N):
    """base_obs[t, b, i] = the row agent i was evaluated on in its turn of step t: its first D columns are the root observation record, the other 2 K the
    neighbour actions it saw (the ``tentative`` record), bit for bit, and every row is written (the record starts as NaN).  The rollout with the record and the one
    without give the same record rows, actions and log-probabilities.  With priority="random" and with given ranks the record is written as well."""
    torch, (env, env2), actor, pmlp, pn = _priority_setup(N, B)
    T, K, D = 2, env.K, env.D
    nan = float("nan")
    r1, r2 = _records(torch, env, T), _records(torch, env2, T)
    base = torch.full((T, B, N, D + 2 * K), nan, device="cuda")
    actor.rollout(env, T, seed=5, counter0=10, wrapper="prioritized", priority=pn, base_obs=base, **r1)
    actor.rollout(env2, T, seed=5, counter0=10, wrapper="prioritized", priority=pn, **r2)
    env.sync()
    env2.sync()
    same = lambda a, b: a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))  # noqa: E731
    assert not torch.isnan(base).any()
    assert same(base[..., :D], r1["obs_rec"]) and same(base[..., D:], r1["tentative"].reshape(T, B, N, 2 * K))
    assert all(same(r1[k], r2[k]) for k in r1)
    assert torch.isfinite(r1["actions"]).all() and (N == 1 or (r1["tentative"] != 0).any())
    for priority in ("random", torch.stack([torch.randperm(N, generator=torch.Generator().manual_seed(b)) for b in range(B)]).to(torch.int32).cuda()):
        for e in (env, env2):
            e.reset_random(seed=3)
        r3 = _records(torch, env, T)
        base3 = torch.full((T, B, N, D + 2 * K), nan, device="cuda")
        actor.rollout(env, T, seed=5, counter0=10, wrapper="prioritized", priority=priority, base_obs=base3, **r3)
        env.sync()
        assert not torch.isnan(base3).any()
        assert same(base3[..., :D], r3["obs_rec"]) and same(base3[..., D:], r3["tentative"].reshape(T, B, N, 2 * K))
    for e in (env, env2):
        e.close()
    actor.close()
    pn.close()


def test_base_observation_record_refusals_and_ranks_out_of_range():
    """base_obs belongs to the prioritized wrapper and has the padded width; a given rank entry outside [0, N) acts for nobody and is never an address: its turn
    writes no row (the record keeps what it held there) and every other row is written."""
    torch, (env, env2), actor, pmlp, pn = _priority_setup(4, 3)
    T, B, N, K, D = 2, env.B, env.N, env.K, env.D
    with pytest.raises(TypeError, match="base_obs"):
        actor.rollout(env, T, wrapper="prioritized", priority=pn, base_obs=torch.zeros((T, B, N, D), device="cuda"))
    with pytest.raises(ValueError, match="base_obs"):
        actor.rollout(env, T, base_obs=torch.zeros((T, B, N, D + 2 * K), device="cuda"))
    ranks = torch.arange(N, dtype=torch.int32, device="cuda").repeat(B, 1)
    ranks[1, 2], ranks[2, 0] = N, -1  # env 1: agent 2 has no turn; env 2: agent 0 has none
    base = torch.full((T, B, N, D + 2 * K), float("nan"), device="cuda")
    r = _records(torch, env, T)
    actor.rollout(env, T, seed=5, counter0=10, wrapper="prioritized", priority=ranks, base_obs=base, **r)
    env.sync()
    written = ~torch.isnan(base).any(-1)
    want = torch.ones((T, B, N), dtype=torch.bool, device="cuda")
    want[:, 1, 2] = want[:, 2, 0] = False
    assert torch.equal(written, want) and torch.isnan(base[~want]).all()
    assert torch.equal(base[..., :D][want], r["obs_rec"][want])
    for e in (env, env2):
        e.close()
    actor.close()
    pn.close()


def test_unchanged_weights_recompute_the_recorded_log_probability():
    """A prioritized rollout records scores and their log-probabilities; ``learn.priority_ppo_head`` on the same, unchanged priority network (exact mode in the
    rollout, so that ``apply`` -- always the exact chain -- sees the very outputs the scores were drawn from) recomputes the log-probability of every recorded score.

    The bound, per row.  Both values are float32 log-densities of one distribution: the head's through x' = atanh(score), q = (x' - loc) / sigma, the rollout's at its
    own x with q = z.  Each lies within priority_train_check's log-density bound of the float64 value of its arguments (``log_density_bound``: MARGIN c_lw 2^-23 S_lp;
    S_lp carries x = loc + sigma z's own rounding through |q| (|loc| + |x|) / sigma).  Between the two stands the score: the float32 tanhf of x, MARGIN roundings of |y|
    away from tanh(x), seen through atanh as 1 / (1 - y^2) in x and through d logp / d x = -q / sigma + 2 tanh(x) in the log-density.  So
        |logp(head) - score_log_prob| <= 2 MARGIN c_lw 2^-23 S_lp + (|q| / sigma + 2) MARGIN 2^-23 |y| / (1 - y^2).
    Held per row in float64 on the records (reference log-density of the recorded score against the recorded value), and by the head: kl_approx, the mean of
    score_log_prob - logp, within the mean of the bounds plus the sum's own roundings, and clip_fraction == 0 exactly (every bound is far inside log1p(+-0.2))."""
    import torch
    from sigmarl_amd import learn

    N, B, T = 4, 8, 4
    torch, (env, env2), actor, pmlp, pn = _priority_setup(N, B, seed=4)
    pn.set_mode("exact")
    D = env.D
    r = _records(torch, env, T)
    sc, slp = torch.zeros((T, B, N), device="cuda"), torch.zeros((T, B, N), device="cuda")
    actor.rollout(env, T, seed=7, counter0=20, wrapper="prioritized", priority=pn, scores=sc, score_log_prob=slp, **r)
    env.sync()
    M = T * B
    index = torch.arange(M, dtype=torch.int32, device="cuda")
    out = pn.apply(env, rows=(r["obs_rec"], 0, N, D, M, N * D), index=index)
    assert tuple(out.shape) == (M, N, 2) and out.grad_fn is not None
    g = torch.Generator().manual_seed(2)
    adv = torch.randn((T, B, N), generator=g).cuda()
    value = torch.zeros(M, device="cuda", requires_grad=True)
    batch = {("info", "priority", "scores"): sc, ("info", "priority", "sample_log_prob"): slp, "advantage": adv, "value_target": torch.zeros((T, B, N), device="cuda")}
    loss, info = learn.priority_ppo_head(env, out, value, batch, index, clip_epsilon=0.2, entropy_coeff=0.01, seed=3, counter=5)
    loss.backward()
    torch.cuda.synchronize()
    assert set(info) == set(pt.RESULT) and all(p.grad is not None and torch.isfinite(p.grad).all() for p in pmlp.parameters()) and torch.isfinite(value.grad).all()
    case = dict(out=out.detach().cpu().numpy(), value=np.zeros(M, np.float32), index=np.arange(M, dtype=np.int32), scores=sc.reshape(M, N).cpu().numpy(),
                score_log_prob=slp.reshape(M, N).cpu().numpy(), advantage=adv.reshape(M, N).cpu().numpy(), value_target=np.zeros((M, N), np.float32),
                clip_epsilon=0.2, entropy_coeff=0.01, critic_coeff=1.0, seed=3, counter=5)
    ref = pt.head(case)
    c = pt.constants_in_force(case, ref)
    y, sig = ref["y"], ref["sigma"]
    assert np.abs(case["scores"]).max() < 1 - 1e-4  # (no score at the clamp)
    q = (np.arctanh(y) - case["out"][..., 0].astype(np.float64)) / sig
    bound = 2 * pt.log_density_bound(ref, c) + (np.abs(q) / sig + 2) * pt.MARGIN * pt.U23 * np.abs(y) / (1 - y * y)
    err = np.abs(ref["lw"])  # the float64 log-density of the recorded score minus the recorded float32 log-probability
    print(f"unchanged weights: max |lw| {err.max():.3g}, max |lw| / bound {float((err / bound).max()):.3g}, kl_approx {float(info['kl_approx']):.3g}, mean bound {bound.mean():.3g}")
    assert (err <= bound).all()
    assert float(info["clip_fraction"]) == 0.0
    assert abs(float(info["kl_approx"])) <= bound.mean() + (pc.sum_depth(M * N) + 3) * pt.U23 * bound.mean()
    # and the head itself holds its criterion on these tensors (backward scales the stored dout by 1: out.grad is not kept, the twin's clipped count is)
    assert pt.head(case, np.float32)["clipped"] == 0 == ref["clipped"]
    for e in (env, env2):
        e.close()
    actor.close()
    pn.close()


def test_priority_ppo_head_is_the_c_call_with_a_graph(env_of):
    """learn.priority_ppo_head against the C call on the same tensors: the info scalars and, through backward, both dout tensors, bit for bit"""
    import torch
    from sigmarl_amd import learn

    M, N = 85, 3
    env = env_of(N)
    case = pt.device_case(M, N)[0]
    da, dc, res = c_head(env, case)
    F = case["scores"].shape[0]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    out, value = dev(case["out"]).requires_grad_(), dev(case["value"]).requires_grad_()
    batch = {("info", "priority", "scores"): dev(case["scores"]).reshape(1, F, N), ("info", "priority", "sample_log_prob"): dev(case["score_log_prob"]).reshape(1, F, N),
             "advantage": dev(case["advantage"]).reshape(1, F, N), "value_target": dev(case["value_target"]).reshape(1, F, N)}
    index = torch.from_numpy(case["index"]).cuda()
    loss, info = learn.priority_ppo_head(env, out, value, batch, index, clip_epsilon=case["clip_epsilon"], entropy_coeff=case["entropy_coeff"],
                                         critic_coeff=case["critic_coeff"], seed=case["seed"], counter=case["counter"])
    loss.backward()
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.grad.cpu().numpy()), bits(da)) and np.array_equal(bits(value.grad.cpu().numpy()), bits(dc))
    assert all(np.float32(float(info[k])).tobytes() == res[i].tobytes() for i, k in enumerate(pt.RESULT))
    assert np.float32(float(loss.detach())) == (res[0] + res[1]) + res[2]
    with pytest.raises(ValueError, match="out"):
        learn.priority_ppo_head(env, out[:, :, :1], value, batch, index, clip_epsilon=0.2, entropy_coeff=0.0, seed=0, counter=0)
    with pytest.raises(TypeError, match="index"):
        learn.priority_ppo_head(env, out, value, batch, index.long(), clip_epsilon=0.2, entropy_coeff=0.0, seed=0, counter=0)


# ---- the base critic's padded next rows -----------------------------------------------------------------------------------------------------------
PAD_N = 3


def _padded_setup(T, B, seed=0):
    """an env of B x 3 agents, synthetic records of T steps (slab [T, B, W], base observations [T, B, N, Dc]) and a critic on N Dc inputs (module on the device)"""
    import torch
    from sigmarl_amd.actor import Critic, make_mlp

    env = make_env(PAD_N, B, is_using_prioritized_marl=True)
    N, D, K = env.N, env.D, env.K
    Dc, W = D + 2 * K, N * (D + 1) + 1
    g = torch.Generator().manual_seed(10 + seed)
    slab = ((torch.rand((T, B, W), generator=g) * 2 - 1) * 1.5).cuda()
    base = ((torch.rand((T, B, N, Dc), generator=g) * 2 - 1) * 1.5).cuda()
    torch.manual_seed(20 + seed)
    cmod = make_mlp(N * Dc, n_out=1)
    with torch.no_grad():
        for m in cmod:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(1.5)
                m.bias.uniform_(-0.3, 0.3)
    cmod = cmod.cuda()
    return torch, env, slab, base, cmod, Critic(cmod)


def _torch_padded(torch, slab, N, D, K):
    """[T, B, N (D + 2 K)]: the record's next observations with every agent's 2 K placeholder columns zero, as a dense copy"""
    T, B = slab.shape[:2]
    return torch.nn.functional.pad(slab[:, :, : N * D].reshape(T, B, N, D), (0, 2 * K)).reshape(T, B, N * (D + 2 * K)).contiguous()


def same_bits(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("mode", ["split", "exact"])
@pytest.mark.parametrize("T,B", [(1, 1), (3, 21), (1, 65), (1, 257)])
def test_rollout_values_on_padded_rows_equal_the_dense_call(T, B, mode):
    """Critic.rollout_values(pad=(D, Dc)): state values from the base-observation record as it lies, next values from the record rows staged padded -- both bit for
    bit ``forward`` on the dense rows (the next rows gathered and padded with torch), in the mode in force; the rewards and the done flag behind the observations and
    NaNs planted in them never reach the network."""
    torch, env, slab, base, cmod, critic = _padded_setup(T, B)
    N, D, K = env.N, env.D, env.K
    assert critic.set_mode(mode) == mode
    slab[:, :, N * D:] = float("nan")  # (reward and done columns: not part of any row)
    sv, nv = critic.rollout_values(env, slab, base, T, pad=(D, D + 2 * K))
    dense = _torch_padded(torch, slab, N, D, K)
    want_nv = critic.forward(env, dense.reshape(T * B, -1)).reshape(T, B)
    want_sv = critic.forward(env, base.reshape(T * B, -1)).reshape(T, B)
    env.sync()
    assert tuple(nv.shape) == (T, B) and torch.isfinite(nv).all()
    assert same_bits(nv, want_nv) and same_bits(sv, want_sv)
    with pytest.raises(ValueError, match="pad"):
        critic.rollout_values(env, slab, base, T, pad=(D + 1, D + 2 * K))
    env.close()
    critic.close()


@pytest.mark.parametrize("M", [1, 63, 65, 257])
def test_apply_on_padded_rows_equals_the_dense_call_in_values_and_gradients(M):
    """Critic.apply(slab, index=, pad=(D, Dc)) on M frames picked with duplicates out of 70: the values and every parameter gradient bit for bit those of
    ``Mlp32.apply`` on the same frames gathered and padded dense (the same saving forward and backward on dense rows); on the base-observation record ``pad`` changes
    nothing.  An index entry outside the record is refused on the host."""
    from sigmarl_amd.actor import Mlp32

    T, B = 2, 35
    torch, env, slab, base, cmod, critic = _padded_setup(T, B, seed=M)
    N, D, K = env.N, env.D, env.K
    Dc, F = D + 2 * K, T * B
    g = torch.Generator().manual_seed(M)
    index = torch.randint(0, F, (M,), generator=g).to(torch.int32).cuda()
    if M > 1:
        index[-1] = index[0]
    dout = (torch.randn((M,), generator=g) / M).cuda()
    pars = list(cmod.parameters())
    v = critic.apply(env, slab, index=index, pad=(D, Dc))
    assert tuple(v.shape) == (M,) and v.grad_fn is not None
    (v * dout).sum().backward()
    got = [p.grad.clone() for p in pars]
    for p in pars:
        p.grad = None
    dense = _torch_padded(torch, slab, N, D, K).reshape(F, N * Dc).index_select(0, index.long()).contiguous()
    vd = Mlp32.apply(critic, env, dense).view(-1)
    (vd * dout).sum().backward()
    torch.cuda.synchronize()
    assert same_bits(v.detach(), vd.detach())
    assert all(same_bits(a, p.grad) for a, p in zip(got, pars)) and all(torch.isfinite(a).all() for a in got)
    # the columns of the padding carry no gradient into the first layer
    assert not got[0].reshape(-1, N, Dc)[:, :, D:].any() and got[0].reshape(-1, N, Dc)[:, :, :D].any()
    # the base-observation record holds the padded rows themselves
    vb = critic.apply(env, base, index=index, pad=(D, Dc))
    assert same_bits(vb.detach(), Mlp32.apply(critic, env, base.reshape(F, N * Dc).index_select(0, index.long()).contiguous()).view(-1).detach())
    with pytest.raises(ValueError, match="index"):
        critic.apply(env, slab, index=torch.tensor([F], dtype=torch.int32, device="cuda"), pad=(D, Dc))
    with pytest.raises(TypeError, match="index"):
        critic.apply(env, slab, pad=(D, Dc))
    env.close()
    critic.close()


# ---- the loop: collect, update and train with a priority module ---------------------------------------------------------------------------------
LT, LB, LN, LMB, LEPOCHS = 4, 8, 4, 8, 2
LKW = dict(num_epochs=LEPOCHS, minibatch_size=LMB, clip_epsilon=0.2, entropy_coeff=1e-2, max_grad_norm=1.0)


class _Nets:
    """the four networks of the configuration and their torch modules (on the device): base actor and critic on the base observation, priority actor and critic on
    the priority observation; ``clone()``: a second set with the same weights"""

    def __init__(self, env, modules=None):
        import torch
        from sigmarl_amd.actor import Actor, Critic, PriorityNet, make_mlp, make_priority_mlp

        N, D, Dc = env.N, env.D, env.D + 2 * env.K
        if modules is None:
            torch.manual_seed(1)
            modules = [make_mlp(Dc).cuda(), make_mlp(N * Dc, n_out=1).cuda(), make_priority_mlp(D).cuda(), make_mlp(N * D, n_out=1).cuda()]
        self.env, self.modules = env, modules
        self.amod, self.cmod, self.pmod, self.pcmod = modules
        self.actor, self.critic, self.pn, self.pc = Actor(self.amod, low=LOW, high=HIGH), Critic(self.cmod), PriorityNet(self.pmod), Critic(self.pcmod)

    def clone(self):
        return _Nets(self.env, [copy.deepcopy(m) for m in self.modules])

    def optims(self, route, lr=3e-4):
        import torch
        from sigmarl_amd import learn

        if route == "device":
            return learn.Adam(self.env, [(self.actor, self.amod), (self.critic, self.cmod)], lr=lr), learn.Adam(self.env, [(self.pn, self.pmod), (self.pc, self.pcmod)], lr=lr)
        return (torch.optim.Adam(list(self.amod.parameters()) + list(self.cmod.parameters()), lr=lr),
                torch.optim.Adam(list(self.pmod.parameters()) + list(self.pcmod.parameters()), lr=lr))

    def priority(self, popt):
        return (self.pn, self.pc, self.pmod, self.pcmod, popt)

    def parameters(self):
        return [p for m in self.modules for p in m.parameters()]

    def close(self):
        for n in (self.actor, self.critic, self.pn, self.pc):
            n.close()


def _loop_env():
    return make_env(LN, LB, is_using_prioritized_marl=True, max_steps=6)


def _written_out_update(learn, torch, env, nets, opt, popt, batch, route, buffer, gen, seed, counter0, infos=None):
    """learn.update(priority=...)'s steps with the public pieces; compares every step's scalars with ``infos`` when given"""
    N, D, K = env.N, env.D, env.K
    Dc, frames = D + 2 * K, LT * LB
    obs, base = batch["observation"], batch[("info", "base_observation")]
    pars, ppars = list(nets.amod.parameters()) + list(nets.cmod.parameters()), list(nets.pmod.parameters()) + list(nets.pcmod.parameters())
    k = 0
    for _ in range(LEPOCHS):
        chunks = [None] * (frames // LMB) if buffer is not None else learn.minibatches(frames, LMB, gen, env.device)[: frames // LMB]
        for idx in chunks:
            if buffer is not None:
                idx, weight = buffer.sample(LMB, seed, counter0 + k)
            out = nets.actor.apply(env, rows=(base, 0, N, Dc, frames, N * Dc), index=idx)
            value = nets.critic.apply(env, base, index=idx, pad=(D, Dc))
            loss, info = learn.ppo_head(env, out, value, batch, idx, low=LOW, high=HIGH, clip_epsilon=0.2, entropy_coeff=1e-2, seed=seed, counter=counter0 + k)
            loss.backward()
            if route == "device":
                opt.step(1.0)
            else:
                torch.nn.utils.clip_grad_norm_(pars, 1.0)
                opt.step()
                opt.zero_grad()
                nets.actor.load(env, nets.amod)
                nets.critic.load(env, nets.cmod)
            pout = nets.pn.apply(env, rows=(obs, 0, N, D, frames, N * D), index=idx)
            pvalue = nets.pc.apply(env, obs, index=idx)
            ploss, pinfo = learn.priority_ppo_head(env, pout, pvalue, batch, idx, clip_epsilon=0.2, entropy_coeff=1e-2, seed=seed, counter=counter0 + k)
            ploss.backward()
            if route == "device":
                popt.step(1.0)
            else:
                torch.nn.utils.clip_grad_norm_(ppars, 1.0)
                popt.step()
                popt.zero_grad()
                nets.pn.load(env, nets.pmod)
                nets.pc.load(env, nets.pcmod)
            td = buffer.refresh(nets.critic, batch, idx) if buffer is not None else None
            if infos is not None:
                for key in ("loss_objective", "loss_entropy", "loss_critic", "entropy", "kl_approx"):
                    assert same_bits(info[key], infos[k][key]) and same_bits(pinfo[key], infos[k]["priority"][key]), (k, key)
                if buffer is not None:
                    assert same_bits(td, infos[k]["td_error"]) and same_bits(weight, infos[k]["_weight"])
            k += 1
    if route == "device":
        opt.resolve()
        popt.resolve()
    return k


@pytest.mark.parametrize("with_buffer", [False, True])
@pytest.mark.parametrize("route", ["device", "torch"])
def test_update_with_a_priority_module_equals_its_steps_written_out(route, with_buffer):
    """learn.collect(wrapper="prioritized", priority=, priority_critic=) -> learn.update(priority=...): bit for bit the loop written out with the public pieces (every
    step's scalars of both heads, the refreshed TD errors, every parameter of the four networks); ``advantage`` is the priority critic's pair and ``base_advantage`` the
    base critic's, each ``learn.gae`` on its own values; every parameter moves; after the update (and, on the device route, its ``resolve``) the priority actor and
    critic compute what fresh networks built from the torch-side parameters compute, and not what they computed before."""
    import torch
    from sigmarl_amd import learn
    from sigmarl_amd.actor import Critic, PriorityNet

    env = _loop_env()
    N, D, K = env.N, env.D, env.K
    Dc, frames = D + 2 * K, LT * LB
    nets = _Nets(env)
    nets2 = nets.clone()
    batch = learn.collect(env, nets.actor, nets.critic, LT, gamma=0.99, lmbda=0.9, seed=5, counter0=0, wrapper="prioritized", priority=nets.pn, priority_critic=nets.pc)
    env.sync()
    # the batch: the keys, and the two pairs
    for key, shape in (((("info", "base_observation")), (LT, LB, N, Dc)), (("info", "priority", "scores"), (LT, LB, N)), (("info", "priority", "sample_log_prob"), (LT, LB, N)),
                       (("info", "priority", "rank"), (LT, LB, N)), (("info", "priority", "state_value"), (LT, LB)), (("next", "info", "priority", "state_value"), (LT, LB)),
                       ("base_advantage", (LT, LB, N)), ("base_value_target", (LT, LB, N)), ("td_error", (LT, LB))):
        assert tuple(batch[key].shape) == shape, key
    slab, obs, base = batch["slab"], batch["observation"], batch[("info", "base_observation")]
    assert same_bits(base[..., :D], obs) and torch.equal(torch.sort(batch[("info", "priority", "rank")].long(), dim=-1).values, torch.arange(N, device="cuda").expand(LT, LB, N))
    psv, pnv = nets.pc.rollout_values(env, slab, obs, LT)
    assert same_bits(psv, batch[("info", "priority", "state_value")]) and same_bits(pnv, batch[("next", "info", "priority", "state_value")])
    padv, pvt, _ = learn.gae(env, slab, psv, pnv, 0.99, 0.9)
    assert same_bits(padv, batch["advantage"]) and same_bits(pvt, batch["value_target"])
    sv, nv = nets.critic.rollout_values(env, slab, base, LT, pad=(D, Dc))
    dense_next = _torch_padded(torch, slab, N, D, K)
    assert same_bits(sv, batch["state_value"]) and same_bits(nv, batch[("next", "state_value")]) and same_bits(nv, nets.critic.forward(env, dense_next.reshape(frames, -1)).reshape(LT, LB))
    badv, bvt, td = learn.gae(env, slab, sv, nv, 0.99, 0.9, td_error=True)
    assert same_bits(badv, batch["base_advantage"]) and same_bits(bvt, batch["base_value_target"]) and same_bits(td, batch["td_error"])
    assert not same_bits(padv, badv)
    # the update
    x = obs.reshape(frames * N, D)[:70].contiguous()
    xc = obs.reshape(frames, N * D).contiguous()
    before = [p.detach().clone() for p in nets.parameters()]
    y0, v0 = nets.pn.forward(env, x).clone(), nets.pc.forward(env, xc).clone()
    opt, popt = nets.optims(route)
    opt2, popt2 = nets2.optims(route)
    buf = buf2 = None
    if with_buffer:
        buf, buf2 = learn.PrioritizedBuffer(env, frames), learn.PrioritizedBuffer(env, frames)
        buf.extend(batch["td_error"])
        buf2.extend(batch["td_error"])
    infos = learn.update(env, nets.actor, nets.critic, nets.amod, nets.cmod, opt, batch, seed=4, counter0=100, generator=torch.Generator(device="cuda").manual_seed(9),
                         buffer=buf, priority=nets.priority(popt), **LKW)
    torch.cuda.synchronize()
    steps = LEPOCHS * (frames // LMB)
    assert len(infos) == steps and all(set(i["priority"]) == set(pt.RESULT) for i in infos)
    assert all(np.isfinite(float(i[k])) and np.isfinite(float(i["priority"][k])) for i in infos for k in pt.RESULT)
    after = nets.parameters()
    assert all(not torch.equal(a, b) and torch.isfinite(b).all() for a, b in zip(before, after))
    if route == "device":
        assert opt.t == popt.t == steps
    k = _written_out_update(learn, torch, env, nets2, opt2, popt2, batch, route, buf2, torch.Generator(device="cuda").manual_seed(9), 4, 100, infos)
    torch.cuda.synchronize()
    assert k == steps and all(same_bits(a, b) for a, b in zip(after, nets2.parameters()))
    if with_buffer:
        assert torch.equal(buf.priorities(), buf2.priorities())
    # the packed weights: moved, and those of fresh networks built from the torch-side parameters
    fresh_pn, fresh_pc = PriorityNet(copy.deepcopy(nets.pmod).cpu()), Critic(copy.deepcopy(nets.pcmod).cpu())
    for mode in ("exact", "split"):
        for net, fresh, inp, old in ((nets.pn, fresh_pn, x, y0), (nets.pc, fresh_pc, xc, v0)):
            assert net.set_mode(mode) == mode and fresh.set_mode(mode) == mode
            got = net.forward(env, inp)
            assert same_bits(got, fresh.forward(env, inp)) and (mode == "exact" or not same_bits(got, old))
    for n in (nets, nets2):
        n.close()
    for n in (fresh_pn, fresh_pc):
        n.close()
    for b in (buf, buf2):
        if b is not None:
            b.close()
    env.close()


def test_two_iterations_of_train_equal_the_parts_written_out():
    """learn.train on the is_using_prioritized_marl / "marl" configuration, device route: two iterations equal collect -> update -> the learning rate written out
    on a second env (the reported means, every parameter of the four networks bit for bit); the next learning rate goes into the base optimiser alone."""
    import torch
    from sigmarl_amd import learn
    from sigmarl_amd.params import rollout_wrapper

    env, env2 = _loop_env(), _loop_env()
    p = env.parameters
    assert rollout_wrapper(p) == "prioritized" and p.prioritization_method == "marl"
    p.n_iters, p.lr, p.lr_min = 5, 3e-4, 1e-5
    nets = _Nets(env)
    nets2 = _Nets(env2, [copy.deepcopy(m) for m in nets.modules])
    opt, popt = nets.optims("device", p.lr)
    opt2, popt2 = nets2.optims("device", p.lr)
    fpb = LT * LB
    means = learn.train(env, nets.actor, nets.critic, nets.amod, nets.cmod, opt, p, n_iters=2, frames_per_batch=fpb, seed=6, counter0=50,
                        generator=torch.Generator(device="cuda").manual_seed(3), rollout_kw=dict(wrapper="prioritized"), priority=nets.priority(popt), **LKW)
    torch.cuda.synchronize()
    returns2, gen2, means2 = learn.EpisodeReturns(env2), torch.Generator(device="cuda").manual_seed(3), []
    steps = learn.steps_per_iteration(p, fpb, LEPOCHS, LMB)
    for i in (1, 2):
        batch = learn.collect(env2, nets2.actor, nets2.critic, LT, params=p, seed=6, counter0=50 + (i - 1) * LT, returns=returns2, wrapper="prioritized", priority=nets2.pn,
                              priority_critic=nets2.pc)
        infos = learn.update(env2, nets2.actor, nets2.critic, nets2.amod, nets2.cmod, opt2, batch, params=p, seed=6, counter0=50 + (i - 1) * steps, generator=gen2,
                             priority=nets2.priority(popt2), **LKW)
        assert len(infos) == steps
        learn.set_lr(opt2, learn.lr_at(p, i + 1))
        means2.append(learn.EpisodeReturns.mean(batch["episode_stats"]))
    torch.cuda.synchronize()
    assert len(means) == 2 and all(a == b or (a != a and b != b) for a, b in zip(means, means2))
    assert all(same_bits(a, b) for a, b in zip(nets.parameters(), nets2.parameters()))
    assert opt.t == popt.t == 2 * steps and opt.lr == learn.lr_at(p, 3) and popt.lr == p.lr
    for n in (nets, nets2):
        n.close()
    env.close()
    env2.close()
