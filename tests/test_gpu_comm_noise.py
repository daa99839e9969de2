"""Communication noise on the propagated actions of the prioritized device rollout (``Actor.rollout(wrapper="prioritized", communication_noise=)``,
sigmaenv_turn_gather_noise_kernel) against tests/comm_noise_check.py: every step's noisy rows against the float64 restatement with the recomputed draws, the
clean actions as the actor's own on the recorded rows (no feedback of the noise into the step), level 0, shards, per-env levels, independence of the action
sample, the distribution of the draws, the layers above (``learn.collect`` / ``learn.update``, ``evaluate``, ``evaluate.noise_sweep``) and the refusals.
cpm_entire, is_obs_noise=False, n_nearing_agents_observed=2 throughout.

A shadow env, reset alike and stepped with the rollout's recorded (clean) actions, gives every step's neighbour table and observation."""
import numpy as np
import pytest

import comm_noise_check as cn
import policy_head_check as ph

pytestmark = pytest.mark.gpu

LOW, HIGH = [-1.0, -0.6], [1.0, 0.6]
SEED, COUNTER0 = (0xBEEF << 32) | 21, 2 ** 32 - 1  # a seed with its high word set; the counters of T = 3 steps cross 2^32
LEVEL = 0.1


def make_env(B, N, base=None, **pkw):
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters

    kw = dict(n_agents=N, scenario_type="cpm_entire", is_use_mtv_distance=False, is_obs_noise=False, n_nearing_agents_observed=2, is_using_prioritized_marl=True)
    kw.update(pkw)
    e = SigmaEnv(Parameters(**kw), n_envs=B, device="cuda:0", env_index_base=base)
    e.reset_random(seed=3)
    return e


def make_actor(env, seed=1, in_extra=True):
    import torch
    from sigmarl_amd.actor import Actor, make_mlp

    torch.manual_seed(seed)
    mlp = make_mlp(env.D + (2 * env.K if in_extra else 0))
    with torch.no_grad():  # larger weights: the propagated-action columns move the actions visibly
        for m in mlp:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(1.7)
                m.bias.uniform_(-0.3, 0.3)
    return Actor(mlp, low=LOW, high=HIGH)


def given_ranks(B, N, seed=5):
    import torch

    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(N, generator=g) for _ in range(B)]).to(torch.int32).cuda()


def records(env, T):
    import torch
    from sigmarl_amd.shard import slab_width

    B, N, K, D = env.B, env.N, env.K, env.D
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    return dict(slab=z(T, B, slab_width(N, D)), log_prob=z(T, B, N), actions=z(T, B, N, 2), tentative=z(T, B, N, K, 2), base_obs=z(T, B, N, D + 2 * K), obs_rec=z(T, B, N, D),
                ranks=torch.zeros((T, B, N), dtype=torch.int32, device="cuda"))


def same_bits(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def close(*xs):
    for x in xs:
        x.close()


def shadow_steps(env2, rec, T, seed, counter0):
    """the shadow env through the rollout's steps: yields (t, neighbour table, observation) before step t, then steps with the recorded actions"""
    from sigmarl_amd import capi

    for t in range(T):
        env2.sync()
        yield t, env2.buffer(capi.BUF_NEARING).cpu().numpy().copy(), env2.obs.clone()
        env2.step_autoreset(rec["actions"][t].contiguous(), seed=seed, counter=counter0 + t)
    env2.sync()


# ---- values, and no feedback ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["split", "exact"])
@pytest.mark.parametrize("priority", ["given", "random"])
@pytest.mark.parametrize("B,N", [(1, 3), (8, 4), (65, 4), (48, 16)])
def test_noisy_rows_hold_the_bar_and_the_actions_are_the_actors_on_them(B, N, priority, mode):
    """T = 3.  At every step: tentative[t] is the last 2 K columns of base_obs[t] and its first D columns are obs_rec[t], bit for bit; seen - clean, clean gathered
    from actions[t] through the env's nearing indices, matches std z_64 within the derived bar per column with the positional stds -- at an undecided neighbour:
    pure noise --; and actions[t] / log_prob[t] are what sigmaenv_actor_forward_f32 on all B N rows of base_obs[t] with (seed, counter0 + t) returns, bit for bit:
    the step consumed clean actions, the actor saw the noisy rows (the property that makes the learner's first importance ratio 1)."""
    import torch
    from sigmarl_amd import capi

    env, env2 = make_env(B, N, base=700), make_env(B, N, base=700)
    actor = make_actor(env)
    actor._mlp32.set_mode(mode)
    T, K, D = 3, env.K, env.D
    assert K == cn.K and actor.obs_dim == D + 2 * K and env.cfg.env_index_base == 700
    rec = records(env, T)
    pr = given_ranks(B, N) if priority == "given" else "random"
    actor.rollout(env, T, seed=SEED, counter0=COUNTER0, wrapper="prioritized", priority=pr, communication_noise=LEVEL, **rec)
    env.sync()
    stds = cn.column_stds(LEVEL)
    out_a, out_lp = torch.zeros(B, N, 2, device="cuda"), torch.zeros(B, N, device="cuda")
    undecided = 0
    for t, near, obs in shadow_steps(env2, rec, T, SEED, COUNTER0):
        assert same_bits(obs, rec["obs_rec"][t]), t
        ranks = rec["ranks"][t].cpu().numpy()
        if priority == "random":
            assert np.array_equal(ranks, ph.random_ranks(SEED, COUNTER0 + t, 700 + np.arange(B), N))
        ref = cn.turn_rows(rec["actions"][t].cpu().numpy(), near, ranks, stds, SEED, COUNTER0 + t, 700)
        r = cn.compare(rec["tentative"][t].cpu().numpy(), rec["base_obs"][t].cpu().numpy(), rec["obs_rec"][t].cpu().numpy(), ref, what=f"{B}x{N} {priority} {mode} t={t}")
        print(r)
        assert r["ok"] and r["rows"] == B * N, r
        seen = rec["base_obs"][t][..., D:].cpu().numpy()
        assert (seen[ref["undecided"]] != 0).all()                       # every column got its draw
        undecided += r["undecided"]
        actor.forward(env2, out_a, out_lp, obs=rec["base_obs"][t].reshape(B * N, D + 2 * K).clone(), seed=SEED, counter=COUNTER0 + t)
        env2.sync()
        assert same_bits(out_a, rec["actions"][t]) and same_bits(out_lp, rec["log_prob"][t]), t
    assert undecided >= T * B * 2 * K                                        # the first agent of every env and step sees nothing but noise
    for w in (capi.BUF_OBS, capi.BUF_STATE, capi.BUF_TIMER, capi.BUF_REWARD):
        assert same_bits(env.buffer(w), env2.buffer(w)), w
    close(env, env2, actor)


# ---- level 0 -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["float", "tensor"])
def test_level_zero_is_the_rollout_without_the_argument(form):
    """communication_noise=0.0 (the pair of zeros: noise off) and a [B] tensor of zeros (the noisy kernel with zero stds): every record compares equal to the
    rollout's without the argument"""
    import torch

    B, N, T = 8, 4, 3
    env, env2 = make_env(B, N), make_env(B, N)
    actor = make_actor(env)
    ra, rb = records(env, T), records(env2, T)
    actor.rollout(env, T, seed=SEED, counter0=7, wrapper="prioritized", priority="random", **ra)
    zero = 0.0 if form == "float" else torch.zeros(B, device="cuda")
    actor.rollout(env2, T, seed=SEED, counter0=7, wrapper="prioritized", priority="random", communication_noise=zero, **rb)
    env.sync()
    env2.sync()
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k
    assert (ra["tentative"] == 0).any() and (ra["tentative"] != 0).any()
    close(env, env2, actor)


# ---- shards ------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_shards_equal_one_handle():
    import torch

    T, N = 3, 16
    whole, shards = make_env(48, N, base=0), [make_env(24, N, base=b) for b in (0, 24)]
    actor = make_actor(whole)
    rw, rs = records(whole, T), [records(s, T) for s in shards]
    kw = dict(seed=SEED, counter0=COUNTER0, wrapper="prioritized", priority="random", communication_noise=LEVEL)
    actor.rollout(whole, T, **kw, **rw)
    for s, r in zip(shards, rs):
        actor.rollout(s, T, **kw, **r)
    for e in [whole] + shards:
        e.sync()
    for k in rw:
        assert same_bits(rw[k], torch.cat([rs[0][k], rs[1][k]], dim=1)), k
    assert not same_bits(rs[0]["tentative"], rs[1]["tentative"])
    close(whole, *shards, actor)


# ---- per-env levels --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_per_env_levels_equal_the_scalar_runs_of_the_same_keys(dtype):
    """a [B] tensor with two levels == per group the scalar run (a float32 tensor holds the float32 of 0.1: the scalar run takes that value; a float64 tensor, as
    ``noise_sweep`` passes, holds 0.1 itself)"""
    import torch

    B, N, T, g = 8, 4, 3, 4
    levels = (0.1, 0.3)
    dt = getattr(torch, dtype)
    per_env = torch.tensor(levels, dtype=dt).repeat_interleave(g).cuda()
    envs = [make_env(B, N) for _ in range(3)]
    actor = make_actor(envs[0])
    recs = [records(e, T) for e in envs]
    ranks = given_ranks(B, N)
    kw = dict(seed=SEED, counter0=3, wrapper="prioritized", priority=ranks)
    actor.rollout(envs[0], T, communication_noise=per_env, **kw, **recs[0])
    for k, level in enumerate(levels):
        actor.rollout(envs[1 + k], T, communication_noise=float(np.float32(level)) if dtype == "float32" else level, **kw, **recs[1 + k])
    for e in envs:
        e.sync()
    for k in range(2):
        for name in recs[0]:
            assert same_bits(recs[0][name][:, k * g:(k + 1) * g], recs[1 + k][name][:, k * g:(k + 1) * g]), (k, name)
    assert not same_bits(recs[1]["tentative"], recs[2]["tentative"])
    close(*envs, actor)


# ---- independence of the action sample ---------------------------------------------------------------------------------------------------------------------------
def test_deterministic_actions_draw_the_same_noise():
    """deterministic=True changes the actions and not the noise: where the clean value is 0 -- an undecided neighbour; the whole first turn -- seen - clean is
    identical between the two runs"""
    import torch
    from sigmarl_amd import capi

    B, N = 65, 4
    env, env2 = make_env(B, N), make_env(B, N)
    actor = make_actor(env)
    near = env.buffer(capi.BUF_NEARING).cpu().numpy().copy()
    ranks = given_ranks(B, N)
    ra, rb = records(env, 1), records(env2, 1)
    kw = dict(seed=SEED, counter0=11, wrapper="prioritized", priority=ranks, communication_noise=LEVEL)
    actor.rollout(env, 1, deterministic=False, **kw, **ra)
    actor.rollout(env2, 1, deterministic=True, **kw, **rb)
    env.sync()
    env2.sync()
    assert not torch.equal(ra["actions"], rb["actions"])
    refs = [cn.turn_rows(r["actions"][0].cpu().numpy(), near, ranks.cpu().numpy(), cn.column_stds(LEVEL), SEED, 11) for r in (ra, rb)]
    und = refs[0]["undecided"]
    assert np.array_equal(und, refs[1]["undecided"]) and und.sum() >= B * 4
    first = ranks[:, 0].long().cpu().numpy()
    assert und[np.arange(B), first].all()
    sa, sb = (r["tentative"][0].reshape(B, N, 4).cpu().numpy() for r in (ra, rb))
    assert np.array_equal(sa[und].view(np.uint32), sb[und].view(np.uint32)) and (sa[und] != 0).all()
    assert cn.compare(rb["tentative"][0].cpu().numpy(), rb["base_obs"][0].cpu().numpy(), rb["obs_rec"][0].cpu().numpy(), refs[1])["ok"]
    close(env, env2, actor)


# ---- the distribution of the draws -------------------------------------------------------------------------------------------------------------------------------------
def test_the_noise_is_normal_with_the_positional_stds_and_independent():
    """B = 1024, N = 4, T = 4, fixed seed.  Per column over the undecided-neighbour samples (seen = std z exactly there): |mean| <= 6 std / sqrt(n), |sample std - std|
    <= 6 std / sqrt(2 n), the correlations with the same key's actor draws and with the next column <= 6 / sqrt(n) -- the bars are these formulas of n."""
    B, N, T, seed, counter0 = 1024, 4, 4, 0x5EED0000ABCD, 100
    env, env2 = make_env(B, N), make_env(B, N)
    actor = make_actor(env)
    rec = records(env, T)
    actor.rollout(env, T, seed=seed, counter0=counter0, wrapper="prioritized", priority="random", communication_noise=LEVEL, **rec)
    env.sync()
    stds = cn.column_stds(LEVEL).astype(np.float64)
    seen, und, actor_z = [], [], []
    env_ids, agent_ids = ph.row_keys(B, N, 0)
    for t, near, _ in shadow_steps(env2, rec, T, seed, counter0):
        ref = cn.turn_rows(rec["actions"][t].cpu().numpy(), near, rec["ranks"][t].cpu().numpy(), stds.astype(np.float32), seed, counter0 + t)
        seen.append(rec["tentative"][t].reshape(B, N, 4).cpu().numpy().astype(np.float64))
        und.append(ref["undecided"])
        actor_z.append(np.stack(ph.normals(seed, counter0 + t, env_ids, agent_ids, ph.ACTOR_DRAWS), -1).reshape(B, N, 2))
    seen, und, actor_z = np.stack(seen), np.stack(und), np.stack(actor_z)

    def corr(a, b):
        return float(np.corrcoef(a, b)[0, 1])

    for q in range(4):
        x = seen[..., q][und[..., q]]
        n = x.size
        assert n > T * B                                                   # at least the first agent of every env and step
        print(q, n, x.mean() / stds[q], x.std(ddof=1) / stds[q])
        assert abs(x.mean()) <= 6 * stds[q] / np.sqrt(n)
        assert abs(x.std(ddof=1) - stds[q]) <= 6 * stds[q] / np.sqrt(2 * n)
        for d in range(2):
            assert abs(corr(x, actor_z[..., d][und[..., q]])) <= 6 / np.sqrt(n), (q, d)
        if q < 3:
            both = und[..., q] & und[..., q + 1]
            assert both.sum() > T * B and abs(corr(seen[..., q][both], seen[..., q + 1][both])) <= 6 / np.sqrt(both.sum()), q
    assert abs(np.std(seen[..., 0][und[..., 0]]) / np.std(seen[..., 2][und[..., 2]]) - stds[0] / stds[2]) < 0.05  # columns 0, 1: the speed's std; 2, 3: the steering's
    close(env, env2, actor)


# ---- the layers above -------------------------------------------------------------------------------------------------------------------------------------------------
def test_collect_holds_the_noisy_record_and_update_equals_its_parts_written_out():
    """learn.collect(wrapper="prioritized", priority=PriorityNet, priority_critic=, communication_noise=0.1) at B = 8, N = 4, T = 4: the batch's base observation is
    the rollout's noisy record; one learn.update(priority=...) on it is bit for bit its parts written out (tests/test_gpu_priority_train.py's, on clean rows there)."""
    import torch
    import test_gpu_priority_train as tp
    from sigmarl_amd import learn

    assert (tp.LT, tp.LB, tp.LN) == (4, 8, 4)
    env, env2 = tp._loop_env(), tp._loop_env()
    N, D, K = env.N, env.D, env.K
    nets = tp._Nets(env)
    nets2 = nets.clone()
    ckw = dict(gamma=0.99, lmbda=0.9, seed=5, counter0=0, wrapper="prioritized", priority=nets.pn, priority_critic=nets.pc)
    batch = learn.collect(env, nets.actor, nets.critic, tp.LT, communication_noise=0.1, **ckw)
    env.sync()
    rec = records(env2, tp.LT)
    rec.pop("ranks")
    nets.actor.rollout(env2, tp.LT, seed=5, counter0=0, wrapper="prioritized", priority=nets.pn, communication_noise=0.1, **rec)
    env2.sync()
    base = batch[("info", "base_observation")]
    assert same_bits(base, rec["base_obs"]) and same_bits(base[..., D:].reshape(rec["tentative"].shape), rec["tentative"]) and same_bits(batch["action"], rec["actions"])
    assert same_bits(base[..., :D], batch["observation"])
    first = batch[("info", "priority", "rank")][..., 0].long()                 # the first agent of every env and step sees pure noise, never zeros
    idx = first[..., None, None].expand(tp.LT, tp.LB, 1, 2 * K)
    assert (base[..., D:].gather(2, idx) != 0).all()
    sv, _ = nets.critic.rollout_values(env, batch["slab"], base, tp.LT, pad=(D, D + 2 * K))
    assert same_bits(sv, batch["state_value"])                                 # the base critic read the noisy rows as well
    opt, popt = nets.optims("device")
    opt2, popt2 = nets2.optims("device")
    infos = learn.update(env, nets.actor, nets.critic, nets.amod, nets.cmod, opt, batch, seed=4, counter0=100, generator=torch.Generator(device="cuda").manual_seed(9),
                         priority=nets.priority(popt), **tp.LKW)
    torch.cuda.synchronize()
    k = tp._written_out_update(learn, torch, env, nets2, opt2, popt2, batch, "device", None, torch.Generator(device="cuda").manual_seed(9), 4, 100, infos)
    torch.cuda.synchronize()
    assert k == len(infos) == tp.LEPOCHS * (tp.LT * tp.LB // tp.LMB)
    assert all(tp.same_bits(a, b) for a, b in zip(nets.parameters(), nets2.parameters()))
    assert float(infos[0]["clip_fraction"]) == 0.0                             # the first ratios are 1 to rounding: the learner recomputes the log-probability on the rows the actor saw
    close(nets, nets2, env, env2)


def _eval_setup(B, N=4, T=6, base=None):
    from sigmarl_amd.evaluate import evaluation_parameters
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters

    p = evaluation_parameters(Parameters(n_agents=N, scenario_type="cpm_entire", is_use_mtv_distance=False, is_obs_noise=False, n_nearing_agents_observed=2,
                                         is_using_prioritized_marl=True), simulation_steps=T + 1, num_envs=B)
    return SigmaEnv(p, device="cuda:0", env_index_base=base)


def test_evaluate_with_noise_equals_the_fused_rollout():
    """evaluate(wrapper="prioritized", priority="random", communication_noise=0.2) -- the rollout with the evaluator attached -- against the same reset and the same
    rollout without an evaluator: records and end state bit for bit; and the noise moved the outcome"""
    import torch
    from sigmarl_amd.evaluate import evaluate
    from sigmarl_amd.env import _buf_layout

    B, T = 8, 6
    env, env2 = _eval_setup(B, T=T), _eval_setup(B, T=T)
    actor = make_actor(env)
    ra, rb = records(env, T - 1), records(env2, T - 1)
    kw = dict(wrapper="prioritized", priority="random", communication_noise=0.2)
    out = evaluate(env, actor, seed=7, counter0=30, **kw, **ra)
    env2.reset_random(7, counter=30 + T - 1)
    actor.rollout(env2, T - 1, seed=7, counter0=30, deterministic=True, **kw, **rb)
    env.sync()
    env2.sync()
    for k in ra:
        assert same_bits(ra[k], rb[k]), k
    for which in _buf_layout(B, env.N, env.K, env.D):
        assert same_bits(env.buffer(which), env2.buffer(which)), which
    assert out["frames"] == T and torch.isfinite(out["metrics"]).all()
    clean = evaluate(env, actor, seed=7, counter0=30, wrapper="prioritized", priority="random")
    assert not torch.equal(clean["metrics"], out["metrics"])
    close(env, env2, actor)


def test_noise_sweep_equals_the_scalar_evaluations_of_its_groups():
    import torch
    from sigmarl_amd.evaluate import evaluate, noise_sweep, summarize

    B, T, levels = 8, 6, (0.05, 0.4)
    env = _eval_setup(B, T=T)
    groups = [_eval_setup(B // 2, T=T, base=b) for b in (0, B // 2)]
    actor = make_actor(env)
    kw = dict(seed=7, counter0=30, wrapper="prioritized", priority="random")
    sweep = noise_sweep(env, actor, levels, **kw)
    assert [s["level"] for s in sweep] == list(levels) and [s["envs"] for s in sweep] == [(0, 4), (4, 8)]
    for s, e, level in zip(sweep, groups, levels):
        one = evaluate(e, actor, communication_noise=level, **kw)
        assert same_bits(s["metrics"], one["metrics"]) and same_bits(s["counts"], one["counts"]) and s["frames"] == one["frames"] == T
        assert same_bits(s["average_speed"], one["average_speed"])
        assert torch.isfinite(summarize(s, 0.107, 1.0, is_remove_max_min=True)["AS_avg"])
    with pytest.raises(ValueError, match="groups of equal size"):
        noise_sweep(env, actor, (0.0, 0.1, 0.2), **kw)
    with pytest.raises(TypeError):
        noise_sweep(env, actor, levels, communication_noise=0.1, **kw)
    close(env, *groups, actor)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import types

    import torch
    from sigmarl_amd import capi

    # K = 1 (N = 2) and K = 3: through the parameters, and through the library for an env made without them
    for N, pkw in ((2, dict()), (6, dict(n_nearing_agents_observed=3))):
        env = make_env(4, N, **pkw)
        actor = make_actor(env)
        assert env.K != 2
        with pytest.raises(NotImplementedError, match="raises in the reference as well"):
            actor.rollout(env, 1, wrapper="prioritized", priority="random", communication_noise=LEVEL)
        env.parameters = None
        with pytest.raises(NotImplementedError, match="raises in the reference as well"):
            actor.rollout(env, 1, wrapper="prioritized", priority="random", communication_noise=LEVEL)
        opts = capi.RolloutOpts()
        opts.wrapper, opts.priority_source, opts.comm_noise_std[0] = capi.WRAP_PRIORITIZED, capi.PRIORITY_RANDOM, 0.1
        assert _ex(env, actor, opts) == -22 and b"n_nearing == 2" in env.lib.last_error(env.h)
        actor.rollout(env, 1, wrapper="prioritized", priority="random")     # without noise such an env rolls out
        env.sync()
        close(env, actor)
    # another wrapper
    env = make_env(4, 4, is_using_opponent_modeling=True, is_using_prioritized_marl=False)
    actor = make_actor(env, in_extra=False)
    for w in ("opponent", "plain", None):
        with pytest.raises(ValueError, match="prioritized"):
            actor.rollout(env, 1, wrapper=w, communication_noise=LEVEL)
    for w in (capi.WRAP_OPPONENT, capi.WRAP_PLAIN):
        opts = capi.RolloutOpts()
        opts.wrapper, opts.comm_noise_std[1] = w, 0.1
        assert _ex(env, actor, opts) == -22 and b"SIGMAENV_WRAP_PRIORITIZED only" in env.lib.last_error(env.h)
    close(env, actor)
    # the level: a [B - 1] tensor, another dtype, a CPU tensor, a negative or non-finite float; and the library's own refusal of such a pair
    env = make_env(4, 4)
    actor = make_actor(env)
    kw = dict(wrapper="prioritized", priority="random")
    for bad in (torch.zeros(3, device="cuda"), torch.zeros(4, device="cuda", dtype=torch.float16), torch.zeros(4), "0.1", True):
        with pytest.raises(TypeError, match="communication_noise"):
            actor.rollout(env, 1, communication_noise=bad, **kw)
    for bad in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="finite"):
            actor.rollout(env, 1, communication_noise=bad, **kw)
        opts = capi.RolloutOpts()
        opts.wrapper, opts.priority_source, opts.comm_noise_std[0] = capi.WRAP_PRIORITIZED, capi.PRIORITY_RANDOM, bad
        assert _ex(env, actor, opts) == -22 and b"finite" in env.lib.last_error(env.h)
    # parameters that ask for noise and a call that passes none
    env.parameters.is_communication_noise = True
    with pytest.raises(NotImplementedError, match="would ignore"):
        actor.rollout(env, 1, **kw)
    from sigmarl_amd.params import communication_noise

    actor.rollout(env, 1, communication_noise=communication_noise(env.parameters), **kw)
    env.sync()
    # a library from before the entry point: it would read the fields as reserved words and run without noise
    real = env.lib
    stub = types.SimpleNamespace(**{n: getattr(real, n) for n in real.names if n != "comm_noise_stds" and hasattr(real, n)}, path=real.path, names=real.names)
    env.lib = stub
    try:
        with pytest.raises(RuntimeError, match="does not add communication noise"):
            actor.rollout(env, 1, communication_noise=LEVEL, **kw)
    finally:
        env.lib = real
    # the entry point states the rule
    import ctypes as C

    out = (C.c_float * 4)()
    assert real.comm_noise_stds(LEVEL, out) == 0 and np.array_equal(np.array(list(out), np.float32), cn.column_stds(LEVEL))
    assert real.comm_noise_stds(-1.0, out) == -22 and real.comm_noise_stds(float("nan"), out) == -22 and real.comm_noise_stds(LEVEL, None) == -22
    close(env, actor)


def _ex(env, actor, opts):
    """sigmaenv_rollout_f32_ex with ``opts`` as they are (past the Python checks)"""
    import ctypes as C

    lo, hi = actor._keep[-2], actor._keep[-1]
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    first, count = env.default_paths()
    return env.lib.rollout_f32_ex(env.h, actor._mlp32.handle(env.lib, env), lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), p(actor._scratch_out4(env)), 1,
                                  p(actor._scratch_actions(env)), None, None, None, 0, 0, int(first), int(count), 0, C.byref(opts))
