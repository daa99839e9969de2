"""The episode return on the device (sigmaenv_episode_return, ``learn.EpisodeReturns``, ``learn.collect(returns=)``) held to tests/episode_check.py -- the record E and
the carry bit for bit to the float32 twin, S and the mean bit for bit to the twin and within the derived bound of float64, K exact --, and the training iteration
(``learn.train_iteration`` / ``learn.train``) held bit for bit to its parts written out.

Synthetic records (hand-made slabs on envs that only lend their B, N, D): T in {1, 2, 33}; N in {1, 4, 16} x B in {1, 3, 48, 257}, so that B * N lies below, at and
off multiples of 64 and 256, plus the lane mappings with idle lanes -- N = 3 (21 envs per wavefront, one idle lane), N = 5 (12 envs, four idle), N = 33 (one env,
31 idle); every done pattern of the yardstick, with a zero and a non-zero incoming carry.  The last sum adds the envs' sums in one workgroup of EPR_LANES lanes, each
lane a chain over b = l, l + EPR_LANES, ..: B = EPR_LANES (one term per lane: one workgroup's worth), EPR_LANES + 1 (one more: the first chain of two) and
2 EPR_LANES + 1 (the first chain of three) with every frame done take it through every pass it has; an env's own chain has 0, 1, 2 and T terms."""
import copy

import numpy as np
import pytest

import episode_check as ec

pytestmark = pytest.mark.gpu

LOW, HIGH = [-1.0, -0.6], [1.0, 0.6]
KW = dict(scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False, max_steps=6)
SHAPES = [(N, B) for N in (1, 4, 16) for B in (1, 3, 48, 257)] + [(3, 48), (5, 33), (33, 3)]
STEPS = (1, 2, 33)


def same(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_envs = {}


def lend(N, B):
    """an env of N agents x B envs, made once: the synthetic cases use its handle (B, N, D), never its state"""
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters

    if (N, B) not in _envs:
        _envs[(N, B)] = SigmaEnv(Parameters(n_agents=N, **KW), n_envs=B, device="cuda:0")
    return _envs[(N, B)]


@pytest.fixture(scope="module", autouse=True)
def close_envs():
    yield
    for e in _envs.values():
        e.close()
    _envs.clear()


def run_device(env, case, record=None, guard=False):
    """the case through ``EpisodeReturns.update``: ``{"E", "carry", "S", "mean", "K"}`` as numpy (``E`` None when not recorded); ``guard``: the record is a slice of
    a wider tensor whose other half must stay untouched"""
    import torch
    from sigmarl_amd import learn

    T, B, N = case["T"], case["B"], case["N"]
    slab = torch.from_numpy(case["slab"]).cuda()
    er = learn.EpisodeReturns(env)
    er.carry.copy_(torch.from_numpy(case["carry"]))
    whole = None
    if guard:
        whole = torch.full((2, T, B, N), -7.0, device="cuda")
        record = whole[0]
    E, stats = er.update(slab, T, env_first=case["env_first"], episode_reward=record)
    torch.cuda.synchronize()
    assert set(stats) == {"episode_reward_mean", "episode_reward_sum", "episodes_done"} and all(v.is_cuda and v.dim() == 0 for v in stats.values())
    if guard:
        assert (whole[1] == -7.0).all()
    return dict(E=None if E is None else E.cpu().numpy(), carry=er.carry.cpu().numpy(), S=stats["episode_reward_sum"].cpu().numpy(),
                mean=stats["episode_reward_mean"].cpu().numpy(), K=int(stats["episodes_done"].item()))


def hold(env, case, what):
    got = run_device(env, case)
    bars = ec.check(got, case)
    ref = ec.reference64(case, got["E"])
    print(what, "K", got["K"], "S", got["S"], "S64", ref["S"], "bound", ref["bound_S"], "mean", got["mean"], "mean64", ref["mean"], "bound", ref["bound_mean"])
    assert all(bars.values()), (what, bars)
    return got


@pytest.mark.parametrize("N,B", SHAPES)
def test_synthetic_records_equal_the_twin_and_hold_the_fp64_bound(N, B):
    env = lend(N, B)
    D = env.D
    for T in STEPS:
        for k, pattern in enumerate(ec.PATTERNS):
            case = ec.make_case(T, B, N, D, pattern, seed=1000 * T + 10 * k + N, carry=bool((k + T) % 2))
            got = hold(env, case, (N, B, T, pattern))
            if pattern == "none":
                assert got["K"] == 0 and np.isnan(got["mean"]) and got["S"] == 0.0
            if pattern == "all":
                assert got["K"] == T * B and not got["carry"].any()
    # two runs give identical bits; without the record the same result and carry
    case = ec.make_case(33, B, N, D, "mixed", seed=7 + N + B, carry=True)
    a, b, c = run_device(env, case), run_device(env, case), run_device(env, case, record=False)
    assert c["E"] is None
    for k in ("carry", "S", "mean"):
        assert ec.same_bits(a[k], b[k]) and ec.same_bits(a[k], c[k]), k
    assert ec.same_bits(a["E"], b["E"]) and a["K"] == b["K"] == c["K"]


def test_the_last_sum_through_every_pass_it_has():
    """B = EPR_LANES, EPR_LANES + 1, 2 EPR_LANES + 1 envs with every frame done, then with 0, 1, 2 and T done steps per env"""
    from sigmarl_amd import capi

    L = capi.EPR_LANES
    assert L == ec.LANES
    for B in (L, L + 1, 2 * L + 1):
        env = lend(2, B)
        got = hold(env, ec.make_case(3, B, 2, env.D, "all", seed=B, carry=True), ("all", B))
        assert got["K"] == 3 * B
        for per_env in (0, 1, 2, 5):
            got = hold(env, ec.done_count_case(5, B, 2, env.D, per_env, seed=B + per_env), ("per_env", B, per_env))
            assert got["K"] == per_env * B


def test_a_record_buffer_wider_than_the_handle():
    """Bt = 2 B, env_first = B: the handle's envs are the second half of every step's block; the other half of a guarded output is untouched"""
    N, B = 4, 48
    env = lend(N, B)
    case = ec.make_case(7, B, N, env.D, "mixed", seed=5, carry=True, Bt=2 * B, env_first=B)
    got = run_device(env, case, guard=True)
    assert all(ec.check(got, case).values()), ec.check(got, case)
    narrow = dict(case, slab=np.ascontiguousarray(case["slab"][:, B:]), env_first=0)  # the same envs in a buffer of their own
    alone = run_device(env, narrow)
    assert all(ec.same_bits(got[k], alone[k]) for k in ("E", "carry", "S", "mean"))
    lower = dict(case, env_first=0)  # the buffer's OTHER half holds no rewards of the case: reading it gives other numbers
    assert not ec.same_bits(run_device(env, lower)["E"], got["E"])


def test_refusals_of_the_library():
    import ctypes as C

    import torch
    from sigmarl_amd import capi

    env = lend(4, 3)
    W = env.N * (env.D + 1) + 1
    slab, carry, result = torch.zeros(2, 3, W, device="cuda"), torch.zeros(3, 4, device="cuda"), torch.zeros(4, device="cuda")
    good = dict(n_steps=2, slab=slab.data_ptr(), slab_stride=0, carry=carry.data_ptr(), result=result.data_ptr())
    for bad in (dict(n_steps=0), dict(n_steps=(1 << 24) // 3 + 1), dict(slab_stride=3 * W - 1), dict(carry=None), dict(slab=None), dict(result=None),
                dict(carry=carry.data_ptr() + 2)):
        a = capi.EpisodeArgs()
        for k, v in dict(good, **bad).items():
            setattr(a, k, v)
        assert env.lib.episode_return(env.h, C.byref(a)) == -22, bad
        assert b"episode_return" in env.lib.last_error(env.h)
    torch.cuda.synchronize()
    assert not carry.any() and not result.any()


# ---- a real env: the carry across rollouts ---------------------------------------------------------------------------------------------
def _networks(env, seed=1):
    import torch
    from sigmarl_amd.actor import Actor, Critic, make_mlp

    torch.manual_seed(seed)
    amod, cmod = make_mlp(env.D).cuda(), make_mlp(env.N * env.D, n_out=1).cuda()
    return amod, cmod, Actor(amod, low=LOW, high=HIGH), Critic(cmod)


def test_two_rollouts_in_a_row_equal_one_restatement_over_both():
    """max_steps = 6, B = 48, N = 16: two collect(T = 10, returns=) calls equal the 20-step restatement over the concatenated slabs bit for bit -- the twin's and the
    device's own --, on a workload in which episodes span the boundary"""
    import torch
    from sigmarl_amd import learn
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters

    env = SigmaEnv(Parameters(n_agents=16, **KW), n_envs=48, device="cuda:0")
    env.reset_random(seed=3)
    amod, cmod, actor, critic = _networks(env)
    T, B, N, D = 10, env.B, env.N, env.D
    er = learn.EpisodeReturns(env)
    first = learn.collect(env, actor, critic, T, gamma=0.99, lmbda=0.9, seed=5, counter0=0, returns=er)
    carry1 = er.carry.clone()
    second = learn.collect(env, actor, critic, T, gamma=0.99, lmbda=0.9, seed=5, counter0=T, returns=er)
    plain = learn.collect(env, actor, critic, 2, gamma=0.99, lmbda=0.9, seed=5, counter0=2 * T)  # without returns=: nothing new
    torch.cuda.synchronize()
    assert ("next", "episode_reward") not in plain and "episode_stats" not in plain
    slab = torch.cat([first["slab"], second["slab"]])
    E = torch.cat([first[("next", "episode_reward")], second[("next", "episode_reward")]])
    assert tuple(E.shape) == (2 * T, B, N)
    done, reward = slab[:, :, N * D + N], slab[:, :, N * D: N * D + N]
    assert same(done, torch.cat([first[("next", "done")], second[("next", "done")]]))
    # an episode spans the boundary: open after the first rollout's last step, with a return so far, which the second rollout's first frame continues
    spans = (done[T - 1] == 0) & (carry1 != 0).any(dim=1)
    assert spans.any(), "no episode spans the boundary: the test shows nothing"
    assert same(E[T][spans], (carry1 + reward[T])[spans]) and not same(E[T][spans], reward[T][spans])
    assert done.sum().item() >= B, "no env finished"
    case = dict(T=2 * T, B=B, N=N, D=D, reward=reward.cpu().numpy().copy(), done=done.cpu().numpy().copy(), carry=np.zeros((B, N), np.float32))
    tw = ec.twin(case)
    assert ec.same_bits(E.cpu().numpy(), tw["E"]) and ec.same_bits(er.carry.cpu().numpy(), tw["carry"])
    again = learn.EpisodeReturns(env)
    E2, stats2 = again.update(slab)
    torch.cuda.synchronize()
    assert same(E2, E) and same(again.carry, er.carry)
    assert ec.same_bits(stats2["episode_reward_sum"].cpu().numpy(), tw["S"]) and int(stats2["episodes_done"].item()) == tw["K"]
    # each rollout's own statistics: the twin on its half, with the carry it started from
    for half, c0, batch in ((slice(0, T), np.zeros((B, N), np.float32), first), (slice(T, 2 * T), carry1.cpu().numpy(), second)):
        h = dict(case, T=T, reward=case["reward"][half], done=case["done"][half], carry=c0)
        got = dict(E=batch[("next", "episode_reward")].cpu().numpy(), carry=ec.twin(h)["carry"], S=batch["episode_stats"]["episode_reward_sum"].cpu().numpy(),
                   mean=batch["episode_stats"]["episode_reward_mean"].cpu().numpy(), K=int(batch["episode_stats"]["episodes_done"].item()))
        assert all(ec.check(got, h).values())
        assert learn.EpisodeReturns.mean(batch["episode_stats"]) == round(float(ec.twin(h)["mean"]), 2)
    er.reset()
    assert not er.carry.any()
    env.close()
    actor.close()


# ---- the iteration against its parts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prb", [False, True])
@pytest.mark.parametrize("route", ["device", "torch"])
def test_train_equals_its_parts_written_out(route, prb, monkeypatch):
    """B = 8, T = 6, minibatches of 16, 2 epochs, two iterations of ``learn.train``: the same parameters, infos and statistics bit for bit as collect ->
    EpisodeReturns.update -> extend -> update -> lr written out with the stated counters; the second iteration trains at lr_at; on_iteration sees ``improved``
    exactly when the rounded mean exceeds the previous best"""
    import torch
    from sigmarl_amd import learn
    from sigmarl_amd.actor import Actor, Critic
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters

    def params():
        return Parameters(n_agents=4, num_vmas_envs=8, n_iters=4, num_epochs=2, minibatch_size=16, lr=3e-4, lr_min=1e-5, is_prb=prb, **KW)

    p, p2 = params(), params()
    assert p.frames_per_batch == 48
    B, T, mb, SEED, C0 = 8, 6, 16, 4, 100
    steps = 2 * (B * T // mb)
    assert learn.steps_per_iteration(p, p.frames_per_batch) == steps == 6
    env, env2 = SigmaEnv(p, n_envs=B, device="cuda:0"), SigmaEnv(p2, n_envs=B, device="cuda:0")
    env.reset_random(seed=3)
    env2.reset_random(seed=3)
    amod, cmod, actor, critic = _networks(env)
    amod2, cmod2, amod0 = copy.deepcopy(amod), copy.deepcopy(cmod), copy.deepcopy(amod)
    actor2, critic2 = Actor(amod2, low=LOW, high=HIGH), Critic(cmod2)

    def optimiser(e, a, am, c, cm):
        return learn.Adam(e, [(a, am), (c, cm)], lr=p.lr) if route == "device" else torch.optim.Adam(list(am.parameters()) + list(cm.parameters()), lr=p.lr)

    def lr_of(opt):
        return opt.lr if route == "device" else opt.param_groups[0]["lr"]

    opt, opt2 = optimiser(env, actor, amod, critic, cmod), optimiser(env2, actor2, amod2, critic2, cmod2)
    buf, buf2 = (learn.PrioritizedBuffer(env, B * T), learn.PrioritizedBuffer(env2, B * T)) if prb else (None, None)
    # the counters train hands to its parts
    seen = {"collect": [], "update": []}
    real_collect, real_update = learn.collect, learn.update
    monkeypatch.setattr(learn, "collect", lambda *a, **k: (seen["collect"].append((a[3], k["seed"], k["counter0"])), real_collect(*a, **k))[1])
    monkeypatch.setattr(learn, "update", lambda *a, **k: (seen["update"].append((k["seed"], k["counter0"])), real_update(*a, **k))[1])
    calls = []

    def on_iteration(i_iter, batch, infos, mean, improved):
        calls.append(dict(i_iter=i_iter, batch=batch, infos=infos, mean=mean, improved=improved, lr_next=lr_of(opt), best=p.episode_reward_intermediate,
                          current=p.episode_reward_mean_current))

    means = learn.train(env, actor, critic, amod, cmod, opt, p, n_iters=2, on_iteration=on_iteration, buffer=buf, seed=SEED, counter0=C0,
                        generator=torch.Generator(device="cuda").manual_seed(9))
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert seen["collect"] == [(T, SEED, C0), (T, SEED, C0 + T)] and seen["update"] == [(SEED, C0), (SEED, C0 + steps)]
    assert [c["i_iter"] for c in calls] == [1, 2] and means == [c["mean"] for c in calls] and len(means) == 2
    # the parts written out
    er2, gen2, best = learn.EpisodeReturns(env2), torch.Generator(device="cuda").manual_seed(9), -1e3
    for j in range(2):
        assert lr_of(opt2) == learn.lr_at(p2, j + 1)  # the rate iteration j + 1 trains at
        batch = real_collect(env2, actor2, critic2, T, params=p2, seed=SEED, counter0=C0 + j * T)
        E, stats = er2.update(batch["slab"], T)
        if prb:
            buf2.extend(batch["td_error"])
        infos = real_update(env2, actor2, critic2, amod2, cmod2, opt2, batch, params=p2, seed=SEED, counter0=C0 + j * steps, generator=gen2, buffer=buf2)
        learn.set_lr(opt2, learn.lr_at(p2, j + 2))
        torch.cuda.synchronize()
        got = calls[j]
        assert same(got["batch"]["slab"], batch["slab"]) and same(got["batch"]["advantage"], batch["advantage"]) and same(got["batch"]["td_error"], batch["td_error"])
        assert same(got["batch"][("next", "episode_reward")], E)
        assert all(same(got["batch"]["episode_stats"][k], stats[k]) for k in stats)
        assert len(got["infos"]) == len(infos) == steps
        for a, b in zip(got["infos"], infos):
            assert set(a) == set(b) and all(same(a[k], b[k]) for k in a)
        mean = learn.EpisodeReturns.mean(stats)
        assert got["mean"] == mean or (np.isnan(mean) and np.isnan(got["mean"]))
        assert got["improved"] == (mean > best)  # compared after the rounding
        best = mean if mean > best else best
        assert got["best"] == best and got["current"] == best  # (the reference's fallback: not improved -> current = the best so far)
        assert got["lr_next"] == learn.lr_at(p, j + 2) == lr_of(opt2)
    assert int(calls[0]["batch"]["episode_stats"]["episodes_done"].item()) >= 1, "no episode finished: the mean is NaN and improved shows nothing"
    assert calls[0]["improved"] is True
    assert learn.lr_at(p, 3) < learn.lr_at(p, 2) and lr_of(opt) == learn.lr_at(p, 3)
    assert all(same(a, b) for a, b in zip(list(amod.parameters()) + list(cmod.parameters()), list(amod2.parameters()) + list(cmod2.parameters())))
    assert not all(same(a, b) for a, b in zip(amod.parameters(), amod0.parameters()))  # (the parameters moved)
    if prb:
        assert same(buf.priorities(), buf2.priorities())
        buf.close()
        buf2.close()
    for e in (env, env2):
        e.close()
    for n in (actor, actor2):
        n.close()
