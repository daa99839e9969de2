#!/usr/bin/env python
"""What training prioritized action propagation adds on the device: the base-observation record of the prioritized rollout, the priority module's 1-D clip-PPO head
and the minibatch update with a priority module.  B envs x N agents, T steps (default 512 x 16, 16: one minibatch of 512 frames is a sixteenth of the batch).  A report, not a pass criterion.

  rollout      ms per T-step prioritized rollout (priority network) with and without ``base_obs=``, the two alternating after an untimed call of each, 8 calls each:
               HIP events around every call and the wall clock around call + synchronise.
  head         ``learn.priority_ppo_head`` forward + backward to both ``dout`` tensors on a minibatch of 512 frames against the same loss written out in torch on
               the device (gather by index, TanhNormal log-probability through atanh, clip objective, one-sample entropy, smooth-L1, autograd), alternating likewise.
  update       one minibatch update of 512 frames, from the records to the stepped and repacked networks, three ways -- the plain update (a plain rollout's batch),
               the prioritized base update alone (base actor and critic on the base observation, the critic's rows of width N (D + 2 K)), base + priority (the priority
               actor, its critic, the 1-D head and a second ``learn.Adam`` behind it) -- each on the device route (``apply(index=)`` -> head -> ``backward`` ->
               ``Adam.step``) against the same steps in torch on the device: gather (+ concat of the observation and the neighbour-action columns), the ``torch.nn``
               networks, the loss written out, ``clip_grad_norm_``, ``torch.optim.Adam``, ``load``.  Never the code under test on the torch side but ``load``.
Prints one JSON line; ``--out FILE`` also writes it there."""
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sigmarl_amd import learn  # noqa: E402
import copy  # noqa: E402

from sigmarl_amd.actor import Actor, Critic, PriorityNet, make_mlp, make_priority_mlp  # noqa: E402
from sigmarl_amd.env import SigmaEnv  # noqa: E402
from sigmarl_amd.params import Parameters  # noqa: E402

B, N, T, REPS, MB = (int(os.environ.get(k, d)) for k, d in (("B", 512), ("N", 16), ("T", 16), ("REPS", 8), ("MB", 512)))


def alternate(routes):
    """{name: fn} -> {name: {"event_ms": [..], "wall_ms": [..]}}: one untimed call of each, then REPS rounds of every route in turn"""
    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    res = {k: {"event_ms": [], "wall_ms": []} for k in routes}
    for _ in range(REPS):
        for k, fn in routes.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            res[k]["wall_ms"].append((time.perf_counter() - t0) * 1e3)
            res[k]["event_ms"].append(s.elapsed_time(e))
    for r in res.values():
        for k in ("event_ms", "wall_ms"):
            v = sorted(r[k])
            r[k + "_median"], r[k + "_min"], r[k + "_max"] = v[len(v) // 2], v[0], v[-1]
    return res


def torch_head(out, value, index, sc, old, adv, vt, z, clip_epsilon, entropy_coeff):
    bias, eps = math.log(math.expm1(0.99)), 1e-6
    idx = index.long()
    s, o, A, t = sc.reshape(-1, N)[idx], old.reshape(-1, N)[idx], adv.reshape(-1, N)[idx], vt.reshape(-1, N)[idx]
    loc, sig = out[..., 0], torch.clamp_min(torch.nn.functional.softplus(out[..., 1] + bias) + 0.01, 1e-4)
    x = torch.atanh(torch.clamp(s, -1 + eps, 1 - eps))
    jac = lambda u: 2.0 * (math.log(2.0) - u - torch.nn.functional.softplus(-2.0 * u))  # noqa: E731
    lw = -((x - loc) ** 2) / (2 * sig ** 2) - torch.log(sig) - 0.5 * math.log(2 * math.pi) - jac(x) - o
    g1, g2 = torch.exp(lw) * A, torch.exp(torch.clamp(lw, math.log1p(-clip_epsilon), math.log1p(clip_epsilon))) * A
    xs = loc + sig * z
    lps = -(z ** 2) / 2 - torch.log(sig) - 0.5 * math.log(2 * math.pi) - jac(xs)
    return -torch.min(g1, g2).mean() + entropy_coeff * lps.mean() + torch.nn.functional.smooth_l1_loss(value.reshape(-1, 1).expand(-1, N), t)


LOW, HIGH = [-1.0, -0.6], [1.0, 0.6]


def torch_head_2d(out, value, act, old, adv, vt, z, clip_epsilon, entropy_coeff):
    """the base loss written out: ClipPPOLoss on the TanhNormal between LOW and HIGH (rows already gathered: act [M,N,2], old / adv / vt [M,N])"""
    bias, eps = math.log(math.expm1(0.99)), 1e-6
    low, high = torch.tensor(LOW, device=out.device), torch.tensor(HIGH, device=out.device)
    h = 0.5 * (high - low)
    loc, sig = out[..., :2], torch.clamp_min(torch.nn.functional.softplus(out[..., 2:] + bias) + 0.01, 1e-4)
    x = torch.atanh(torch.clamp((act - low) / h - 1.0, -1 + eps, 1 - eps))
    jac = lambda u: 2.0 * (math.log(2.0) - u - torch.nn.functional.softplus(-2.0 * u))  # noqa: E731
    c = 0.5 * math.log(2 * math.pi)
    lw = (-((x - loc) ** 2) / (2 * sig ** 2) - torch.log(sig) - c - jac(x) - torch.log(h)).sum(-1) - old
    g1, g2 = torch.exp(lw) * adv, torch.exp(torch.clamp(lw, math.log1p(-clip_epsilon), math.log1p(clip_epsilon))) * adv
    xs = loc + sig * z
    lps = (-(z ** 2) / 2 - torch.log(sig) - c - jac(xs) - torch.log(h)).sum(-1)
    return -torch.min(g1, g2).mean() + entropy_coeff * lps.mean() + torch.nn.functional.smooth_l1_loss(value.reshape(-1, 1).expand(-1, N), vt)


def update_routes(env, batch, prioritized, with_priority):
    """(device route, torch route) of one minibatch update on ``batch``: closures over their own networks and optimisers, a new index every call"""
    D, K = env.D, env.K
    Dc = D + 2 * K if prioritized else D
    frames = T * B
    obs = batch["observation"]
    base = batch[learn.BASE_OBS] if prioritized else obs
    pad = (D, Dc) if prioritized else None
    torch.manual_seed(2)
    mods = [make_mlp(Dc).cuda(), make_mlp(N * Dc, n_out=1).cuda(), make_priority_mlp(D).cuda(), make_mlp(N * D, n_out=1).cuda()]

    def nets(ms):
        return Actor(ms[0], low=LOW, high=HIGH), Critic(ms[1]), PriorityNet(ms[2]), Critic(ms[3])

    md, mt = mods, [copy.deepcopy(m) for m in mods]
    (ad, cd, pd_, pcd), (at, ct, pt_, pct) = nets(md), nets(mt)
    opt, popt = learn.Adam(env, [(ad, md[0]), (cd, md[1])], lr=3e-4), learn.Adam(env, [(pd_, md[2]), (pcd, md[3])], lr=3e-4)
    topt = torch.optim.Adam(list(mt[0].parameters()) + list(mt[1].parameters()), lr=3e-4)
    tpopt = torch.optim.Adam(list(mt[2].parameters()) + list(mt[3].parameters()), lr=3e-4)
    ctr = [0]

    def index():
        ctr[0] += 1
        return torch.randperm(frames, device="cuda")[:MB].to(torch.int32)

    def device():
        idx = index()
        out = ad.apply(env, rows=(base, 0, N, Dc, frames, N * Dc), index=idx, check_index=False)
        value = cd.apply(env, base, index=idx, check_index=False, pad=pad)
        loss, _ = learn.ppo_head(env, out, value, batch, idx, low=LOW, high=HIGH, clip_epsilon=0.2, entropy_coeff=0.01, seed=1, counter=ctr[0])
        loss.backward()
        opt.step(1.0)
        if with_priority:
            pout = pd_.apply(env, rows=(obs, 0, N, D, frames, N * D), index=idx, check_index=False)
            pvalue = pcd.apply(env, obs, index=idx, check_index=False)
            ploss, _ = learn.priority_ppo_head(env, pout, pvalue, batch, idx, clip_epsilon=0.2, entropy_coeff=0.01, seed=1, counter=ctr[0])
            ploss.backward()
            popt.step(1.0)

    flat = lambda k: batch[k].reshape(frames, N, -1) if batch[k].dim() == 4 else batch[k].reshape(frames, N)  # noqa: E731

    def torch_route():
        idx = index().long()
        o = flat("observation")[idx]
        x = torch.cat([o, base.reshape(frames, N, Dc)[idx][..., D:]], -1) if prioritized else o  # gather + concat
        out, value = mt[0](x), mt[1](x.reshape(MB, N * Dc)).reshape(MB)
        loss = torch_head_2d(out, value, flat("action")[idx], flat("sample_log_prob")[idx], flat("advantage")[idx], flat("value_target")[idx],
                             torch.randn((MB, N, 2), device="cuda"), 0.2, 0.01)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(mt[0].parameters()) + list(mt[1].parameters()), 1.0)
        topt.step()
        topt.zero_grad()
        at.load(env, mt[0])
        ct.load(env, mt[1])
        if with_priority:
            pout, pvalue = mt[2](o), mt[3](o.reshape(MB, N * D)).reshape(MB)
            ploss = torch_head(pout, pvalue, idx, batch[learn.PRIORITY + ("scores",)], batch[learn.PRIORITY + ("sample_log_prob",)], batch["advantage"],
                               batch["value_target"], torch.randn((MB, N), device="cuda"), 0.2, 0.01)
            ploss.backward()
            torch.nn.utils.clip_grad_norm_(list(mt[2].parameters()) + list(mt[3].parameters()), 1.0)
            tpopt.step()
            tpopt.zero_grad()
            pt_.load(env, mt[2])
            pct.load(env, mt[3])

    return {"device": device, "torch": torch_route}


def updates():
    """the three update comparisons: {"plain" | "prioritized_base" | "base_plus_priority": alternate(...)}"""
    res = {}
    kw = dict(n_agents=N, scenario_type="cpm_entire", dt=0.05, is_use_mtv_distance=False, rew_method="distance", is_apply_mask=False, is_obs_noise=False, max_steps=128)
    env = SigmaEnv(Parameters(**kw), n_envs=B, device="cuda:0")
    env.reset_random(seed=1)
    torch.manual_seed(1)
    a, c = Actor(make_mlp(env.D).cuda(), low=LOW, high=HIGH), Critic(make_mlp(N * env.D, n_out=1).cuda())
    batch = learn.collect(env, a, c, T, gamma=0.99, lmbda=0.9, seed=1, counter0=0)
    res["plain"] = alternate(update_routes(env, batch, False, False))
    env.close()
    env = SigmaEnv(Parameters(is_using_prioritized_marl=True, **kw), n_envs=B, device="cuda:0")
    env.reset_random(seed=1)
    Dc = env.D + 2 * env.K
    a, c = Actor(make_mlp(Dc).cuda(), low=LOW, high=HIGH), Critic(make_mlp(N * Dc, n_out=1).cuda())
    pn, pc = PriorityNet(make_priority_mlp(env.D).cuda()), Critic(make_mlp(N * env.D, n_out=1).cuda())
    batch = learn.collect(env, a, c, T, gamma=0.99, lmbda=0.9, seed=1, counter0=0, wrapper="prioritized", priority=pn, priority_critic=pc)
    res["prioritized_base"] = alternate(update_routes(env, batch, True, False))
    res["base_plus_priority"] = alternate(update_routes(env, batch, True, True))
    env.close()
    return res


def main():
    torch.manual_seed(0)
    env = SigmaEnv(Parameters(n_agents=N, scenario_type="cpm_entire", dt=0.05, is_use_mtv_distance=False, rew_method="distance", is_apply_mask=False, is_obs_noise=False,
                              max_steps=128, is_using_prioritized_marl=True), n_envs=B, device="cuda:0")
    env.reset_random(seed=1)
    D, K = env.D, env.K
    actor = Actor(make_mlp(D + 2 * K), low=[-1.0, -0.6], high=[1.0, 0.6])
    pmlp = make_priority_mlp(D).cuda()
    pn = PriorityNet(pmlp)
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    sc, slp, obs, base = z(T, B, N), z(T, B, N), z(T, B, N, D), z(T, B, N, D + 2 * K)
    ctr = [0]

    def rollout(**kw):
        ctr[0] += T
        actor.rollout(env, T, seed=1, counter0=ctr[0], wrapper="prioritized", priority=pn, scores=sc, score_log_prob=slp, obs_rec=obs, **kw)

    out = {"n_envs": B, "n_agents": N, "steps": T, "minibatch_frames": MB, "reps": REPS, "obs_dim": D, "n_nearing": K,
           "rollout": alternate({"without_base_obs": rollout, "with_base_obs": lambda: rollout(base_obs=base)})}
    # the head on one minibatch of the records just made
    index = torch.randperm(T * B, device="cuda")[:MB].to(torch.int32)
    adv, vt = torch.randn((T, B, N), device="cuda"), torch.randn((T, B, N), device="cuda")
    batch = {("info", "priority", "scores"): sc, ("info", "priority", "sample_log_prob"): slp, "advantage": adv, "value_target": vt}
    o0 = pn.apply(env, rows=(obs, 0, N, D, T * B, N * D), index=index).detach()
    v0, zs = torch.randn(MB, device="cuda"), torch.randn((MB, N), device="cuda")

    def device_head():
        o, v = o0.clone().requires_grad_(), v0.clone().requires_grad_()
        loss, _ = learn.priority_ppo_head(env, o, v, batch, index, clip_epsilon=0.2, entropy_coeff=0.01, seed=1, counter=3)
        loss.backward()

    def torch_route():
        o, v = o0.clone().requires_grad_(), v0.clone().requires_grad_()
        torch_head(o, v, index, sc, slp, adv, vt, zs, 0.2, 0.01).backward()

    out["head"] = alternate({"device": device_head, "torch": torch_route})
    env.close()
    out["update"] = updates()
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
