#!/usr/bin/env python
"""What one minibatch update costs from the records to the parameters' .grad -- forward, loss head, backward -- at the benchmark's networks (N agents, default 16;
actor D -> 256^3 -> 4, critic N D -> 256^3 -> 1) and the reference's minibatch_size (default 512 frames = 8192 actor rows), on a learn.collect batch of T x B frames:
  device   Actor.apply / Critic.apply(index=) read the frames where they lie, learn.ppo_head (sigmaenv_ppo_head), loss.backward() (sigmaenv_mlp32_backward_indexed)
  torch    index_select gathers of the observations and the four records, the torch.nn modules, the same loss written in torch, autograd; fp32, same device
Both routes end with the .grad of every parameter of both networks; the tail of the update is not in these figures.  HIP events around each call; one untimed call
of each route, then REPS (default 3) repetitions with the two routes alternating inside one process.
``whole_update``, measured afterwards: the device route above followed by either tail of a minibatch update (tools/optim_step_timing.py times the tails alone) --
  device   learn.Adam.step (sigmaenv_optim_step: clip, Adam, repack; no host wait, one Adam.resolve() at the end of a run)
  parent   clip_grad_norm_ + torch.optim.Adam.step + zero_grad + actor.load + critic.load
by HIP events around one update and by the host's wall clock over UPDATES (default 8) consecutive updates without a synchronisation in between; same alternation.
A report, not a bound.  Writes the JSON to the path given (default profiles/ppo_update_timing.json) and prints it."""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sigmarl_amd import learn  # noqa: E402
from sigmarl_amd.actor import Actor, Critic, make_mlp  # noqa: E402
from sigmarl_amd.env import SigmaEnv  # noqa: E402
from sigmarl_amd.params import Parameters  # noqa: E402

B, N, T, REPS = int(os.environ.get("B", 512)), int(os.environ.get("N", 16)), int(os.environ.get("T", 16)), int(os.environ.get("REPS", 3))
MB = int(os.environ.get("MINIBATCH", Parameters().minibatch_size))
UPDATES = int(os.environ.get("UPDATES", 8))
LOW, HIGH, EPS, CE = [-1.0, -0.6], [1.0, 0.6], 0.2, 1e-4
BIAS, LOG_SQRT_2PI, LOG2 = 0.5254587192925021, 0.91893853320467274, 0.69314718055994531


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def torch_loss(out, value, act, old, adv, vt, z):
    """sigmaenv_ppo_head's formulas (include/sigmaenv.h) in torch"""
    low, high = torch.tensor(LOW, device=out.device), torch.tensor(HIGH, device=out.device)
    sp = torch.nn.functional.softplus
    loc, sig = out[..., :2], torch.clamp_min(sp(out[..., 2:] + BIAS) + 0.01, 1e-4)
    h = 0.5 * (high - low)
    y = torch.clamp((act - low) / h - 1.0, -1.0 + 1e-6, 1.0 - 1e-6)
    x = 0.5 * (torch.log1p(y) - torch.log1p(-y))
    jac = lambda u: 2.0 * (LOG2 - u - sp(-2.0 * u))  # noqa: E731
    lw = (-((x - loc) ** 2) / (2 * sig ** 2) - torch.log(sig) - LOG_SQRT_2PI - jac(x) - torch.log(h)).sum(-1) - old
    g1, g2 = torch.exp(lw) * adv, torch.exp(torch.clamp(lw, math.log1p(-EPS), math.log1p(EPS))) * adv
    lps = (-(z ** 2) / 2 - torch.log(sig) - LOG_SQRT_2PI - jac(loc + sig * z) - torch.log(h)).sum(-1)
    e = value.unsqueeze(-1) - vt
    return -torch.min(g1, g2).mean() + CE * lps.mean() + torch.where(e.abs() < 1.0, 0.5 * e * e, e.abs() - 0.5).mean()


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ppo_update_timing.json")
    torch.manual_seed(0)
    env = SigmaEnv(Parameters(n_agents=N, scenario_type="cpm_entire", dt=0.05, is_use_mtv_distance=False, rew_method="distance", is_apply_mask=False,
                              is_obs_noise=False, max_steps=128), n_envs=B, device="cuda:0")
    env.reset_random(seed=1)
    D, frames = env.D, T * B
    amod, cmod = make_mlp(D).cuda(), make_mlp(N * D, n_out=1).cuda()
    actor, critic = Actor(amod, low=LOW, high=HIGH), Critic(cmod)
    batch = learn.collect(env, actor, critic, T, gamma=0.99, lmbda=0.9, seed=1, counter0=0)
    env.sync()
    obs = batch["observation"]
    index = learn.minibatches(frames, MB, torch.Generator(device="cuda").manual_seed(1))[0]
    M = index.numel()
    pars = list(amod.parameters()) + list(cmod.parameters())

    def zero():
        for p in pars:
            p.grad = None

    def device():
        zero()
        out = actor.apply(env, rows=(obs, 0, N, D, frames, N * D), index=index, check_index=False)
        value = critic.apply(env, obs, index=index, check_index=False)
        loss, _ = learn.ppo_head(env, out, value, batch, index, low=LOW, high=HIGH, clip_epsilon=EPS, entropy_coeff=CE, seed=1, counter=0)
        loss.backward()

    flat = {k: batch[k].reshape(frames, *batch[k].shape[2:]) for k in ("observation", "action", "sample_log_prob", "advantage", "value_target")}

    def torch_route():
        zero()
        idx = index.long()
        x, act, old, adv, vt = (flat[k].index_select(0, idx) for k in ("observation", "action", "sample_log_prob", "advantage", "value_target"))
        out = amod(x.reshape(M * N, D)).view(M, N, 4)
        value = cmod(x.reshape(M, N * D)).view(M)
        torch_loss(out, value, act, old, adv, vt, torch.randn((M, N, 2), device=x.device)).backward()

    routes = {"device": device, "torch": torch_route}
    for fn in routes.values():  # one untimed call each: allocations, kernel loads
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(REPS):
        for k, fn in routes.items():
            ms[k].append(timed(fn))
    res = {"n_agents": N, "n_envs": B, "steps": T, "frames": frames, "minibatch_frames": M, "actor_rows": M * N, "critic_rows": M, "obs_dim": D, "reps": REPS,
           "ms": ms, "best_ms": {k: min(v) for k, v in ms.items()}}
    # a whole minibatch update: the device route to the gradients, then either tail
    dev_opt, par_opt = learn.Adam(env, [(actor, amod), (critic, cmod)], lr=3e-4), torch.optim.Adam(pars, lr=3e-4)

    def whole_device():
        device()
        dev_opt.step(1.0)

    def whole_parent():
        device()
        torch.nn.utils.clip_grad_norm_(pars, 1.0)
        par_opt.step()
        par_opt.zero_grad()
        actor.load(env, amod)
        critic.load(env, cmod)

    whole = {"device": (whole_device, dev_opt.resolve), "parent": (whole_parent, lambda: None)}

    def wall(fn, finish):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(UPDATES):
            fn()
        finish()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / UPDATES

    for fn, finish in whole.values():
        fn()
        finish()
    torch.cuda.synchronize()
    ev, wl = {k: [] for k in whole}, {k: [] for k in whole}
    for _ in range(REPS):
        for k, (fn, finish) in whole.items():
            ev[k].append(timed(fn))
            finish()
        for k, (fn, finish) in whole.items():
            wl[k].append(wall(fn, finish))
    res["whole_update"] = {"updates_per_wall_run": UPDATES, "event_ms": ev, "wall_ms_per_update": wl,
                           "best": {"event_ms": {k: min(v) for k, v in ev.items()}, "wall_ms_per_update": {k: min(v) for k, v in wl.items()}}}
    actor.close()
    critic.close()
    env.close()
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
