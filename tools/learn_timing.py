#!/usr/bin/env python
"""What the learner-ready rollout costs (sigmarl_amd/learn.py), at N agents x B envs, T steps (default 16 x 4096, 32), fp32 split critic, one MI355X:
  critic   the critic over a rollout's record (both GAE passes, 2 x T B rows) through sigmaenv_mlp32_forward_rows, against the route without it: torch slice +
           .contiguous() of the observation part + Critic.forward on the same rows
  rollout  the fp32 device rollout with and without the root-observation record (one B N D copy per step)
  gae      the sigmaenv_gae launch (advantage + value target), with the TD priorities, and its bytes moved / time against the HBM figures
  episode  EpisodeReturns.update (sigmaenv_episode_return: the RewardSum record and its done-frame mean) on the same records, with and without the record, next
           to gae; and the host restatement it replaces: the rewards and done flags copied to the CPU and the loop over t there (a host clock: the copy waits)
  collect  learn.collect per step, beside the plain rollout per step (tools/wrapper_timing.py's figure on the same box)
HIP events around each call, after CONDITION_MS (default 200) of the same work so that the device is at its sustained clocks; REPS (default 3)
repetitions with the compared routes alternating inside one process.  A report, not a pass criterion.  Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sigmarl_amd import learn  # noqa: E402
from sigmarl_amd.actor import Actor, Critic, make_mlp  # noqa: E402
from sigmarl_amd.env import SigmaEnv  # noqa: E402
from sigmarl_amd.params import Parameters  # noqa: E402

B, N, T, REPS = int(os.environ.get("B", 4096)), int(os.environ.get("N", 16)), int(os.environ.get("T", 32)), int(os.environ.get("REPS", 3))
CONDITION_MS = float(os.environ.get("CONDITION_MS", 200))
HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12  # bytes / s: the specification, and what a device copy achieves


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def condition(fn):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < CONDITION_MS:
        fn()
        torch.cuda.synchronize()


def compare(routes: dict) -> dict:
    """ms of every route, REPS times, the routes alternating; conditioned on the first."""
    for fn in routes.values():  # (first calls: allocations, kernel loads)
        fn()
    torch.cuda.synchronize()
    condition(next(iter(routes.values())))
    out = {k: [] for k in routes}
    for _ in range(REPS):
        for k, fn in routes.items():
            out[k].append(timed(fn))
    return out


torch.manual_seed(0)
env = SigmaEnv(Parameters(n_agents=N, scenario_type="cpm_entire", dt=0.05, is_use_mtv_distance=False, rew_method="distance", is_apply_mask=False, is_obs_noise=False,
                          max_steps=128), n_envs=B, device="cuda:0")
env.reset_random(seed=1)
D, W = env.D, N * (env.D + 1) + 1
actor = Actor(make_mlp(D), low=[-1.0, -0.6], high=[1.0, 0.6])
critic = Critic(make_mlp(N * D, n_out=1))
kw = dict(dtype=torch.float32, device="cuda")
slab, rec = torch.empty((T, B, W), **kw), torch.empty((T, B, N, D), **kw)
res = {"n_agents": N, "n_envs": B, "steps": T, "reps": REPS, "condition_ms": CONDITION_MS, "critic_mode": critic.mode, "ms": {}}
ctr = [0]


def rollout(**rk):
    actor.rollout(env, T, slab=slab, seed=1, counter0=ctr[0], **rk)
    ctr[0] += T


res["ms"]["rollout"] = compare({"without_obs_rec": lambda: rollout(), "with_obs_rec": lambda: rollout(obs_rec=rec)})
res["obs_rec_copy_bytes_per_step"] = 2 * B * N * D * 4  # read + write

sv, nv = torch.empty((T, B), **kw), torch.empty((T, B), **kw)


def critic_rows():
    critic.rollout_values(env, slab, rec, T, state_value=sv, next_state_value=nv)


def critic_staged():  # the route without forward_rows: a dense copy of the observation part in front of every pass
    critic.forward(env, rec.view(T * B, N * D), out=sv.view(T * B, 1))  # (the env's stream is torch's current stream: the copy below is ordered with the kernels)
    x = slab[:, :, : N * D].contiguous()
    critic.forward(env, x.view(T * B, N * D), out=nv.view(T * B, 1))


res["ms"]["critic"] = compare({"forward_rows": critic_rows, "slice_contiguous_forward": critic_staged})
adv, vt, td = torch.empty((T, B, N), **kw), torch.empty((T, B, N), **kw), torch.empty((T, B), **kw)
p = env.parameters
res["ms"]["gae"] = compare({"gae": lambda: learn.gae(env, slab, sv, nv, p.gamma, p.lmbda, advantage=adv, value_target=vt),
                            "gae_and_td_priorities": lambda: learn.gae(env, slab, sv, nv, p.gamma, p.lmbda, advantage=adv, value_target=vt, td_error=td)})
gae_bytes = T * B * (N + 1 + 2) * 4 + 2 * T * B * N * 4  # rewards + done + two values read (the rows' cache lines hold more), advantage + value target written
g = min(res["ms"]["gae"]["gae"]) * 1e-3
res["gae_bytes"] = gae_bytes
res["gae_bytes_per_s"] = gae_bytes / g
res["gae_fraction_of_hbm_spec"] = gae_bytes / g / HBM_SPEC
res["gae_fraction_of_hbm_copy"] = gae_bytes / g / HBM_COPY

# the episode return on the same records, next to gae (alternating with it), and the host restatement it replaces
returns = learn.EpisodeReturns(env)
er = torch.empty((T, B, N), **kw)
res["ms"]["episode"] = compare({"gae": lambda: learn.gae(env, slab, sv, nv, p.gamma, p.lmbda, advantage=adv, value_target=vt),
                                "episode_return": lambda: returns.update(slab, T, episode_reward=er),
                                "episode_return_no_record": lambda: returns.update(slab, T, episode_reward=False)})
episode_bytes = T * B * (N + 1) * 4 + T * B * N * 4 + 2 * B * N * 4  # rewards + done read (the rows' cache lines hold more), the record written, the carry both ways
e = min(res["ms"]["episode"]["episode_return"]) * 1e-3
res["episode_bytes"] = episode_bytes
res["episode_bytes_per_s"] = episode_bytes / e
res["episode_fraction_of_hbm_copy"] = episode_bytes / e / HBM_COPY
res["episodes_done_in_the_records"] = float(returns.update(slab, T, episode_reward=False)[1]["episodes_done"])


def host_restatement():
    """what a user did without the entry point: [T, B, N] rewards and [T, B] done flags to the CPU, the RewardSum loop over t and the done-frame mean there"""
    t0 = time.perf_counter()
    r, d = slab[:, :, N * D: N * D + N].cpu(), slab[:, :, N * D + N].cpu() != 0
    c, E = torch.zeros((B, N)), torch.empty((T, B, N))
    for t in range(T):
        E[t] = c + r[t]
        c = torch.where(d[t][:, None], torch.zeros(()), E[t])
    mean = float(E[d].mean()) if d.any() else float("nan")
    return (time.perf_counter() - t0) * 1e3, mean


host_restatement()
host = [host_restatement() for _ in range(REPS)]
res["ms"]["episode"]["host_restatement_wall"] = [h[0] for h in host]
returns.reset()  # (the host restatement starts from a zero carry)
res["episode_mean"] = {"device": float(returns.update(slab, T, episode_reward=False)[1]["episode_reward_mean"]), "host_restatement": host[0][1]}


def collect():
    learn.collect(env, actor, critic, T, seed=1, counter0=ctr[0])
    ctr[0] += T


res["ms"]["collect"] = compare({"plain_rollout": lambda: rollout(), "collect": collect})
res["ms_per_step"] = {k: min(v) / T for k, v in {**res["ms"]["rollout"], **res["ms"]["collect"]}.items()}
env.close()
print(json.dumps(res))
