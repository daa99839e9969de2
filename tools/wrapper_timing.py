#!/usr/bin/env python
"""ms per step of the fp32 device rollout with each policy wrapper of the collector (sigmaenv_rollout_f32_ex): plain, opponent modelling, prioritized action
propagation (priority network, random ranks, random ranks with communication noise next to their noise-free line), in chunks of T steps at N agents x B envs (default 32 x (16 x 4096)).  A report, not a pass criterion.
Prints one JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sigmarl_amd.actor import Actor, PriorityNet, make_mlp, make_priority_mlp  # noqa: E402
from sigmarl_amd.env import SigmaEnv  # noqa: E402
from sigmarl_amd.params import Parameters  # noqa: E402

B, N, T, REPS = int(os.environ.get("B", 4096)), int(os.environ.get("N", 16)), int(os.environ.get("T", 32)), int(os.environ.get("REPS", 5))


def make(**kw):
    env = SigmaEnv(Parameters(n_agents=N, scenario_type="cpm_entire", dt=0.05, is_use_mtv_distance=False, rew_method="distance", is_apply_mask=False,
                              is_obs_noise=False, max_steps=128, **kw), n_envs=B, device="cuda:0")
    env.reset_random(seed=1)
    return env


def time_rollout(actor, env, **kw):
    actor.rollout(env, T, seed=1, counter0=0, **kw)  # warm-up (workspace, kernel loads)
    env.sync()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for r in range(REPS):
        actor.rollout(env, T, seed=1, counter0=(r + 1) * T, **kw)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / (REPS * T)


torch.manual_seed(0)
out = {"n_agents": N, "n_envs": B, "chunk_steps": T, "reps": REPS, "ms_per_step": {}}
env = make()
actor = Actor(make_mlp(env.D), low=[-1.0, -0.6], high=[1.0, 0.6])
out["ms_per_step"]["plain"] = time_rollout(actor, env)
env.close()
env = make(is_using_opponent_modeling=True)
actor = Actor(make_mlp(env.D), low=[-1.0, -0.6], high=[1.0, 0.6])
out["ms_per_step"]["opponent"] = time_rollout(actor, env, wrapper="opponent")
env.close()
env = make(is_using_prioritized_marl=True)
actor = Actor(make_mlp(env.D + 2 * env.K), low=[-1.0, -0.6], high=[1.0, 0.6])
pn = PriorityNet(make_priority_mlp(env.D))
out["ms_per_step"]["prioritized_net"] = time_rollout(actor, env, wrapper="prioritized", priority=pn)
out["ms_per_step"]["prioritized_random"] = time_rollout(actor, env, wrapper="prioritized", priority="random")
if hasattr(env.lib, "comm_noise_stds"):  # (an older build of the library as the A/B baseline has no noise)
    out["ms_per_step"]["prioritized_random_noise"] = time_rollout(actor, env, wrapper="prioritized", priority="random", communication_noise=0.1)
    out["ms_per_step"]["prioritized_random_again"] = time_rollout(actor, env, wrapper="prioritized", priority="random")  # the noise-free line once more: the run's own spread
env.close()
print(json.dumps(out))
