#!/usr/bin/env python
"""What the challenging initial-state buffer costs a rollout: the fp32 closed-loop rollout (``Actor.rollout``: policy -> step + record + resets, T = 128 steps) at
16 agents x 4096 envs,
  unattached   the fused launch per step, as every caller without a bank runs it (the figure that must not move against the parent commit's library)
  attached     inside ``InitialStateBank(env).attached()`` at the reference's defaults (capacity 100, probability_record 1.0, probability_use_recording 0.2,
               n_steps_stored 10): step -> record (2 launches) -> restart (3) -> auto_reset -> settle per step
by the wall clock around a rollout that ends in a synchronise, REPS (default 5) repetitions after one untimed rollout of each, the two alternating inside one
process.  ``ms_per_step`` = rollout time / T.  A library without the entry points (an older build through SIGMAENV_LIB, tools/ab_libs.sh's switches) gives the
unattached figure alone: that is how the parent commit's library is measured with the same script; ATTACHED=0 measures this library the same way (no attached
rollout between the unattached ones: like for like).  A report; no test asserts a time.  Prints one JSON line and
appends it to the file named on the command line, if any."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sigmarl_amd.actor import Actor, make_mlp  # noqa: E402
from sigmarl_amd.env import SigmaEnv  # noqa: E402
from sigmarl_amd.params import Parameters  # noqa: E402

REPS, T, N, B = int(os.environ.get("REPS", 5)), int(os.environ.get("T", 128)), int(os.environ.get("AGENTS", 16)), int(os.environ.get("ENVS", 4096))


def main():
    env = SigmaEnv(Parameters(n_agents=N, scenario_type="cpm_entire", dt=0.05, is_use_mtv_distance=False, rew_method="distance", is_apply_mask=False, is_obs_noise=False,
                              max_steps=128), n_envs=B, device="cuda:0")
    env.reset_random(seed=3)
    torch.manual_seed(1)
    actor = Actor(make_mlp(env.D), low=[-1.0, -0.6], high=[1.0, 0.6])
    slab = torch.empty(T, B, N * (env.D + 1) + 1, device="cuda")
    bank = None
    if hasattr(env.lib, "isb_create") and os.environ.get("ATTACHED", "1") != "0":
        from sigmarl_amd.initial_states import InitialStateBank

        bank = InitialStateBank(env)
    calls = [0]

    def rollout():
        calls[0] += 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        actor.rollout(env, T, slab=slab, seed=5, counter0=calls[0] * T, precision="fp32")
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / T

    def attached():
        with bank.attached():
            return rollout()

    routes = {"unattached": rollout}
    if bank is not None:
        routes["attached"] = attached
    for fn in routes.values():
        fn()
    ms = {k: [] for k in routes}
    for _ in range(REPS):
        for k, fn in routes.items():
            ms[k].append(fn())
    out = {"library": os.path.basename(env.lib.path), "agents": N, "envs": B, "T": T, "reps": REPS,
           "ms_per_step": {k: [round(x, 5) for x in v] for k, v in ms.items()}, "best_ms_per_step": {k: round(min(v), 5) for k, v in ms.items()}}
    if bank is not None:
        out["bank_count"] = bank.count
        out["attached_cost_ms_per_step"] = round(min(ms["attached"]) - min(ms["unattached"]), 5)
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
