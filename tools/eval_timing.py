#!/usr/bin/env python
"""What evaluating on the device costs, at 16 agents x 4096 envs on the CPM map in testing mode (``N_AGENTS`` / ``N_ENVS`` change the shape):
  fused        ``Actor.rollout`` per step with nothing attached: actor forward + the fused step / record / reset launch -- the code path of every rollout so far
  attached     the same rollout with an ``Evaluator`` attached: actor forward + step + accumulate + auto-reset, three launches where ``fused`` has one
  accumulate   ``sigmaenv_eval_accumulate`` alone, per launch
  torch        the same frame reduced with torch on the env's buffer views: the norm of (vx, vy) summed, dist_ref summed, the two ``any`` flags, added into [B]
               accumulators (fp32 sums: what the obvious host loop would write)
One process; one untimed pass of every route, then REPS (default 7) repetitions with the routes alternating; every figure is the host's wall clock around STEPS
(default 256) steps / CALLS (default 2048) launches that end in a device synchronise, divided by their number.  Best, median and spread (max - min) per route.
A report: no test asserts a time.  Writes profiles/eval_timing.txt (or the path given)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sigmarl_amd import capi  # noqa: E402
from sigmarl_amd.actor import Actor, make_mlp  # noqa: E402
from sigmarl_amd.env import SigmaEnv  # noqa: E402
from sigmarl_amd.evaluate import Evaluator  # noqa: E402
from sigmarl_amd.params import Parameters  # noqa: E402

REPS, STEPS, CALLS = int(os.environ.get("REPS", 7)), int(os.environ.get("STEPS", 256)), int(os.environ.get("CALLS", 2048))
N, B = int(os.environ.get("N_AGENTS", 16)), int(os.environ.get("N_ENVS", 4096))
LOW, HIGH = [-1.0, -0.6], [1.0, 0.6]


def wall_us(fn, n):
    """microseconds per unit of a call that enqueues n units, ended by a device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / n


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "eval_timing.txt")
    env = SigmaEnv(Parameters(n_agents=N, scenario_type="cpm_entire", dt=0.05, is_use_mtv_distance=False, rew_method="distance", is_apply_mask=False, is_obs_noise=False,
                              is_testing_mode=True, max_steps=128), n_envs=B, device="cuda:0")
    env.reset_random(seed=1)
    torch.manual_seed(0)
    actor = Actor(make_mlp(env.D), low=LOW, high=HIGH)
    ev = Evaluator(env)
    state, dist_ref, col_agents, col_flags = (env.buffer(w) for w in (capi.BUF_STATE, capi.BUF_DIST_REF, capi.BUF_COL_AGENTS, capi.BUF_COL_FLAGS))
    acc = {k: torch.zeros(B, device="cuda") for k in ("speed", "dref", "aa", "al")}
    counter = {"k": 0}

    def fused():
        actor.rollout(env, STEPS, seed=1, counter0=counter["k"], deterministic=True)
        counter["k"] += STEPS

    def attached():
        ev.reset()
        with ev.attached():
            actor.rollout(env, STEPS, seed=1, counter0=counter["k"], deterministic=True)
        counter["k"] += STEPS

    def accumulate():
        ev.reset()
        for _ in range(CALLS):
            ev.accumulate()

    def torch_frame():
        for _ in range(CALLS):
            acc["speed"] += state[..., 5:7].norm(dim=-1).sum(dim=-1)
            acc["dref"] += dist_ref.sum(dim=-1)
            acc["aa"] += col_agents.flatten(1).any(dim=-1)
            acc["al"] += col_flags[..., 0].any(dim=-1)

    routes = {"fused": (fused, STEPS, "step"), "attached": (attached, STEPS, "step"), "accumulate": (accumulate, CALLS, "launch"), "torch": (torch_frame, CALLS, "frame")}
    for fn, _, _ in routes.values():  # untimed: allocations, code loading
        fn()
    torch.cuda.synchronize()
    us = {k: [] for k in routes}
    for _ in range(REPS):
        for k, (fn, n, _) in routes.items():
            us[k].append(wall_us(fn, n))
    best = {k: min(v) for k, v in us.items()}
    lines = [f"eval_timing: {N} agents x {B} envs, cpm_entire, testing mode; {torch.cuda.get_device_name(0)}; {REPS} repetitions, routes alternating in one process",
             f"wall clock around {STEPS} rollout steps / {CALLS} launches ending in a device synchronise, microseconds per unit", ""]
    for k, (_, n, unit) in routes.items():
        v = us[k]
        lines.append(f"{k:<11} us/{unit:<7} best {min(v):9.2f}  median {statistics.median(v):9.2f}  spread {max(v) - min(v):8.2f}   all " + " ".join(f"{x:.2f}" for x in v))
    cost = best["attached"] - best["fused"]
    lines += ["", f"attachment over the fused step: {cost:+.2f} us/step ({100.0 * cost / best['fused']:+.1f} % of the fused step's {best['fused']:.2f} us; best of {REPS}); "
                  f"the fused route is measured in this run, on this build, and is the code path of a rollout without an evaluator",
              f"accumulate launch against the torch expression on the same buffers: {best['accumulate']:.2f} us vs {best['torch']:.2f} us per frame: "
              + ("the launch is %.1fx faster" % (best["torch"] / best["accumulate"]) if best["accumulate"] < best["torch"] else "the launch does NOT beat torch here")]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    for x in (ev, actor, env):
        x.close()


if __name__ == "__main__":
    main()
