#!/usr/bin/env python
"""What evaluating on the device costs, at 16 agents x 4096 envs on the CPM map in testing mode (``N_AGENTS`` / ``N_ENVS`` change the shape):
  fused        ``Actor.rollout`` per step with nothing attached: actor forward + the fused step / record / reset launch -- the code path of every rollout so far
  attached     the same rollout with an ``Evaluator`` attached: actor forward + step + accumulate + auto-reset, three launches where ``fused`` has one
  accumulate   ``sigmaenv_eval_accumulate`` alone, per launch
  torch        the same frame reduced with torch on the env's buffer views: the norm of (vx, vy) summed, dist_ref summed, the two ``any`` flags, added into [B]
               accumulators (fp32 sums: what the obvious host loop would write)
  attached_study    ``attached`` with a study evaluator (``Evaluator(env, study=True)``): the same three launches, the accumulate one being the study instantiation
  accumulate_study  ``sigmaenv_eval_accumulate_study`` alone, per launch
  torch_study       what the study launch replaces: per frame, the copies of the applied and nominal action and the three event-reward rows into stacked tensors
                    ``[STEPS, ..]``, and -- once per STEPS frames, its cost spread over them -- the reference's ``compute_total_reward`` and
                    ``compute_cbf_activation_percentage`` (evaluation_itsc26.py:926-1035) in fp32 torch on the stacked tensors, reduced per env
``ROUTES`` (comma-separated) picks routes; the study routes are left out on a build of the library from before them (an A/B baseline through ``SIGMAENV_LIB``).
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
    has_study = hasattr(env.lib, "eval_accumulate_study")
    sev = Evaluator(env, study=True) if has_study else None
    applied, nominal, rinfo = (env.buffer(w) for w in (capi.BUF_ACTION, capi.BUF_CBF_NOMINAL, capi.BUF_REWARD_INFO))
    stack = {k: torch.zeros((STEPS, B, N) + tail, device="cuda") for k, tail in (("applied", (2,)), ("nominal", (2,)), ("event", (3,)))}
    study_out = {}
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

    def attached_study():
        sev.reset()
        with sev.attached():
            actor.rollout(env, STEPS, seed=1, counter0=counter["k"], deterministic=True)
        counter["k"] += STEPS

    def accumulate_study():
        sev.reset()
        for _ in range(CALLS):
            sev.accumulate()

    def torch_study():
        rows = list(capi.EVL_REW_ROWS)
        for t in range(STEPS):
            stack["applied"][t].copy_(applied)
            stack["nominal"][t].copy_(nominal)
            stack["event"][t].copy_(rinfo[rows].permute(1, 2, 0))
        v, nv = stack["applied"][..., 0], stack["nominal"][..., 0]  # [T, B, N]
        d, nd = stack["applied"][..., 1], stack["nominal"][..., 1]
        event = stack["event"].sum(dim=-1).sum(dim=(0, 2))
        zero = torch.zeros_like(v[:1])
        a = torch.cat([zero, (v[1:] - v[:-1]) / 0.1], dim=0)
        jerk = torch.cat([zero, (a[1:] - a[:-1]) / 0.1], dim=0)
        comfort = -0.2 * (a.abs() / 3.0).pow(2).mean(dim=(0, 2)) + -0.2 * (jerk.abs() / 20.0).pow(2).mean(dim=(0, 2))
        d_vel, d_steer = v - nv, d - nd
        degree = 0.5 * (d_vel.abs().mean(dim=(0, 2)) / (v.abs().mean(dim=(0, 2)) + 1e-9) + d_steer.abs().mean(dim=(0, 2)) / (d.abs().mean(dim=(0, 2)) + 1e-9))
        rate = ((d_vel.abs() > 1e-9) | (d_steer.abs() > 1e-9)).float().mean(dim=(0, 2))
        study_out["torch"] = (event + comfort, 100 * degree, 100 * rate)

    routes = {"fused": (fused, STEPS, "step"), "attached": (attached, STEPS, "step"), "accumulate": (accumulate, CALLS, "launch"), "torch": (torch_frame, CALLS, "frame")}
    if has_study:
        routes.update({"attached_study": (attached_study, STEPS, "step"), "accumulate_study": (accumulate_study, CALLS, "launch"), "torch_study": (torch_study, STEPS, "frame")})
    if os.environ.get("ROUTES"):
        routes = {k: routes[k] for k in os.environ["ROUTES"].split(",") if k in routes}
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
        lines.append(f"{k:<16} us/{unit:<7} best {min(v):9.2f}  median {statistics.median(v):9.2f}  spread {max(v) - min(v):8.2f}   all " + " ".join(f"{x:.2f}" for x in v))
    if {"attached_study", "attached", "accumulate_study", "accumulate", "torch_study"} <= set(best):
        lines += ["", f"study instantiation over the plain one: {best['accumulate_study'] - best['accumulate']:+.2f} us per launch ({best['accumulate_study']:.2f} vs {best['accumulate']:.2f}), "
                      f"{best['attached_study'] - best['attached']:+.2f} us per attached step ({best['attached_study']:.2f} vs {best['attached']:.2f}); best of {REPS}",
                  f"study launch against what it replaces (per-step copies + the reference's two functions in torch on the stacked tensors): {best['accumulate_study']:.2f} us vs "
                  f"{best['torch_study']:.2f} us per frame"]
    if {"attached", "fused", "accumulate", "torch"} <= set(best):
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
    for x in (sev, ev, actor, env):
        if x is not None:
            x.close()


if __name__ == "__main__":
    main()
