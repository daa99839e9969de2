#!/usr/bin/env python
"""What a frame costs: ``Renderer.frame()`` at 16 agents x 4096 envs (cpm_entire) with 64 selected envs at 512 x 512, S = 1, 2 and 4, short-term paths on, by device
events around back-to-back launches after a warm-up of the same shape.  The launches per window are scaled from a first short window so that every timed window lasts
at least WINDOW_S (default 0.5 s); ROUNDS (default 5) windows, reported as best / median / worst.  Next to two figures from the same process:
  step        one ``sigmaenv_step_autoreset`` at 16 x 4096, timed the same way
  hbm_floor   the time the frame's bytes -- the background's resolved colours read for every tile plus the frame written, 2 x n_sel x H x W x 3 -- would take at the
              6.29 TB/s a float4 copy measures on this chip (HBM3E, 79 % of the 8 TB/s specification).  A lower bound that assumes every tile is empty; a shaded
              tile reads its coverage words instead and computes.
and the attached rollout (``Actor.rollout`` fp32, T = 128, ``attached(every=1)`` into a ring of 4 frames of the same 64 envs at S = 2) against the same rollout
detached: the wall clock around as many back-to-back rollouts as fill WINDOW_S, ending in a synchronise, the two routes alternating, ROUNDS windows each, reported as
best / median / worst ms per step.  The share of (tile, env) pairs whose list is empty is counted on the host from the env's state.
A report: no test asserts a time.  WRITES the report (replacing the file) to the path named on the command line, default profiles/render_timing.txt; its last line
is the same numbers as one JSON line, which is also printed."""
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sigmarl_amd import capi  # noqa: E402
from sigmarl_amd.actor import Actor, make_mlp  # noqa: E402
from sigmarl_amd.env import SigmaEnv  # noqa: E402
from sigmarl_amd.params import Parameters  # noqa: E402
from sigmarl_amd.render import Renderer  # noqa: E402

WINDOW_S, ROUNDS = float(os.environ.get("WINDOW_S", 0.5)), int(os.environ.get("ROUNDS", 5))
T, N, B, N_SEL, SIZE = int(os.environ.get("T", 128)), int(os.environ.get("AGENTS", 16)), int(os.environ.get("ENVS", 4096)), int(os.environ.get("SEL", 64)), int(os.environ.get("SIZE", 512))
HBM_BYTES_PER_S = 6.29e12


def event_ms(fn, reps):
    """ms per call of ``fn`` over ``reps`` enqueued calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def spread(ms):
    ms = sorted(ms)
    return {"best": round(ms[0], 5), "median": round(statistics.median(ms), 5), "worst": round(ms[-1], 5)}


def rounds(fn):
    """ROUNDS windows of at least WINDOW_S each: the launches per window come from a first short window (which is also the warm-up)"""
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    reps = max(200, int(WINDOW_S * 1e3 / event_ms(fn, 200)) + 1)
    out = spread(event_ms(fn, reps) for _ in range(ROUNDS))
    out["launches_per_window"] = reps
    return out


def empty_tile_share(env, r):
    """the share of (tile, selected env) pairs no vehicle's or path's bounding box meets, from the env's vertices and short-term points (inflated by the half-width)"""
    s, x0, y1 = r.view
    v = env.buffer(capi.BUF_VERTICES)[torch.as_tensor(r.selection.astype(np.int64), device=env.device)][:, :, :4].cpu().numpy()
    st = env.buffer(capi.BUF_SHORT_TERM)[torch.as_tensor(r.selection.astype(np.int64), device=env.device)].cpu().numpy()
    tx, ty = (r.width + capi.RND_TILE_W - 1) // capi.RND_TILE_W, (r.height + capi.RND_TILE_H - 1) // capi.RND_TILE_H
    hit = np.zeros((len(r.selection), ty, tx), bool)
    for pts, h in ((v, r.h_path), (st, r.h_path + 0.01 * s)):
        px, py = (pts[..., 0] - x0) * s, (y1 - pts[..., 1]) * s
        c0, c1 = np.floor((px.min(-1) - h) / capi.RND_TILE_W), np.floor((px.max(-1) + h) / capi.RND_TILE_W)
        r0, r1 = np.floor((py.min(-1) - h) / capi.RND_TILE_H), np.floor((py.max(-1) + h) / capi.RND_TILE_H)
        for k in range(hit.shape[0]):
            for i in range(pts.shape[1]):
                hit[k, max(int(r0[k, i]), 0): int(r1[k, i]) + 1, max(int(c0[k, i]), 0): int(c1[k, i]) + 1] = True
    return float(1.0 - hit.mean())


def main():
    env = SigmaEnv(Parameters(n_agents=N, scenario_type="cpm_entire", dt=0.05, is_use_mtv_distance=False, rew_method="distance", is_apply_mask=False, is_obs_noise=False,
                              max_steps=128), n_envs=B, device="cuda:0")
    env.reset_random(seed=3)
    torch.manual_seed(1)
    actor = Actor(make_mlp(env.D), low=[-1.0, -0.6], high=[1.0, 0.6])
    actor.rollout(env, 16, seed=5, counter0=0, precision="fp32")  # the vehicles have left their starting points
    sel = np.linspace(0, B - 1, N_SEL).astype(np.int64)
    out = {"agents": N, "envs": B, "selected": N_SEL, "size": SIZE, "window_s": WINDOW_S, "rounds": ROUNDS, "frame_ms": {}, "library": os.path.basename(env.lib.path)}
    for S in (1, 2, 4):
        r = Renderer(env, envs=sel, width=SIZE, height=SIZE, view=None, samples=S, short_term_path=True)
        frame = torch.empty(r.shape, dtype=torch.uint8, device="cuda")
        out["frame_ms"][f"S{S}"] = rounds(lambda: r.frame(frame))
        if S == 1:  # (neither depends on S)
            out["empty_tile_share"] = round(empty_tile_share(env, r), 4)
            out["frame_bytes"] = int(frame.numel())
        r.close()
    out["hbm_floor_ms"] = round(2 * out["frame_bytes"] / HBM_BYTES_PER_S * 1e3, 5)
    act = torch.zeros(B, N, 2, device="cuda")
    act[..., 0] = 0.5
    counter = [1000]

    def step():
        counter[0] += 1
        env.step_autoreset(act, seed=5, counter=counter[0])

    out["step_autoreset_ms"] = rounds(step)
    # the attached rollout against the detached one
    slab = torch.empty(T, B, N * (env.D + 1) + 1, device="cuda")
    r = Renderer(env, envs=sel, width=SIZE, height=SIZE, samples=2, ring_frames=4, short_term_path=True)
    calls = [0]

    def rollouts(k):
        """ms per step over k back-to-back rollouts between two synchronises"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            calls[0] += 1
            actor.rollout(env, T, slab=slab, seed=5, counter0=2000 + calls[0] * T, precision="fp32")
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / (k * T)

    def attached(k):
        with r.attached(1):
            return rollouts(k)

    routes = {"detached": rollouts, "attached": attached}
    per_window = {k: max(2, int(WINDOW_S * 1e3 / (fn(2) * T)) + 1) for k, fn in routes.items()}  # (the first two rollouts of each route: warm-up and calibration)
    ms = {k: [] for k in routes}
    for _ in range(ROUNDS):
        for k, fn in routes.items():
            ms[k].append(fn(per_window[k]))
    out["rollout_ms_per_step"] = {k: dict(spread(v), rollouts_per_window=per_window[k]) for k, v in ms.items()}
    out["attached_cost_ms_per_step"] = round(out["rollout_ms_per_step"]["attached"]["median"] - out["rollout_ms_per_step"]["detached"]["median"], 5)
    line = json.dumps(out)
    print(line)
    f3 = lambda d: f"{d['best']:.5f} {d['median']:.5f} {d['worst']:.5f}"  # noqa: E731
    med = {k: v["median"] for k, v in out["frame_ms"].items()}
    step_ms, floor = out["step_autoreset_ms"]["median"], out["hbm_floor_ms"]
    near = {k: ("the step" if abs(math.log(v / step_ms)) < abs(math.log(v / floor)) else "the HBM floor") for k, v in med.items()}
    report = [
        f"render_timing: tools/render_timing.py, Renderer.frame() of {N_SEL} selected envs at {SIZE} x {SIZE} with short-term paths, {N} agents x {B} envs, cpm_entire (16 rollout",
        f"steps after the reset), one MI355X, {out['library']}; device events around back-to-back launches, every window at least {WINDOW_S} s, {ROUNDS} windows:",
        f"best / median / worst in ms.  A frame is {out['frame_bytes']} bytes; {100 * out['empty_tile_share']:.1f} % of its (tile, env) pairs have an empty list.",
        "",
    ]
    for k, v in out["frame_ms"].items():
        report.append(f"   frame S = {k[1:]}            {f3(v)}   ({v['launches_per_window']} launches per window)   = {v['median'] / step_ms:.2f} steps = {v['median'] / floor:.1f} HBM floors: nearer {near[k]}")
    report += [
        f"   sigmaenv_step_autoreset  {f3(out['step_autoreset_ms'])}   ({out['step_autoreset_ms']['launches_per_window']} launches per window)",
        f"   HBM floor                {floor:.5f}   (2 x {out['frame_bytes']} bytes at 6.29 TB/s)",
        "",
        f"   rollout, T = {T}, ms per step over back-to-back rollouts between two synchronises, {ROUNDS} windows each, the routes alternating:",
        f"   detached                 {f3(out['rollout_ms_per_step']['detached'])}   ({per_window['detached']} rollouts per window)",
        f"   attached(every=1), S = 2 {f3(out['rollout_ms_per_step']['attached'])}   ({per_window['attached']} rollouts per window)",
        f"   attached cost per step (median - median): {out['attached_cost_ms_per_step']:.5f} ms",
        "",
        line,
    ]
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "render_timing.txt")
    with open(path, "w") as f:
        f.write("\n".join(report) + "\n")


if __name__ == "__main__":
    main()
