#!/usr/bin/env python
"""Randomised differential run: HIP path vs the CPU oracle over random configurations (map, agents, envs, distance type, reward method,
testing mode, observation switches, fixed-duration resets), every buffer compared after every fused step / reset launch.
Diagnostic tool for the GPU box (uses tests/' helpers):   python tools/fuzz_parity.py [--seconds 300] [--seed 0]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import oracle_binding as ob
import test_gpu_parity as tp
from sigmarl_amd import capi
from sigmarl_amd.maps import load_map
from sigmarl_amd.params import Parameters, make_config

MAPS = ["cpm_entire", "cpm_entire", "cpm_entire", "intersection_1", "on_ramp_1", "roundabout_1", "interchange_2", "intersection_5", "on_ramp_2_multilane", "cpm_mixed"]
REW = ["distance", "ttc", "sparse", "distance_sparse", "ttc_sparse"]


LDS_LIMIT = 64 * 1024  # a drawn tiling whose workgroups would need more LDS than every device grants without the opt-in attribute is shrunk, not requested
TILING_SWITCHES = ("SIGMAENV_WPB", "SIGMAENV_WAVE_SPEC")


def _hip_env_with_tiling(cfg, mp, N, tiling_rng):
    """The HIP handle at a tiling drawn from `tiling_rng` (a generator of its own: the case's stream is untouched): cfg.envs_per_group anywhere in 1 .. 64 // N
    (divisors of the batch or not), SIGMAENV_WPB in {1, 2, 4}, and now and then SIGMAENV_WAVE_SPEC=0.  The tiling is applied, read back with launch_shape() and
    asserted; one that does not fit the LDS is shrunk (first one tile per workgroup, then half the envs per tile)."""
    epg, wpb, spec0 = int(tiling_rng.integers(1, 64 // N + 1)), int(tiling_rng.choice([1, 2, 4])), bool(tiling_rng.integers(3) == 0)
    saved = {k: os.environ.get(k) for k in TILING_SWITCHES}
    try:
        while True:
            os.environ["SIGMAENV_WPB"] = str(wpb)
            os.environ.pop("SIGMAENV_WAVE_SPEC", None)
            if spec0:
                os.environ["SIGMAENV_WAVE_SPEC"] = "0"
            cfg.envs_per_group = epg
            dev = tp._hip_env(cfg, mp)
            ls = dev.env.launch_shape()
            assert (ls["wave_G"], ls["G"], ls["wave_wpb"]) == (epg, epg, wpb), (epg, wpb, ls)
            assert ls["wave_grid"] == ((cfg.n_envs + epg - 1) // epg + wpb - 1) // wpb, ls
            if spec0:
                assert ls["wave_spec"] == 0 and ls["kern_sn"] == 0 and ls["kern_sg"] == 0, ls
            assert ls["kern_par"] == int(2 * epg * N <= 64), ls
            if max(ls["wave_lds_bytes"], ls["smem_bytes"]) <= LDS_LIMIT or (wpb == 1 and epg == 1):
                return dev, f"tiling {N} x {epg}, {wpb} per workgroup, instantiation {ls['instantiation']}"
            dev.close()
            if wpb > 1:
                wpb = 1
            else:
                epg = max(1, epg // 2)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ranges of the Parameters-exposed reward constants (tests/perturbed_constants.py: the default's sign, within about +-40 % of it; lower thresholds a
# fraction of their upper ones): drawn in a third of the cases when one_case is given a `const_rng`
CONST_RANGES = {"reward_progress": (0.06, 0.14), "penalty_near_boundary": (-0.28, -0.12), "penalty_near_other_agents": (-0.28, -0.12),
                "threshold_near_boundary_high": (0.012, 0.028), "threshold_near_other_agents_c2c_high": (0.18, 0.42), "ttc_high": (2.3, 5.2)}
CONST_LOW_OF = {"threshold_near_boundary_low": "threshold_near_boundary_high", "threshold_near_other_agents_c2c_low": "threshold_near_other_agents_c2c_high",
                "ttc_low": "ttc_high"}


def draw_constants(const_rng):
    kw = {k: float(const_rng.uniform(lo, hi)) for k, (lo, hi) in CONST_RANGES.items()}
    for low, high in CONST_LOW_OF.items():
        kw[low] = float(const_rng.uniform(0.02, 0.25)) * kw[high]
    return kw


def one_case(rng, k, tiling_rng=None, const_rng=None):
    """One random configuration.  `tiling_rng` (optional, a second generator) also draws a tiling of the step kernel; `const_rng` (optional, a third one) draws,
    in a third of the cases, the Parameters-exposed reward constants away from their defaults.  Without them the function consumes exactly the random numbers
    it always did, the library chooses the tiling and the constants are the defaults."""
    scen = MAPS[rng.integers(len(MAPS))]
    mp = load_map(scen)
    n_max = 20 if scen == "cpm_entire" else 6
    N = int(rng.integers(1, n_max + 1))
    if scen == "cpm_entire" and rng.integers(8) == 0:  # now and then a crowded map: up to 64 agents (one env per wavefront, no lane pairing)
        N = int(rng.integers(21, 65))
    B = int(rng.integers(3, 160))
    kw = dict(n_agents=N, scenario_type=scen, is_use_mtv_distance=bool(rng.integers(2)), rew_method=REW[rng.integers(len(REW))], dt=float(rng.choice([0.05, 0.1])),
              is_testing_mode=bool(rng.integers(4) == 0), is_apply_mask=bool(rng.integers(3) == 0), is_obs_noise=bool(rng.integers(4) == 0), max_steps=int(rng.integers(6, 40)),
              reset_agent_fixed_duration=float(rng.choice([0, 0, 0.5])), n_points_short_term=int(rng.choice([3, 3, 3, 2, 5])),
              is_using_opponent_modeling=bool(rng.integers(6) == 0))
    if rng.integers(3) == 0:  # observation switches
        kw.update(is_obs_steering=bool(rng.integers(2)), is_observe_ref_path_other_agents=bool(rng.integers(2)), is_observe_vertices=bool(rng.integers(2)),
                  is_observe_distance_to_agents=bool(rng.integers(2)), is_observe_distance_to_center_line=bool(rng.integers(2)),
                  is_observe_distance_to_boundaries=bool(rng.integers(2)))
        if rng.integers(3) == 0:  # bird view, with or without the (lanelet-relation) mask; a third of those with the full observation where the reference's reshape allows it
            kw.update(is_ego_view=False)
            if rng.integers(3) == 0:
                kw.update(is_partial_observation=False, n_nearing_agents_observed=int(rng.integers(1, 5)))
                try:
                    from sigmarl_amd.params import obs_flags
                    capi.obs_dim(min(kw["n_nearing_agents_observed"], N - 1), obs_flags(Parameters(**kw)), kw["n_points_short_term"], N)
                except ValueError:
                    kw.update(is_partial_observation=True, n_nearing_agents_observed=2)
    if const_rng is not None and const_rng.integers(3) == 0:
        kw.update(draw_constants(const_rng))
    p = Parameters(**kw)
    cfg = make_config(p, mp, B)
    tiling = ""
    if tiling_rng is None:
        dev = tp._hip_env(cfg, mp)
    else:
        dev, tiling = _hip_env_with_tiling(cfg, mp, N, tiling_rng)
    ora = ob.OracleEnv(cfg, mp)
    dev.env.buffer(capi.BUF_DONE).fill_(1)
    ora.get(capi.BUF_DONE, copy=False)[:] = 1
    lst = int(rng.integers(len(mp.list_first)))
    if mp.list_count[lst] < 1:
        lst = 0
    pf, pc = int(mp.list_first[lst]), int(mp.list_count[lst])
    mixed = scen == "cpm_mixed" and bool(rng.integers(2))  # the sub-scenario lists instead of one path range (sigmaenv_set_scenario_lists)
    if mixed:
        probs = [float(v) for v in rng.uniform(0.0, 1.0, 3)]
        dev.set_scenario_lists(probs)
        ora.set_scenario_lists(probs)
        pf, pc = 0, capi.SCENARIO_LISTS
    seed = int(rng.integers(1 << 30))
    dev.auto_reset(seed, 0, pf, pc)
    ora.auto_reset(seed, 0, pf, pc)
    tag = f"case {k}: {scen} N={N} B={B} " + (tiling + " " if tiling else "") + " ".join(f"{a}={b:.4g}" if isinstance(b, float) else f"{a}={b}" for a, b in kw.items() if a not in ("n_agents", "scenario_type"))
    n_diff = tp._compare_all(dev, ora, tag + " | initial reset")
    T = int(rng.integers(8, 40))
    for t in range(T):
        mode = rng.integers(4)
        lo, hi, s = [(0, 1, 0.25), (0.1, 0.4, 0.03), (-0.5, 1.6, 0.9), (0.0, 0.0, 0.0)][mode]
        act = np.stack([rng.uniform(lo, hi, (B, N)) if hi > lo else np.zeros((B, N)), rng.uniform(-s, s, (B, N)) if s > 0 else np.zeros((B, N))], axis=-1).astype(np.float32)
        if rng.integers(2):
            dev.step_autoreset(act, seed, t + 1, pf, pc)
        elif rng.integers(3) == 0:  # the in-kernel step loop with a chunk of one step (longer chunks: tests/test_gpu_nstep.py)
            import torch

            dev.env.step_autoreset_n(torch.as_tensor(act[None]).to(dev.env.device).contiguous(), seed=seed, counter0=t + 1, path_first=pf, path_count=pc)
            dev.env.sync()
        else:
            dev.step(act)
            n_diff += 0
            dev.auto_reset(seed, t + 1, pf, pc)
        ora.step(act)
        ora.auto_reset(seed, t + 1, pf, pc)
        n_diff += tp._compare_all(dev, ora, tag + f" | step {t}")
        if rng.integers(4) == 0 and not mixed:  # host-driven resets (sigmaenv_reset): single agents of some envs, or whole envs, onto random centre-line points
            full = bool(rng.integers(2))
            envs = rng.choice(B, size=int(rng.integers(1, min(B, 6) + 1)), replace=False)
            ei, ai, ids, st8 = [], [], [], []
            for e in envs:
                agents = range(N) if full else rng.choice(N, size=int(rng.integers(1, N + 1)), replace=False)
                for i in agents:
                    gp = pf + int(rng.integers(pc))
                    pt = int(rng.integers(1, max(2, int(mp.n_center[gp]) - 2)))
                    x, y = [float(v) for v in mp.center[gp, pt]]
                    yaw = float(mp.yaw[gp, min(pt, int(mp.n_yaw[gp]) - 1)])
                    sp = float(rng.uniform(0, 1))
                    ei.append(int(e)); ai.append(int(i)); ids.append((gp, lst, gp - pf, pt))
                    st8.append((x, y, yaw, sp, 0.0, sp * np.cos(np.float32(yaw)), sp * np.sin(np.float32(yaw)), 0.0))
            for env_ in (dev, ora):
                env_.reset(np.asarray(ei, np.int32), np.asarray(ai, np.int32), np.asarray(ids, np.int32), np.asarray(st8, np.float32), int(full))
                env_.observe()
            n_diff += tp._compare_all(dev, ora, tag + f" | host reset after step {t}")
    dev.close()
    ora.close()
    return tag, T * B * N, n_diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    const_rng = np.random.default_rng([args.seed, 0xC0257])  # a stream of its own: the cases of a seed are the ones they always were, a third of them at drawn constants
    t0 = time.time()
    k = n_steps = n_diff = 0
    while time.time() - t0 < args.seconds:
        tag, steps, diff = one_case(rng, k, const_rng=const_rng)
        n_steps += steps
        n_diff += diff
        if diff:
            print("differing non-observation words:", diff, tag)
        k += 1
    print(f"fuzz: {k} configurations, {n_steps} agent-steps compared, {n_diff} differing non-observation fp32 words, no mask / index mismatch, all floats within {tp.FTOL}")


if __name__ == "__main__":
    main()
