"""The device's observation rows against real arithmetic (tests/observation_check.py): every test reads the device's buffers back, compares the device's BUF_OBS with
the float64 row of the device's OWN input buffers within the derived rounding bound of the kernels' formulation, asserts that no element exceeds it (none is left out)
and prints the worst error / bound per column class.  The oracle is not involved: tests/test_observation_check.py holds it to the same float64 row on the host."""
import json

import numpy as np
import pytest

import observation_check as oc
from sigmarl_amd import capi
from sigmarl_amd.maps import load_map
from sigmarl_amd.params import Parameters, make_config
from test_gpu_parity import OBS_VARIANTS

pytestmark = pytest.mark.gpu
f32 = np.float32


def _hip_env(cfg, mp):
    from sigmarl_amd.env import NumpyAdapter, SigmaEnv

    return NumpyAdapter(SigmaEnv(cfg=cfg, map_table=mp, device="cuda:0"))


def _params(N, scen="cpm_entire", **kw):
    base = dict(n_agents=N, scenario_type=scen, is_use_mtv_distance=False, rew_method="distance", dt=0.05, is_apply_mask=False, is_obs_noise=False, max_steps=9)
    base.update(kw)
    return Parameters(**base)


class _Worst:
    """the worst ratio per class over the comparisons of one test"""

    def __init__(self, name):
        self.name, self.worst, self.count, self.n = name, {}, {}, 0

    def check(self, dev, cfg, mp, fresh, tag, got=None):
        bufs = oc.read_bufs(dev, fresh)
        res = oc.compare(bufs[capi.BUF_OBS] if got is None else got, cfg, mp, bufs)
        for k, v in res["worst"].items():
            self.worst[k] = max(self.worst.get(k, 0.0), v)
            self.count[k] = self.count.get(k, 0) + res["count"][k]
        self.n += 1
        assert res["ok"] and res["excluded"] == 0, f"{self.name}, {tag}: {oc.report(res)}"
        return bufs

    def done(self):
        print("OBSCHECK " + json.dumps(dict(test=self.name, comparisons=self.n, worst={k: round(v, 4) for k, v in self.worst.items() if self.count[k]}, elements=self.count)))


def _run(w, cfg, mp, steps, seed=123, reset_seed=5):
    """full reset, then ``steps`` x (step, auto_reset) with the actions of test_hip_vs_oracle_seeded, compared after every launch; returns (env, fresh flags, envs done, auto_reset launches that re-placed only some envs, per-agent reset requests of unfinished envs)"""
    B, N = cfg.n_envs, cfg.n_agents
    dev = _hip_env(cfg, mp)
    fr = oc.FreshTracker(B, N)
    dev.env.buffer(capi.BUF_DONE).fill_(1)
    pf, pc = mp.list_first[0], mp.list_count[0]
    fr.before_auto_reset(dev)
    dev.auto_reset(reset_seed, 0, pf, pc)
    w.check(dev, cfg, mp, fr.fresh, "full reset")
    rng = np.random.default_rng(seed)
    seen_done = partial = requests = 0
    for t in range(steps):
        act = np.stack([rng.uniform(-0.2, 1.3, (B, N)), rng.uniform(-0.7, 0.7, (B, N))], axis=-1).astype(f32)
        if t % 3 == 2:
            act = np.stack([rng.uniform(0.0, 0.3, (B, N)), rng.uniform(-0.05, 0.05, (B, N))], axis=-1).astype(f32)
        dev.step(act)
        fr.step()
        w.check(dev, cfg, mp, fr.fresh, f"step {t}")
        done = int(dev.get(capi.BUF_DONE).sum())
        seen_done += done
        partial += int(0 < done < B)
        requests += int((dev.get(capi.BUF_COL_FLAGS)[..., 3].astype(bool) & ~dev.get(capi.BUF_DONE).astype(bool)[:, None]).sum())
        fr.before_auto_reset(dev)
        dev.auto_reset(reset_seed, t + 1, pf, pc)
        w.check(dev, cfg, mp, fr.fresh, f"reset after step {t}")
    return dev, fr, seen_done, partial, requests


# ---- the step kernel, default row -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec0", [False, True], ids=["fixed", "generic"])
@pytest.mark.parametrize("N,B", [(16, 33), (32, 5), (5, 33), (2, 7), (1, 9), (16, 1)])
def test_step_kernel_default_row(N, B, spec0, monkeypatch):
    """obs_flags == 0 after each of 6 seeded steps and each device-side reset: the fixed-shape instantiations and the generic one (SIGMAENV_WAVE_SPEC=0), n_nearing 1 / 2 / 4
    where N allows, distance mask and mtv distance on and off"""
    if spec0:
        monkeypatch.setenv("SIGMAENV_WAVE_SPEC", "0")
    else:
        monkeypatch.delenv("SIGMAENV_WAVE_SPEC", raising=False)
    w = _Worst(f"default row N={N} B={B} {'generic' if spec0 else 'fixed'}")
    seen = set()
    for K, mask, mtv in [(1, False, False), (2, True, True), (4, True, False), (2, False, True)]:
        p = _params(N, n_nearing_agents_observed=K, is_apply_mask=mask, is_use_mtv_distance=mtv)
        mp = load_map("cpm_entire")
        cfg = make_config(p, mp, B)
        key = (cfg.n_nearing, mask, mtv)
        if key in seen:
            continue
        seen.add(key)
        assert cfg.obs_flags == 0
        dev, _, seen_done, _, _ = _run(w, cfg, mp, 6)
        assert dev.env.launch_shape() is not None
        dev.close()
    w.done()


@pytest.mark.parametrize("ns,N,B", [(2, 16, 33), (5, 5, 33)])
def test_step_kernel_default_row_other_short_term_builds(ns, N, B):
    w = _Worst(f"default row NS={ns} N={N} B={B}")
    p = _params(N, n_points_short_term=ns, is_apply_mask=True)
    mp = load_map("cpm_entire")
    cfg = make_config(p, mp, B)
    assert cfg.obs_flags == 0
    dev, *_ = _run(w, cfg, mp, 6)
    assert dev.get(capi.BUF_SHORT_TERM).shape[2] == ns
    dev.close()
    w.done()


@pytest.mark.parametrize("scen,N", [("intersection_1", 4), ("on_ramp_1", 6)])
def test_step_kernel_default_row_other_maps_and_noise(scen, N):
    """entry / exit maps, sensor noise on (the draws are recomputed on the host)"""
    w = _Worst(f"default row {scen} noise")
    p = _params(N, scen=scen, dt=0.1, is_apply_mask=True, is_obs_noise=True, obs_noise_level=0.05, random_seed=11)
    mp = load_map(scen)
    cfg = make_config(p, mp, 24)
    dev, *_ = _run(w, cfg, mp, 6)
    dev.close()
    w.done()


# ---- observe_tile_variant ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", OBS_VARIANTS)
def test_observation_variants(kw):
    """every switch combination of test_observation_variants_hip_vs_oracle at its shape (N = 8, B = 40): after the full reset (every agent fresh: the boundary points'
    reset shift), after steps (no agent fresh) and device-side resets, and the stand-alone observe()"""
    N, B = 8, 40
    p = _params(N, **kw)
    mp = load_map("cpm_entire")
    cfg = make_config(p, mp, B)
    assert cfg.obs_flags != 0
    w = _Worst(f"variant flags={cfg.obs_flags} NS={p.n_points_short_term}")
    dev, fr, _, _, _ = _run(w, cfg, mp, 4, seed=77, reset_seed=7)
    dev.env.observe()
    w.check(dev, cfg, mp, fr.fresh, "observe")
    dev.close()
    w.done()


def test_full_observation_16_agents_with_noise():
    N, B = 16, 12
    p = _params(N, is_use_mtv_distance=True, rew_method="ttc", is_apply_mask=True, is_obs_noise=True, obs_noise_level=0.05, random_seed=11, is_ego_view=False,
                is_partial_observation=False)
    mp = load_map("cpm_entire")
    cfg = make_config(p, mp, B)
    assert cfg.obs_flags & capi.OBS_FULL
    w = _Worst("full observation 16 agents, noise")
    dev, *_ = _run(w, cfg, mp, 4, seed=8, reset_seed=4)
    assert dev.D == 430
    dev.close()
    w.done()


# ---- the other producers ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(is_observe_distance_to_boundaries=False, is_obs_steering=True)], ids=["default", "variant"])
def test_partial_auto_reset_fused_launch_observe_and_slab(kw):
    """auto_reset on a batch where only some envs finished (the env_sel path), the observation part of a rollout-record row, step_autoreset, and the stand-alone
    observe() (noise off)"""
    import torch

    N, B = 8, 40
    p = _params(N, **kw)
    mp = load_map("cpm_entire")
    cfg = make_config(p, mp, B)
    w = _Worst(f"producers flags={cfg.obs_flags}")
    dev, fr, seen_done, partial, requests = _run(w, cfg, mp, 6)
    assert partial > 0  # auto_reset launches that re-placed some, not all, envs
    assert requests == 0  # no per-agent reset in this configuration: after the fused launch below an env is fresh entirely or not at all
    D = dev.D
    slab = torch.full((B, N * (D + 1) + 1), float("nan"), device="cuda")
    dev.env.set_slab(slab)
    rng = np.random.default_rng(9)
    act = np.stack([rng.uniform(-0.2, 1.3, (B, N)), rng.uniform(-0.7, 0.7, (B, N))], axis=-1).astype(f32)
    dev.step(act)
    fr.step()
    rec = slab[:, : N * D].reshape(B, N, D).cpu().numpy()
    assert np.array_equal(rec, dev.get(capi.BUF_OBS))
    w.check(dev, cfg, mp, fr.fresh, "slab row", got=rec)
    pf, pc = mp.list_first[0], mp.list_count[0]
    dev.auto_reset(5, 50, pf, pc)
    # the fused launch: the record's done flag tells which envs the launch re-placed; BUF_OBS holds the rows after the resets
    dev.step_autoreset(act, 5, 51, pf, pc)
    done = slab[:, -1].cpu().numpy() > 0
    assert 0 < done.sum() < B
    fresh = np.broadcast_to(done[:, None], (B, N)).copy()
    w.check(dev, cfg, mp, fresh, "step_autoreset")
    dev.env.set_slab(None)
    dev.env.observe()
    w.check(dev, cfg, mp, fresh, "observe")
    dev.close()
    w.done()


# ---- injected edge states -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(is_apply_mask=True), dict(is_observe_vertices=False, is_obs_steering=True), dict(is_ego_view=False, is_obs_steering=True)],
                         ids=["default", "mask", "novert-steer", "bird"])
def test_injected_edge_states(kw):
    """reset() with injected states + observe(): coincident agents, an agent at (9, -3), |psi| around 100 rad, psi_j - psi_i within 1e-6 of +-pi, zero speed, a neighbour
    exactly at distance_mask_agents (observation_check.injected_edge_states)"""
    p = _params(6, **kw)
    mp = load_map("cpm_entire")
    cfg = make_config(p, mp, len(oc.EDGE_ENVS))
    dev = _hip_env(cfg, mp)
    dev.reset(*oc.injected_edge_states(cfg, mp), 1)
    dev.observe()
    w = _Worst(f"edge states {kw}")
    bufs = w.check(dev, cfg, mp, np.ones((cfg.n_envs, 6), bool), "reset + observe")
    e = oc.EDGE_ENVS.index
    obs = bufs[capi.BUF_OBS]
    if not kw:
        assert (obs[e("zero_speed"), :, 0] == 0).all()
    if kw.get("is_apply_mask"):
        d, dm = bufs[capi.BUF_DIST_AGENTS][e("at_mask")], f32(cfg.distance_mask_agents)
        near = list(bufs[capi.BUF_NEARING][e("at_mask"), 0])
        assert d[0, 1] == dm and d[0, 2] == np.nextafter(dm, f32(0)) and set(near) == {1, 2}
        blk = obs[e("at_mask"), 0, 10:].reshape(2, 11)
        k1 = near.index(1)
        assert (blk[k1, :8] == 1).all() and blk[k1, 10] == 1 and (blk[k1, 8:10] == 0).all() and blk[1 - k1, 10] != 1   # masked exactly at the distance, not an ulp nearer
    # a step from these states (no agent fresh)
    dev.step(np.tile(f32([0.3, 0.1]), (cfg.n_envs, 6, 1)))
    w.check(dev, cfg, mp, np.zeros((cfg.n_envs, 6), bool), "step from the edge states")
    dev.close()
    w.done()
