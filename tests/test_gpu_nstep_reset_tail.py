"""Resets inside a T-step launch (``sigmaenv_step_autoreset_n``) before its last step store only what no later step of the launch writes back
(path rows, the episode counter, the request words) and what the next step reads from LDS; the last step's phases write everything else.
Every case holds one T-step launch to T single ``step_autoreset`` launches bit for bit -- the record rows and every buffer -- with envs restarting
(and agents being re-placed) at steps before the last one AND at the last one, then again after a second chunk of 3 steps, then again after one more
single launch on both sides, which shows that the HBM state the T-step launch left behind is complete."""
import numpy as np
import pytest

from sigmarl_amd import capi
from sigmarl_amd.maps import load_map
from sigmarl_amd.params import Parameters, make_config
from test_gpu_parity import FLT_BUFS, INT_BUFS, _hip_env

pytestmark = pytest.mark.gpu


def _gentle(T, B, N):
    rng = np.random.default_rng(11)
    return np.stack([rng.uniform(0.0, 0.3, (T, B, N)), rng.uniform(-0.05, 0.05, (T, B, N))], axis=-1).astype(np.float32)


def _wild(T, B, N):  # the "wild" generator of test_gpu_nstep.py
    rng = np.random.default_rng(11)
    a = np.stack([rng.uniform(-0.2, 1.3, (T, B, N)), rng.uniform(-0.7, 0.7, (T, B, N))], axis=-1)
    a[2::3] = np.stack([rng.uniform(0.0, 0.3, (T, B, N)), rng.uniform(-0.05, 0.05, (T, B, N))], axis=-1)[2::3]
    return a.astype(np.float32)


def _same_buffers(one, many, tag):
    for w in INT_BUFS + FLT_BUFS:
        assert one.get(w).tobytes() == many.get(w).tobytes(), f"buffer {w} differs {tag}"


def _launch_equals_single_launches(cfg, mp, N, B, T, acts, pf, pc, prepare=None, probe=False):
    """One T-step launch against T single launches (+ second chunk, + one more single launch).  Returns the finished envs per step (the record's done
    column) and, with probe, the per-agent requests per step: the fused launch clears the request byte of every env it touches, so they are read between
    the two launches of a third env that steps and resets separately -- and that is held to the single-launch run buffer by buffer."""
    import torch
    from sigmarl_amd.shard import slab_width

    envs = [_hip_env(cfg, mp), _hip_env(cfg, mp)] + ([_hip_env(cfg, mp)] if probe else [])
    one, many = envs[0], envs[1]
    for d in envs:
        if prepare:
            prepare(d)
        d.env.buffer(capi.BUF_DONE).fill_(1)
        d.auto_reset(5, 0, pf, pc)
    W = slab_width(N, one.env.D)
    ta = torch.as_tensor(acts).cuda()
    rec_one = torch.full((T, B, W), float("nan"), device="cuda")
    rec_many = torch.full((T, B, W), float("nan"), device="cuda")
    requests = []
    for t in range(T):
        one.env.set_slab(rec_one[t])
        one.env.step_autoreset(ta[t], 5, 100 + t, pf, pc)
        if probe:
            envs[2].step(acts[t])
            requests.append(int(envs[2].get(capi.BUF_COL_FLAGS)[..., 3].astype(bool).sum()))
            envs[2].auto_reset(5, 100 + t, pf, pc)
    one.env.set_slab(None)
    many.env.step_autoreset_n(ta, rec_many, 5, 100, pf, pc)
    many.env.sync()
    finished = rec_one[..., -1].sum(dim=1).to(torch.int64).tolist()
    print(f"finished envs per step {finished}" + (f", per-agent requests per step {requests}" if probe else ""))
    assert torch.equal(rec_one.view(torch.int32), rec_many.view(torch.int32)), "record rows differ"
    _same_buffers(one, many, f"between {T} launches and the one {T}-step launch")
    if probe:
        _same_buffers(one, envs[2], "between the fused launches and the separate step / reset launches")
    # a second chunk continues exactly where the first one stopped (stride 0: the same action block every step; no record)
    for t in range(3):
        one.env.step_autoreset(ta[0], 5, 200 + t, pf, pc)
    many.env.step_autoreset_n_ptr(ta.data_ptr(), 3, 0, 0, 0, 5, 200, pf, pc)
    _same_buffers(one, many, "after the second chunk")
    # one more single launch on both sides: everything a step reads from HBM is what single launches would have left there
    for d in (one, many):
        d.env.step_autoreset(ta[1], 5, 300, pf, pc)
    _same_buffers(one, many, "after a single launch that follows the chunks")
    for d in envs:
        d.close()
    return finished, requests


def _timeout_case(scen, N, B, T, testing=False, mid=True, end=True, **kw):
    base = dict(n_agents=N, scenario_type=scen, is_use_mtv_distance=False, rew_method="distance", dt=0.05, is_testing_mode=testing, is_apply_mask=False,
                is_obs_noise=False, max_steps=5)
    base.update(kw)
    mp = load_map(scen)
    cfg = make_config(Parameters(**base), mp, B)
    finished, _ = _launch_equals_single_launches(cfg, mp, N, B, T, _gentle(T, B, N), mp.list_first[0], mp.list_count[0])
    # without envs finishing where the case says they do, it proves nothing
    if mid:
        assert sum(finished[: T - 1]) > 0, "no env finished before the last step of the launch"
    if end:
        assert finished[T - 1] > 0, "no env finished at the last step of the launch"
    return cfg


@pytest.mark.parametrize("scen,N,B,testing", [
    ("cpm_entire", 16, 64, False),       # the headline's instantiation (16 x 1)
    ("cpm_entire", 8, 24, True),         # 8 x 2 tiles, testing mode
    ("cpm_entire", 4, 64, False),        # 4 x 4 tiles: the env list of tiles of several envs
    ("cpm_entire", 5, 33, False),        # ragged tile (generic instantiation)
    ("intersection_1", 4, 40, False),    # non-loop map
    ("cpm_entire", 32, 16, False),       # 32 x 1
])
def test_whole_env_restarts_mid_launch_and_at_the_last_step(scen, N, B, testing):
    """max_steps = 5, T = 8: every env that lives that long times out at step index 3 (mid-launch) and again at step index 7 (the last step)."""
    _timeout_case(scen, N, B, 8, testing)


def test_restarts_at_mid_launch_steps_only():
    _timeout_case("cpm_entire", 16, 64, 6, end=False)


def test_timeout_at_the_last_step_only():
    _timeout_case("cpm_entire", 16, 64, 4, mid=False)


def test_per_agent_replacement_inside_the_loop():
    """Testing mode: agents that collide or leave are re-placed one by one in an env that goes on -- at steps before the last one and at the last one."""
    N, B, T = 8, 24, 12
    p = Parameters(n_agents=N, scenario_type="cpm_entire", is_use_mtv_distance=False, rew_method="distance", dt=0.1, is_testing_mode=True, is_apply_mask=False,
                   is_obs_noise=False, max_steps=64)
    mp = load_map("cpm_entire")
    _, requests = _launch_equals_single_launches(make_config(p, mp, B), mp, N, B, T, _wild(T, B, N), mp.list_first[0], mp.list_count[0], probe=True)
    assert sum(requests[: T - 1]) > 0, "no per-agent request before the last step of the launch"
    assert requests[T - 1] > 0, "no per-agent request at the last step of the launch"


def test_bird_view_with_boundary_points():
    """The boundary points of the row shift by the agent's `fresh` flag, which a mid-launch reset keeps in LDS only."""
    cfg = _timeout_case("cpm_entire", 16, 64, 8, is_ego_view=False, is_observe_distance_to_boundaries=False)
    assert cfg.obs_flags != 0


def test_sensor_noise_key_does_not_move():
    """The noise of an observation is keyed on the env's episode counter and step count: the LDS timer row, kept by a mid-launch reset."""
    cfg = _timeout_case("cpm_entire", 16, 64, 8, is_obs_noise=True, obs_noise_level=0.05, random_seed=11)
    assert cfg.obs_noise_level > 0.0


def test_mixed_scenario_lists():
    """cpm_mixed: word 1 of the path row (the env's sub-scenario) is written by resets only, and per-agent resets read it back."""
    N, B, T = 4, 64, 8
    probs = [0.5, 0.3, 0.2]
    p = Parameters(n_agents=N, scenario_type="cpm_mixed", is_use_mtv_distance=False, rew_method="distance", dt=0.05, is_apply_mask=False, is_obs_noise=False,
                   max_steps=5, cpm_scenario_probabilities=probs)
    mp = load_map("cpm_mixed")
    finished, _ = _launch_equals_single_launches(make_config(p, mp, B), mp, N, B, T, _gentle(T, B, N), 0, capi.SCENARIO_LISTS,
                                                 prepare=lambda d: d.set_scenario_lists(probs))
    assert sum(finished[: T - 1]) > 0 and finished[T - 1] > 0


def test_mtv_distance():
    """The MTVS instantiation: phase B1 reads last step's vertices (s.vold), which phase A copies from the vertices a mid-launch reset keeps in LDS."""
    _timeout_case("cpm_entire", 16, 64, 8, is_use_mtv_distance=True)


def test_full_observation():
    """The full observation (one [others] block per env, rows composed at write-out) reads dref / dleft / dright in phase D: rewritten by phase S before."""
    cfg = _timeout_case("cpm_entire", 16, 64, 8, is_ego_view=False, is_partial_observation=False)
    assert cfg.obs_flags != 0
