"""The candidate chunks from the per-level neighbour lists (NeighRow; neigh_list_select / neigh_candidates in sigmaenv.hip), on the GPU against the C oracle
(run with -m gpu on an MI355X).  The lists only say WHICH chunk boxes are tested, so every output must stay what it was: bit for bit.

Maps: `dense` (every level of every chunk overflows its list: the group-box search stands in), `hairpin` (two runs of neighbours; levels at the capacity and above it,
so one task's tight level is answered by its near or far list), `long257` (chunk 63) and cpm_entire (the headline's map).  That the tables of these maps have such rows
is asserted in tests/test_neigh_list_host.py.  Shapes: 16 agents x 2 envs (the fixed 16 x 1 instantiation), 4 x 6 (fixed 4 x 4, ragged second tile), 3 x 7 (generic,
five envs per wavefront, ragged) and a single agent.  Sequence:

  reset with the given states + observe                       the block kernels' mask_stage3 at the tight level,
  every agent's state overwritten with its far-teleport row   (closest indices stale by up to 250 segments, the first agents' corner queries metres behind),
  one step_autoreset_n launch of eight steps                  its first step selects the far level or the group-box search, the later ones the tight and near
                                                              levels; max_steps lets envs finish and restart from the start table inside the launch,
  closest indices beyond every polyline's end, two more steps the reload of mask_stage2,

each compared as tests/test_gpu_scan_synthetic.py compares: masks, indices, done and timers bit for bit, and the distance, short-term-path and reward buffers bit for
bit as well."""
import numpy as np
import pytest

import oracle_binding as ob
import synthetic_maps as sm
import test_gpu_scan_synthetic as ts
import test_scan_bound_host as hb
from sigmarl_amd import capi
from sigmarl_amd.params import Parameters, make_config

MAPS = ("dense", "hairpin", "long257", "cpm_entire")
# N -> (envs, cfg.envs_per_group, the step kernel's instantiation <FASTDIV, PAR, SN, SG, VAR, MTVS>)
SHAPES = {16: (2, 1, (True, True, 16, 1, False, False)), 4: (6, 4, (True, True, 4, 4, False, False)), 3: (7, 5, (True, True, 0, 0, False, False)),
          1: (24, 1, (True, True, 0, 0, False, False))}
MAX_STEPS = 5  # every env runs out of steps inside the launch of eight


def _placement(mp, N, rows):
    B = SHAPES[N][0]
    rows = rows[:B * N]
    ids = np.zeros((B * N, 4), np.int32)
    ids[:, 0] = mp.list_first[0] + rows[:, 0].astype(np.int32)
    ids[:, 2] = rows[:, 0].astype(np.int32)
    ids[:, 3] = rows[:, 1].astype(np.int32)
    return np.repeat(np.arange(B), N).astype(np.int32), np.tile(np.arange(N), B).astype(np.int32), ids, sm.state8(rows)


def _launch(dev, ora, acts, counter0, pf, pc):
    import torch

    dev.env.step_autoreset_n(torch.as_tensor(acts).to(dev.env.device).contiguous(), None, seed=5, counter0=counter0, path_first=pf, path_count=pc)
    dev.env.sync()
    done = 0
    for k in range(len(acts)):
        ora.step(acts[k])
        done += int(ora.get(capi.BUF_DONE).sum())
        ora.auto_reset(5, counter0 + k, pf, pc)
    return done


@pytest.mark.gpu
@pytest.mark.parametrize("N", sorted(SHAPES))
@pytest.mark.parametrize("name", MAPS)
def test_list_walk_equals_the_oracle(name, N, monkeypatch):
    import torch

    B, G, inst = SHAPES[N]
    mp = hb.map_table(name)
    p = Parameters(n_agents=N, scenario_type=name, is_use_mtv_distance=False, rew_method="distance", dt=0.05, is_apply_mask=False, is_obs_noise=False,
                   max_steps=MAX_STEPS)
    cfg = make_config(p, mp, B)
    cfg.envs_per_group = G
    dev, ora = ts._handle(monkeypatch, cfg, mp), ob.OracleEnv(cfg, mp)
    try:
        ls = dev.env.launch_shape()
        assert ls["pruned_scan"] == 1 and ls["map_fast_div"] == 1 and (ls["wave_G"], ls["wave_wpb"]) == (G, 1) and ls["instantiation"] == inst, ls
        pf, pc = mp.list_first[0], mp.list_count[0]
        rows, tele = hb.state_rows(name)
        rows, tele = rows[:B * N], tele[:B * N]
        rng = np.random.default_rng(31 * MAPS.index(name) + N)
        envs = [dev, ora]

        def actions(T):
            return np.stack([np.stack([rng.uniform(-0.2, 1.0, (B, N)), rng.uniform(-0.5, 0.5, (B, N))], axis=-1) for _ in range(T)]).astype(np.float32)

        for e in envs:
            e.reset(*_placement(mp, N, rows), 1)
            e.observe()
        ts._check(envs, f"{name} N={N}: reset + observe")
        # the far teleport: the states move, the closest indices and the vertices (the first agents' corner queries) stay behind
        st8 = sm.state8(tele).reshape(B, N, 8)
        dev.env.buffer(capi.BUF_STATE).view(B, N, 8)[:] = torch.as_tensor(st8).to(dev.env.device)
        dev.env.sync()
        ora.get(capi.BUF_STATE, copy=False).reshape(B, N, 8)[:] = st8
        done = _launch(dev, ora, actions(8), 1, pf, pc)
        ts._check(envs, f"{name} N={N}: step_autoreset_n of 8 steps from the teleported states")
        assert done >= B, done  # (every env finished inside the launch)
        # a caller's closest indices beyond the end of every polyline: mask_stage2 reloads the last segment and its row
        beyond = mp.center.shape[1] + 2
        dev.env.buffer(capi.BUF_CLOSEST).view(B, N, 3)[:, ::2, :] = beyond
        dev.env.sync()
        ora.get(capi.BUF_CLOSEST, copy=False).reshape(B, N, 3)[:, ::2, :] = beyond
        _launch(dev, ora, actions(2), 9, pf, pc)
        ts._check(envs, f"{name} N={N}: two steps from closest indices beyond the polylines' ends")
    finally:
        dev.close()
        ora.close()


@pytest.mark.parametrize("N", sorted(SHAPES))
@pytest.mark.parametrize("name", MAPS)
def test_teleported_tasks_leave_the_tight_level(name, N):
    """No GPU: with mask_stage2's threshold restated (tests/test_scan_bound_host.py), the teleported tasks of every case ask for more than the far radius (the
    group-box search) or for the far level, and the placed ones for the tight or near level -- the launch's first step and the reset walk different lists."""
    B = SHAPES[N][0]
    radii = [float(np.float32(k) * np.float32(sm.RECT_RADIUS)) for k in (3.6, 6.0, 9.0)]
    reach = {"placed": [], "teleported": []}
    for r in hb.evaluated(name):
        t = r["task"]
        if t["kind"] in reach and t["row"] < B * N:
            _, T, dg = hb.thresholds(t)
            reach[t["kind"]].append(float(T) + float(dg))
    assert min(reach["placed"]) <= radii[1] and max(reach["teleported"]) > radii[1], (name, N, min(reach["placed"]), max(reach["teleported"]))
