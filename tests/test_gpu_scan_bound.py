"""The pruned scan's threshold on the device (run with -m gpu on an MI355X): the states of tests/test_scan_bound_host.py that exercise the rule -- where it drops a
chunk the rule before it kept, where only a corner's own term keeps the chunk of that corner's winner, where one wrong term would lose a winner -- placed on the
hairpin, the dense-boundary map and cpm_entire, at the tile shapes 16 x 1, 4 x 4, the generic 3 x 5 (ragged last tile) and a single agent, at most 64 envs.

Each case: reset + observe, two steps, the first agent of every env moved to its teleport row by writing its state (its corner queries stay at the vertices it had:
metres stale) and a step, the far-teleport reset of every agent (closest indices stale by more than 100) + observe and a step, then ONE step_autoreset_n launch of
eight steps with record rows in which every env runs out of steps and is re-placed.  After every launch: masks, closest indices, collision flags, done and timers
and the distance, short-term-path and reward buffers bit for bit against the C oracle, the other floats (observations) within 1e-5
(tests/test_gpu_scan_synthetic.py's _check); the record rows likewise; and a handle with SIGMAENV_PRUNE=0 (the full scan) holds the same bytes in every buffer."""
import numpy as np
import pytest

import oracle_binding as ob
import synthetic_maps as sm
import test_gpu_parity as tp
import test_gpu_scan_synthetic as ts
import test_scan_bound_host as hb
from sigmarl_amd import capi
from sigmarl_amd.params import Parameters, make_config

MAPS = ("hairpin", hb.DENSE_BOUNDARY, "cpm_entire")
# N -> (envs, cfg.envs_per_group, (SN, SG) of the step kernel's instantiation)
SHAPES = {16: (4, 1, (16, 1)), 4: (16, 4, (4, 4)), 3: (21, 5, (0, 0)), 1: (64, 1, (0, 0))}
MAX_STEPS = 9  # four single steps, then the launch of eight: every env runs out of steps inside it


def _selection(name, N):
    """Row indices for the B * N slots (slot b * N + i: agent i of env b): the rows a defect would lose first, then the rows where only a corner's term keeps a chunk,
    then the rows that drop a chunk, then the others; the first-agent slots take the rows the host test evaluates as first agents."""
    B = SHAPES[N][0]
    rows = hb.state_rows(name)[0]
    lost = hb.rows_a_defect_loses(name, ("placed", "stepped", "jumped"))
    drop, corner = hb.exercising_rows(name)
    prio = list(dict.fromkeys(list(range(sm.N_STATES, len(rows))) + sorted(set().union(*lost.values())) + corner + drop + list(range(sm.N_STATES))))
    firsts = [r for r in prio if r % 4 == 0 or r >= sm.N_STATES]
    sel = np.full(B * N, -1)
    sel[::N] = (firsts + [r for r in prio if r not in firsts])[:B]
    rest = [r for r in prio if r not in set(sel.tolist())]
    sel[sel < 0] = rest[:B * N - B]
    return sel


def _placement(mp, N, rows):
    B = SHAPES[N][0]
    ids = np.zeros((B * N, 4), np.int32)
    ids[:, 0] = mp.list_first[0] + rows[:, 0].astype(np.int32)
    ids[:, 2] = rows[:, 0].astype(np.int32)
    ids[:, 3] = rows[:, 1].astype(np.int32)
    return np.repeat(np.arange(B), N).astype(np.int32), np.tile(np.arange(N), B).astype(np.int32), ids, sm.state8(rows)


def _same_bytes(pruned, full, tag):
    for which in tp.INT_BUFS + tp.FLT_BUFS:
        assert full.get(which).tobytes() == pruned.get(which).tobytes(), f"{tag}: buffer {which} differs between the full and the pruned scan"


def _drive(name, N, devs, ora):
    import torch
    from sigmarl_amd.shard import slab_width, unpack_slab

    B = SHAPES[N][0]
    mp = hb.map_table(name)
    pf, pc = mp.list_first[0], mp.list_count[0]
    rows, tele = hb.state_rows(name)
    sel = _selection(name, N)
    rows, tele = rows[sel], tele[sel]
    rows[::N, 5] = 0.8  # the first agents at speed: 0.04 m per step ahead of their corner queries
    rng = np.random.default_rng(77 * MAPS.index(name) + N)
    envs = devs + [ora]
    seen = {"stale_move": 0.0, "jump": 0, "done": 0}

    def actions():
        return np.stack([rng.uniform(0.2, 1.0, (B, N)), rng.uniform(-0.5, 0.5, (B, N))], axis=-1).astype(np.float32)

    def check(tag):
        ts._check(envs, f"{name} N={N}: {tag}")
        if len(devs) == 2:
            _same_bytes(devs[0], devs[1], f"{name} N={N}: {tag}")

    def step(tag):
        before = ora.get(capi.BUF_STATE).reshape(B, N, 8)[:, 0, :2].copy()
        act = actions()
        for e in envs:
            e.step(act)
        check(tag)
        return float(np.linalg.norm(ora.get(capi.BUF_STATE).reshape(B, N, 8)[:, 0, :2] - before, axis=1).max())

    for e in envs:
        e.reset(*_placement(mp, N, rows), 1)
        e.observe()
    check("reset + observe")
    seen["stale_move"] = max(step("step 0"), step("step 1"))  # (the first agent's corner queries lie one move behind)
    # the first agents jump: their state is written, the vertices their corner queries use and their closest indices stay
    st8 = sm.state8(tele[::N])
    for d in devs:
        d.env.buffer(capi.BUF_STATE).view(B, N, 8)[:, 0, :] = torch.as_tensor(st8).to(d.env.device)
        d.env.sync()
    ora.get(capi.BUF_STATE, copy=False).reshape(B, N, 8)[:, 0, :] = st8
    assert all(np.array_equal(e.get(capi.BUF_STATE).reshape(B, N, 8)[:, 0], st8) for e in envs)
    far = np.linalg.norm(ora.get(capi.BUF_VERTICES).reshape(B, N, 5, 2)[:, 0, 0] - st8[:, :2], axis=1)
    seen["jump_m"] = float(far.max())
    stale = ora.get(capi.BUF_CLOSEST).copy()
    step("step 2, the first agents moved by up to %.1f m" % far.max())
    seen["jump"] = int(np.abs(ora.get(capi.BUF_CLOSEST).astype(int) - stale).max())  # (the step kernel's scan started from indices this far off)
    stale = ora.get(capi.BUF_CLOSEST).copy()
    for e in envs:
        e.reset(*_placement(mp, N, tele), 0)
        e.observe()
    check("teleport reset + observe")
    seen["jump"] = max(seen["jump"], int(np.abs(ora.get(capi.BUF_CLOSEST).astype(int) - stale).max()))  # (... and the reset's scan)
    step("step 3")
    acts = np.stack([actions() for _ in range(8)])
    recs = []
    for d in devs:
        rec = torch.full((8, B, slab_width(N, d.env.D)), float("nan"), device=d.env.device)
        d.env.step_autoreset_n(torch.as_tensor(acts).to(d.env.device).contiguous(), rec, seed=5, counter0=1, path_first=pf, path_count=pc)
        d.env.sync()
        recs.append(unpack_slab(rec, N, d.env.D))
    for k in range(8):
        ora.step(acts[k])
        for obs, rew, dn in recs:
            assert np.abs(obs[k].cpu().numpy() - ora.get(capi.BUF_OBS)).max() <= tp.FTOL, f"{name} N={N}: record row {k}: observations"
            assert np.array_equal(rew[k].cpu().numpy().reshape(-1), ora.get(capi.BUF_REWARD).reshape(-1)), f"{name} N={N}: record row {k}: rewards"
            assert np.array_equal(dn[k].cpu().numpy().reshape(-1), ora.get(capi.BUF_DONE).astype(bool).reshape(-1)), f"{name} N={N}: record row {k}: done"
        seen["done"] += int(ora.get(capi.BUF_DONE).sum())
        ora.auto_reset(5, 1 + k, pf, pc)
    check("step_autoreset_n of 8 steps")
    return seen


def _config(name, N):
    mp = hb.map_table(name)
    p = Parameters(n_agents=N, scenario_type=name, is_use_mtv_distance=False, rew_method="distance", dt=0.05, is_apply_mask=False, is_obs_noise=False,
                   max_steps=MAX_STEPS)
    cfg = make_config(p, mp, SHAPES[N][0])
    cfg.envs_per_group = SHAPES[N][1]
    return cfg, mp


@pytest.mark.parametrize("name", MAPS)
def test_selection_holds_the_rows_that_exercise_the_rule(name):
    """No GPU: every case places the extra first agents, rows where a corner's term alone keeps a chunk and rows that drop a chunk; the 16-, 4- and 3-agent cases also
    every row a planted defect would lose."""
    lost = set().union(*hb.rows_a_defect_loses(name, ("placed", "stepped", "jumped")).values())
    drop, corner = hb.exercising_rows(name)
    for N in SHAPES:
        sel = _selection(name, N)
        assert len(set(sel.tolist())) == len(sel) == SHAPES[N][0] * N <= 64 * N and SHAPES[N][0] <= 64
        assert set(range(sm.N_STATES, len(hb.state_rows(name)[0]))) <= set(sel[::N].tolist())
        assert set(sel.tolist()) & set(corner) and set(sel.tolist()) & set(drop)
        if N > 1:
            assert lost <= set(sel.tolist()), (name, N, sorted(lost - set(sel.tolist())))


@pytest.mark.parametrize("N", sorted(SHAPES))
@pytest.mark.parametrize("name", MAPS)
def test_workload_meets_its_conditions_on_the_oracle(name, N):
    """No GPU: the driver alone, on the oracle -- a first agent more than 0.03 m ahead of its corner queries after a step and metres after the jump, closest indices
    stale by more than 100 at the teleport, every env finished inside the launch."""
    cfg, mp = _config(name, N)
    ora = ob.OracleEnv(cfg, mp)
    try:
        seen = _drive(name, N, [], ora)
    finally:
        ora.close()
    assert seen["stale_move"] > 0.03 and seen["jump_m"] > 0.3 and seen["jump"] > 100 and seen["done"] >= SHAPES[N][0], seen


@pytest.mark.gpu
@pytest.mark.parametrize("N", sorted(SHAPES))
@pytest.mark.parametrize("name", MAPS)
def test_scan_with_the_per_query_bound_equals_the_oracle(name, N, monkeypatch):
    cfg, mp = _config(name, N)
    pruned, full, ora = ts._handle(monkeypatch, cfg, mp), ts._handle(monkeypatch, cfg, mp, {"SIGMAENV_PRUNE": 0}), ob.OracleEnv(cfg, mp)
    try:
        ls = pruned.env.launch_shape()
        assert (ls["pruned_scan"], full.env.launch_shape()["pruned_scan"]) == (1, 0), ls
        assert ls["wave_G"] == SHAPES[N][1] and tuple(ls["instantiation"][2:4]) == SHAPES[N][2], ls
        _drive(name, N, [pruned, full], ora)
    finally:
        pruned.close()
        full.close()
        ora.close()
