"""The lane-boundary scan of the HIP kernels on maps beyond the shipped ones (run with -m gpu on an MI355X).

Maps and query states: tests/synthetic_maps.py (257 and 258 points, a dense boundary that overflows the near list, a hairpin, a 5e-10 m segment); that the states
reach what they are meant to reach is asserted on the reference's numbers in tests/test_scan_synthetic_host.py, and the oracle is pinned on the reference there.
Here every map runs at 16 agents (fixed 16 x 1 instantiation), 4 (fixed 4 x 4), 3 (generic, five envs per wavefront, ragged last tile) and 1 (one task per
polyline: 64 candidate chunks fill ITEM_CAP's floor exactly) through

  reset with the given states + observe (the stand-alone kernels), six single steps with the far-teleport reset (closest indices stale by up to 250) in their
  middle, and one step_autoreset_n launch of eight steps with max_steps small enough that envs are re-placed from the start table inside the launch,

and after every launch the comparison of test_gpu_parity._compare_all holds against the C oracle: masks, indices, done and timers bit for bit, floats within FTOL;
on top of it the distance, short-term-path and reward buffers must not differ in a single bit (the scan's arithmetic is the oracle's, DESIGN.md "Pruned scan").
No diagnostic switch is set unless a test says so."""
import numpy as np
import pytest

import oracle_binding as ob
import synthetic_maps as sm
import test_gpu_cbf as tc
import test_gpu_parity as tp
from sigmarl_amd import capi, cbf
from sigmarl_amd.maps import MapTable
from sigmarl_amd.params import Parameters, make_config

SWITCHES = ("SIGMAENV_WAVE_G", "SIGMAENV_WPB", "SIGMAENV_WAVE_SPEC", "SIGMAENV_FASTDIV", "SIGMAENV_PRUNE", "SIGMAENV_G", "SIGMAENV_BLOCK", "SIGMAENV_RESET_BLOCK")
# N -> (envs, cfg.envs_per_group, the step kernel's instantiation <FASTDIV, PAR, SN, SG, VAR, MTVS> on a map with the shared-reciprocal division)
SHAPES = {16: (6, 1, (True, True, 16, 1, False, False)), 4: (24, 4, (True, True, 4, 4, False, False)), 3: (24, 5, (True, True, 0, 0, False, False)),
          1: (24, 1, (True, True, 0, 0, False, False))}
BIT_EXACT = (capi.BUF_SHORT_TERM, capi.BUF_DIST_REF, capi.BUF_DIST_LEFT, capi.BUF_DIST_RIGHT, capi.BUF_DIST_BOUND, capi.BUF_REWARD)
MAX_STEPS = 9  # six single steps, then the launch of eight: every env runs out of steps inside it

_maps = {}


def _map(name):
    if name not in _maps:
        _maps[name] = MapTable(name, table=sm.table(name))
    return _maps[name]


def _config(name, N, **kw):
    mp = _map(name)
    p = Parameters(n_agents=N, scenario_type=name, is_use_mtv_distance=False, rew_method=kw.pop("rew_method", "distance"), dt=0.05, is_apply_mask=False,
                   is_obs_noise=False, max_steps=MAX_STEPS, **kw)
    cfg = make_config(p, mp, SHAPES[N][0])
    cfg.envs_per_group = SHAPES[N][1]
    return p, cfg, mp


def _handle(monkeypatch, cfg, mp, switches=None):
    with monkeypatch.context() as m:
        for k in SWITCHES:
            m.delenv(k, raising=False)
        for k, v in (switches or {}).items():
            m.setenv(k, str(v))
        return tp._hip_env(cfg, mp)


def _placement(name, N, rows):
    """(env index, agent index, path ids, state8) that put state row b * N + i on agent i of env b."""
    B = SHAPES[N][0]
    rows = rows[:B * N]
    mp = _map(name)
    ids = np.zeros((B * N, 4), np.int32)
    ids[:, 0] = mp.list_first[0] + rows[:, 0].astype(np.int32)
    ids[:, 2] = rows[:, 0].astype(np.int32)
    ids[:, 3] = rows[:, 1].astype(np.int32)
    return np.repeat(np.arange(B), N).astype(np.int32), np.tile(np.arange(N), B).astype(np.int32), ids, sm.state8(rows)


def _check(envs, tag):
    ora = envs[-1]
    for dev in envs[:-1]:
        diff = {}
        tp._compare_all(dev, ora, tag, diff)
        for which in BIT_EXACT:
            assert which not in diff, f"{tag}: float buffer {which} differs from the oracle in {diff[which]} values (required: bit for bit)"


def _drive(name, N, envs):
    """The workload on every env of `envs` (HIP handles first, the oracle last); returns what happened, counted on the oracle."""
    B = SHAPES[N][0]
    mp, ora = _map(name), envs[-1]
    pf, pc = mp.list_first[0], mp.list_count[0]
    rng = np.random.default_rng(1000 * sm.NAMES.index(name) + N)
    seen = {"lane_hits": 0, "done": 0, "replaced": 0}

    def actions():
        return np.stack([rng.uniform(-0.2, 1.0, (B, N)), rng.uniform(-0.5, 0.5, (B, N))], axis=-1).astype(np.float32)

    place = _placement(name, N, sm.states(name))
    for e in envs:
        e.reset(*place, 1)
        e.observe()
    _check(envs, f"{name} N={N}: reset + observe")
    seen["lane_hits"] += int(ora.get(capi.BUF_COL_FLAGS)[..., 0].sum())
    for t in range(6):
        if t == 3:
            # the far teleport: every agent, singly (full_env = 0: timers and the other agents stay), to the mirrored arc length of its path -- the other end, on the
            # hairpin the other leg 0.3 m beside -- while the closest indices it holds are up to 250 segments stale
            stale = ora.get(capi.BUF_CLOSEST).copy()
            tele = _placement(name, N, sm.teleported(name))
            for e in envs:
                e.reset(*tele, 0)
                e.observe()
            _check(envs, f"{name} N={N}: teleport reset + observe")
            seen["jump"] = int(np.abs(ora.get(capi.BUF_CLOSEST).astype(int) - stale).max())
        act = actions()
        for e in envs:
            e.step(act)
        _check(envs, f"{name} N={N}: step {t}")
        seen["lane_hits"] += int(ora.get(capi.BUF_COL_FLAGS)[..., 0].sum())
    acts = np.stack([actions() for _ in range(8)])
    for dev in envs[:-1]:
        import torch

        dev.env.step_autoreset_n(torch.as_tensor(acts).to(dev.env.device).contiguous(), None, seed=5, counter0=1, path_first=pf, path_count=pc)
        dev.env.sync()
    for k in range(8):
        ora.step(acts[k])
        done = ora.get(capi.BUF_DONE).astype(bool)
        seen["done"] += int(done.sum())
        before = ora.get(capi.BUF_STATE)[done].copy()
        ora.auto_reset(5, 1 + k, pf, pc)
        if done.any():
            seen["replaced"] += int((np.abs(ora.get(capi.BUF_STATE)[done] - before).max(axis=(1, 2)) > 0).sum())
    _check(envs, f"{name} N={N}: step_autoreset_n of 8 steps")
    return seen


@pytest.mark.parametrize("N", sorted(SHAPES))
@pytest.mark.parametrize("name", sm.NAMES)
def test_workload_meets_its_conditions_on_the_oracle(name, N):
    """No GPU: the driver alone, on the oracle -- boundary collisions happen, envs finish inside the eight-step launch and are re-placed from the start table."""
    _, cfg, mp = _config(name, N)
    ora = ob.OracleEnv(cfg, mp)
    seen = _drive(name, N, [ora])
    ora.close()
    assert seen["lane_hits"] > 0 and seen["done"] >= SHAPES[N][0] and seen["replaced"] > 0 and seen["jump"] >= (100 if name != "origin" else 50), seen


@pytest.mark.gpu
@pytest.mark.parametrize("N", sorted(SHAPES))
@pytest.mark.parametrize("name", sm.NAMES)
def test_scan_on_synthetic_map_equals_the_oracle(name, N, monkeypatch):
    _, cfg, mp = _config(name, N)
    dev, ora = _handle(monkeypatch, cfg, mp), ob.OracleEnv(cfg, mp)
    try:
        ls = dev.env.launch_shape()
        B, G, inst = SHAPES[N]
        assert ls["pruned_scan"] == (0 if name == "long258" else 1), ls   # 257 points: 64 chunks, pruned; 258: the full scan
        assert ls["map_fast_div"] == (0 if name == "origin" else 1), ls    # a segment of squared length below 2^-60 turns the shared reciprocal off
        assert (ls["wave_G"], ls["wave_wpb"]) == (G, 1), ls
        assert ls["instantiation"] == ((False, inst[1], 0, 0, False, False) if name == "origin" else inst), ls
        _drive(name, N, [dev, ora])
    finally:
        dev.close()
        ora.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,N", [("long257", 16), ("long257", 1), ("dense", 4), ("dense", 3)])
def test_full_scan_by_switch_gives_the_same_bits(name, N, monkeypatch):
    """SIGMAENV_PRUNE=0 on the maps the pruned scan takes: same oracle comparison, and every buffer equal to the pruned handle's byte for byte."""
    _, cfg, mp = _config(name, N)
    full, pruned, ora = _handle(monkeypatch, cfg, mp, {"SIGMAENV_PRUNE": 0}), _handle(monkeypatch, cfg, mp), ob.OracleEnv(cfg, mp)
    try:
        assert (full.env.launch_shape()["pruned_scan"], pruned.env.launch_shape()["pruned_scan"]) == (0, 1)
        _drive(name, N, [full, pruned, ora])
        for which in tp.INT_BUFS + tp.FLT_BUFS:
            assert full.get(which).tobytes() == pruned.get(which).tobytes(), f"{name} N={N}: buffer {which} differs between the full and the pruned scan"
    finally:
        full.close()
        pruned.close()
        ora.close()


def _cmp_cbf(dev, ora, got, want, tag):
    """tests/test_gpu_cbf.py's _cmp_margins and _cmp_rewards (MARGIN_RTOL, REW_TOL) for states on which the reference's formula itself leaves the numbers: a vehicle
    whose stencil reaches past the end of its path has +-inf margins and NaN channels in the oracle (x - y is NaN there, which the helpers of test_gpu_cbf.py do not
    expect).  Non-finite entries must be the SAME non-finite value on both sides; every finite entry is held to the same bars.  Returns the finite margins compared."""
    n = 0
    for key, x, y in zip(("lane_left", "lane_right", "pair"), got, want):
        fin = np.isfinite(y)
        assert np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(x[np.isinf(y)], y[np.isinf(y)]) and np.array_equal(np.isfinite(x), fin), \
            f"{tag}: {key}: different NaN / infinite entries"
        if fin.any():
            d = np.abs(x[fin] - y[fin]) / np.maximum(1.0, np.abs(y[fin]))
            assert d.max() <= tc.MARGIN_RTOL, f"{tag}: {key}: max rel err {d.max():.3e}"
            n += int(fin.sum())
    a, b = dev.get(capi.BUF_REWARD_INFO)[4:7], ora.get(capi.BUF_REWARD_INFO)[4:7]
    fin = np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isfinite(a), fin) and np.array_equal(a[np.isinf(b)], b[np.isinf(b)]), \
        f"{tag}: reward channels: different NaN / infinite entries"
    assert np.abs(a[fin].astype(np.float64) - b[fin]).max() <= tc.REW_TOL, f"{tag}: reward channels differ by {np.abs(a[fin] - b[fin]).max()}"
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("N", [4, 16])
@pytest.mark.parametrize("name", ["long257", "long258", "hairpin"])
def test_cbf_margins_on_synthetic_map_equal_the_oracle(name, N, monkeypatch):
    """The CBF stencil kernel on tables from cbf.segment_tables: the five-point path (one or two chunks: the first set of four is clamped), chunks up to 63, and
    the branch without chunk boxes (long258).  Margins within MARGIN_RTOL and reward channels within REW_TOL of tests/test_gpu_cbf.py."""
    p, cfg, mp = _config(name, N, rew_method="cbf", is_solve_qp=False, is_using_cbf_training=True)
    dev, ora = _handle(monkeypatch, cfg, mp), ob.OracleEnv(cfg, mp)
    try:
        seg_l, seg_r = cbf.load_segment_tables(mp)
        cc = cbf.make_cbf_config(p)
        rng = np.random.default_rng(N)
        n_finite = 0
        for tag, rows in (("given states", sm.states(name)), ("teleported", sm.teleported(name))):
            place = _placement(name, N, rows)
            assert (place[2][:, 2] == 1).any()  # the map's second path (long maps: the five-point one; hairpin: the closed loop) is among them
            for e in (dev, ora):
                if tag == "given states":
                    e.cbf_attach(cc, seg_l, seg_r)
                e.reset(*place, 1 if tag == "given states" else 0)
                e.observe()
            for t in range(2):
                act = np.stack([rng.uniform(-0.2, 1.0, cfg.n_envs * N), rng.uniform(-0.5, 0.5, cfg.n_envs * N)], axis=-1).astype(np.float32).reshape(cfg.n_envs, N, 2)
                n_finite += _cmp_cbf(dev, ora, dev.cbf_rewards(act), ora.cbf_rewards(act), f"{name} N={N} {tag} {t}")
        assert n_finite > 2 * 2 * cfg.n_envs * N * 3  # (most margins are ordinary numbers)
    finally:
        dev.close()
        ora.close()
