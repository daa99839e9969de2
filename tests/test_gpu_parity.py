"""Parity tests proper (run with -m gpu on an MI355X): the HIP fused step, called through the C-ABI, against
(1) the reference goldens, (2) the CPU oracle on seeded inputs, (3) size-independent properties at BASELINE sizes.

Bar: masks / indices / counters bit-exact; fp32 states, rewards, observations within 1e-5 abs (mtv distance included, against
the reference goldens only, see test_oracle_golden.py; HIP vs oracle share the arithmetic contract and are held to 1e-5).
"""
import os

import numpy as np
import pytest

import oracle_binding as ob
import traj_replay as tr
from sigmarl_amd import capi
from sigmarl_amd.maps import load_map
from sigmarl_amd.params import Parameters, make_config

pytestmark = pytest.mark.gpu

FTOL = 1e-5
MTV_TOL = 1e-5

INT_BUFS = [capi.BUF_PATH, capi.BUF_CLOSEST, capi.BUF_COL_AGENTS, capi.BUF_COL_FLAGS, capi.BUF_NEARING, capi.BUF_DONE, capi.BUF_TIMER]
FLT_BUFS = [capi.BUF_STATE, capi.BUF_PREV_POS, capi.BUF_VERTICES, capi.BUF_SHORT_TERM, capi.BUF_DIST_REF, capi.BUF_DIST_LEFT,
            capi.BUF_DIST_RIGHT, capi.BUF_DIST_BOUND, capi.BUF_DIST_AGENTS, capi.BUF_REWARD, capi.BUF_REWARD_INFO, capi.BUF_OBS, capi.BUF_ACTION]


def _hip_env(cfg, mp):
    from sigmarl_amd.env import NumpyAdapter, SigmaEnv

    return NumpyAdapter(SigmaEnv(cfg=cfg, map_table=mp, device="cuda:0"))


def test_extension_is_loaded_and_exports_abi():
    lib = capi.load_library()
    # (SIGMAENV_LIB: an explicitly chosen other build of the same HIP library from the same directory -- the poison build of tools/poison_suite.sh)
    chosen = os.environ.get("SIGMAENV_LIB")
    assert lib.path.endswith("sigmarl_amd/csrc/libsigmaenv.so") or (chosen and lib.path == chosen and os.path.basename(chosen).startswith("libsigmaenv"))
    assert lib.obs_dim(2) == 32
    # the library was built from the sources of this tree (the .so files are not rebuilt on the GPU box: a stale one must not be tested silently)
    assert lib.build_id().decode() == capi.source_build_id()


@pytest.mark.parametrize("name", tr.TRAJ_NAMES)
def test_hip_vs_reference_goldens(name):
    z, meta = tr.load_fixture(name)
    cfg, mp = tr.config_from_meta(meta)
    env = _hip_env(cfg, mp)
    twin = ob.OracleEnv(cfg, mp)  # the quirk-free oracle: holds the envs the reference's env-0 reset side effect hides from the snapshot comparison
    rep = tr.replay(env, z, meta, mp, twin=twin)
    env.close()
    twin.close()
    assert getattr(rep, "unchecked", 0) == 0
    assert rep.total_mismatch() == 0, str(rep)
    if rep.cbf_count:
        print(f"{name}: {rep}")
    assert rep.cbf_ok(name), str(rep)
    for key, err in rep.max_abs.items():
        tol = MTV_TOL if (meta["is_use_mtv_distance"] and key in ("dist_agents", "obs", "reward", "rew_total", "rew_near_other_agents")) else FTOL
        assert err <= tol, (key, err, str(rep))


def _compare_all(dev, ora, tag, diff_by_buffer=None):
    n_float_diff = 0
    for which in INT_BUFS:
        a, b = dev.get(which), ora.get(which)
        assert np.array_equal(a, b), f"{tag}: integer/mask buffer {which}: {(a != b).sum()} mismatches"
    for which in FLT_BUFS:
        a, b = dev.get(which), ora.get(which)
        both_inf = np.isinf(a) & np.isinf(b) & (np.sign(a) == np.sign(b))
        d = np.where(both_inf, 0.0, np.abs(a.astype(np.float64) - b.astype(np.float64)))
        assert d.max() <= FTOL, f"{tag}: float buffer {which}: max |err| {d.max()}"
        if which != capi.BUF_OBS:  # the HIP observation uses the rotation form of the ego transform (no atan2): ~1e-7 off, by design
            nd = int((a != b).sum() - (np.isnan(a) & np.isnan(b)).sum())
            n_float_diff += nd
            if nd and diff_by_buffer is not None:
                diff_by_buffer[which] = diff_by_buffer.get(which, 0) + nd
    return n_float_diff


class _OneEnvFixture:
    """Env `e` of a golden trajectory as a fixture of its own (B = 1): every [B, ...] / [T, B, ...] array sliced, the reset events of the other envs dropped."""

    def __init__(self, z, e):
        B = z["init_pos"].shape[0]
        keep = np.nonzero(z["ev_env"] == e)[0]
        self._d = {}
        for k in z.files:
            a = z[k]
            if k == "meta_json":
                pass
            elif k.startswith("ev_"):
                a = a[keep]
                if k == "ev_env":
                    a = np.zeros_like(a)
            elif k.startswith("init_"):
                a = a[e:e + 1]
            elif k.startswith("post_") or k.startswith("next_") or k in ("act", "done"):   # [T, B, ...]
                assert a.shape[1] == B, k
                a = a[:, e:e + 1]
            self._d[k] = a
        self.files = list(self._d)

    def __getitem__(self, k):
        return self._d[k]


# (env 0 only: the reference's env-0 reset quirk -- traj_replay.replay -- leaves traces in the OTHER envs' snapshots that only the batched replay can account for)
@pytest.mark.parametrize("name,e", [("intersection4_c2c", 0), ("cpm16_c2c", 0), ("intersection4_birdview_mask", 0), ("onramp6_mtv", 0), ("intersection4_mask", 0)])
def test_single_env_replay_of_reference_goldens(name, e):
    """BASELINE config 1 is "4 agents, num_envs = 1": a launch of ONE wavefront.  Env e of a reference trajectory replayed ALONE through the C-ABI (a handle with
    n_envs = 1): the same tolerances as the batched replay (masks / indices / counters bit-exact, fp32 within 1e-5 of the reference)."""
    z, meta = tr.load_fixture(name)
    if "cbf_in_state" in z.files:
        pytest.skip("CBF fixtures carry per-batch margins")
    one = _OneEnvFixture(z, e)
    meta1 = dict(meta, B=1)
    cfg, mp = tr.config_from_meta(meta1, n_envs=1)
    assert cfg.n_envs == 1
    env = _hip_env(cfg, mp)
    twin = ob.OracleEnv(cfg, mp)
    rep = tr.replay(env, one, meta1, mp, twin=twin)
    env.close()
    twin.close()
    assert getattr(rep, "unchecked", 0) == 0
    assert rep.total_mismatch() == 0, str(rep)
    assert rep.worst_float() <= FTOL, str(rep)


CASES = [
    # scenario, N, B, mtv, rew_method, dt, testing, steps
    ("cpm_entire", 16, 64, False, "distance", 0.05, False, 12),
    ("cpm_entire", 16, 48, True, "ttc_sparse", 0.1, False, 12),
    ("cpm_entire", 5, 33, False, "sparse", 0.05, False, 10),       # ragged: N not a divisor of the wave count, odd B
    ("cpm_entire", 32, 16, True, "distance_sparse", 0.05, False, 8),  # 32 agents: two agents per wavefront slot
    ("cpm_entire", 2, 7, False, "ttc", 0.05, True, 10),            # minimum: 2 agents, 1 neighbour, testing-mode reward/done
    ("cpm_entire", 8, 24, True, "sparse", 0.1, True, 12),           # testing mode: colliders are re-placed one by one on device
    ("intersection_1", 4, 40, False, "distance", 0.1, False, 16),  # non-loop map: entry/exit segments, reset requests
    ("on_ramp_1", 6, 40, True, "ttc", 0.1, False, 16),
    # BASELINE config 1's shape: num_envs = 1 -- ONE wavefront, one tile, every per-env reduction over a single env
    ("intersection_1", 4, 1, False, "distance", 0.1, False, 40),
    ("cpm_entire", 16, 1, False, "distance", 0.05, False, 40),
    ("cpm_entire", 16, 1, True, "ttc_sparse", 0.1, True, 30),
]


@pytest.mark.parametrize("scen,N,B,mtv,rew,dt,testing,steps", CASES)
def test_hip_vs_oracle_seeded(scen, N, B, mtv, rew, dt, testing, steps):
    """Same seeded inputs through the HIP path and the oracle, incl. the shared-specification device-side resets."""
    p = Parameters(n_agents=N, scenario_type=scen, is_use_mtv_distance=mtv, rew_method=rew, dt=dt, is_testing_mode=testing,
                   is_apply_mask=False, is_obs_noise=False, max_steps=9)
    mp = load_map(scen)
    cfg = make_config(p, mp, B)
    dev, ora = _hip_env(cfg, mp), ob.OracleEnv(cfg, mp)
    dev.env.buffer(capi.BUF_DONE).fill_(1)
    ora.get(capi.BUF_DONE, copy=False)[:] = 1
    pf, pc = mp.list_first[0], mp.list_count[0]
    dev.auto_reset(5, 0, pf, pc)
    ora.auto_reset(5, 0, pf, pc)
    _compare_all(dev, ora, "after initial reset")
    rng = np.random.default_rng(123)
    n_diff = 0
    by_buf = {}
    seen_done = seen_req = 0
    for t in range(steps):
        act = np.stack([rng.uniform(-0.2, 1.3, (B, N)), rng.uniform(-0.7, 0.7, (B, N))], axis=-1).astype(np.float32)
        if t % 3 == 2:  # gentle actions so that some episodes live long enough to hit max_steps
            act = np.stack([rng.uniform(0.0, 0.3, (B, N)), rng.uniform(-0.05, 0.05, (B, N))], axis=-1).astype(np.float32)
        dev.step(act)
        ora.step(act)
        n_diff += _compare_all(dev, ora, f"step {t}", by_buf)
        seen_done += int(ora.get(capi.BUF_DONE).sum())
        seen_req += int(ora.get(capi.BUF_COL_FLAGS)[..., 3].sum())
        dev.auto_reset(5, t + 1, pf, pc)
        ora.auto_reset(5, t + 1, pf, pc)
        n_diff += _compare_all(dev, ora, f"reset after step {t}", by_buf)
    assert seen_done > 0
    if testing:
        assert seen_req > 0  # device-side per-agent resets (reset requests of unfinished envs) were exercised
    # the two sides share the arithmetic contract ("HIP vs oracle agrees on every fp32 word"): apart from the observation rows
    # (see _compare_all) NO fp32 word may differ -- the observed count is asserted, and a failure names the buffers that differ
    print(f"{scen} N={N} B={B}: differing non-observation fp32 words over the run: {n_diff}; per-agent reset requests served: {seen_req}")
    assert n_diff == 0, f"{n_diff} differing fp32 words, by buffer id: {by_buf}"
    dev.close()
    ora.close()


def test_distance_mask_hip_vs_oracle():
    """Parameters' default is_apply_mask=True on the CPM map: neighbours at or beyond 5 vehicle lengths are masked in the observation."""
    N, B = 16, 48
    p = Parameters(n_agents=N, scenario_type="cpm_entire", is_use_mtv_distance=True, rew_method="ttc", dt=0.05, is_apply_mask=True, is_obs_noise=False,
                   max_steps=9)
    mp = load_map("cpm_entire")
    cfg = make_config(p, mp, B)
    assert cfg.is_apply_mask == 1 and abs(cfg.distance_mask_agents - 1.1) < 1e-6
    dev, ora = _hip_env(cfg, mp), ob.OracleEnv(cfg, mp)
    dev.env.buffer(capi.BUF_DONE).fill_(1)
    ora.get(capi.BUF_DONE, copy=False)[:] = 1
    pf, pc = mp.list_first[0], mp.list_count[0]
    dev.auto_reset(2, 0, pf, pc)
    ora.auto_reset(2, 0, pf, pc)
    _compare_all(dev, ora, "after reset")
    rng = np.random.default_rng(5)
    masked = 0
    for t in range(8):
        act = np.stack([rng.uniform(-0.2, 1.3, (B, N)), rng.uniform(-0.7, 0.7, (B, N))], axis=-1).astype(np.float32)
        dev.step(act)
        ora.step(act)
        _compare_all(dev, ora, f"step {t}")
        blk = ora.get(capi.BUF_OBS)[..., 10:].reshape(B, N, 2, 11)
        masked += int(((blk[..., 10] == 1.0) & (blk[..., 0] == 1.0) & (blk[..., 8] == 0.0)).sum())
        dev.auto_reset(2, t + 1, pf, pc)
        ora.auto_reset(2, t + 1, pf, pc)
    assert masked > 100
    dev.close()
    ora.close()


def test_forced_overlaps_and_edge_cases():
    """Injected states: overlapping rectangles (collision masks, negative mtv), coincident agents (atan2(0,0), zero distance),
    an agent far outside the map, zero speed, steering beyond the clamp."""
    for mtv in (False, True):
        p = Parameters(n_agents=6, scenario_type="cpm_entire", is_use_mtv_distance=mtv, rew_method="distance_sparse", is_apply_mask=False,
                       is_obs_noise=False)
        mp = load_map("cpm_entire")
        B = 4
        cfg = make_config(p, mp, B)
        dev, ora = _hip_env(cfg, mp), ob.OracleEnv(cfg, mp)
        c = mp.center[3]
        st = np.zeros((B, 6, 8), np.float32)
        ids = np.zeros((B, 6, 4), np.int32)
        ids[..., 0] = 3
        ids[..., 2] = 3
        for b in range(B):
            for i in range(6):
                k = 5 + 9 * i
                st[b, i, 0:2] = c[k]
                st[b, i, 2] = mp.yaw[3][k]
        st[0, 1, 0:2] = st[0, 0, 0:2] + np.float32([0.05, 0.01])  # overlapping pair
        st[0, 1, 2] = st[0, 0, 2] + 0.4
        st[1, 2] = st[1, 3]                                         # coincident agents
        st[2, 4, 0:2] = np.float32([9.0, -3.0])                     # far outside the 4.5 x 4.0 world
        st[3, :, 3] = 0.9
        st[3, :, 4] = 0.5
        env_idx = np.repeat(np.arange(B), 6)
        agent_idx = np.tile(np.arange(6), B)
        for e in (dev, ora):
            e.reset(env_idx, agent_idx, ids.reshape(-1, 4), st.reshape(-1, 8), 1)
            e.observe()
        _compare_all(dev, ora, f"mtv={mtv} injected reset")
        rng = np.random.default_rng(7)
        for t in range(5):
            act = np.stack([rng.uniform(-2, 2, (B, 6)), rng.uniform(-2, 2, (B, 6))], axis=-1).astype(np.float32)
            dev.step(act)
            ora.step(act)
            _compare_all(dev, ora, f"mtv={mtv} step {t}")
        ca = ora.get(capi.BUF_COL_AGENTS)
        da = ora.get(capi.BUF_DIST_AGENTS)
        if not mtv:
            assert ca[0, 0, 1] == 1 and ca[0, 1, 0] == 1
        else:
            assert da[0, 0, 1] < 0
        dev.close()
        ora.close()


@pytest.mark.parametrize("N,B", [(16, 4096), (32, 8192)])
def test_full_size_properties(N, B):
    """BASELINE sizes (config 2: 16 x 4096, config 4 shape: 32 x 8192): determinism, invariants, and oracle parity on a slice."""
    scen = "cpm_entire"
    p = Parameters(n_agents=N, scenario_type=scen, is_use_mtv_distance=False, rew_method="distance", is_apply_mask=False, is_obs_noise=False)
    mp = load_map(scen)
    cfg = make_config(p, mp, B)
    pf, pc = mp.list_first[0], mp.list_count[0]
    rng = np.random.default_rng(1)
    acts = [np.stack([rng.uniform(0, 1, (B, N)), rng.uniform(-0.25, 0.25, (B, N))], axis=-1).astype(np.float32) for _ in range(3)]

    def run():
        dev = _hip_env(cfg, mp)
        dev.env.buffer(capi.BUF_DONE).fill_(1)
        dev.auto_reset(9, 0, pf, pc)
        outs = []
        for t, a in enumerate(acts):
            dev.step(a)
            outs.append({w: dev.get(w) for w in INT_BUFS + FLT_BUFS})
            dev.auto_reset(9, t + 1, pf, pc)
        dev.close()
        return outs

    o1, o2 = run(), run()
    for a, b in zip(o1, o2):  # same input -> bit-identical output across launches (no atomics / races in the data path)
        for w in a:
            assert a[w].tobytes() == b[w].tobytes(), f"non-deterministic buffer {w}"
    last = o1[-1]
    st = last[capi.BUF_STATE]
    assert np.isfinite(st).all() and np.isfinite(last[capi.BUF_OBS]).all() and np.isfinite(last[capi.BUF_REWARD]).all()
    assert (np.abs(last[capi.BUF_REWARD]) <= 1.0).all()
    assert np.array_equal(last[capi.BUF_PREV_POS], st[..., 0:2])          # state_buffer.add after the last agent
    da = last[capi.BUF_DIST_AGENTS]
    assert np.array_equal(da, da.transpose(0, 2, 1))                      # symmetric matrix
    assert (last[capi.BUF_DIST_REF] >= 0).all()
    ca = last[capi.BUF_COL_AGENTS]
    assert np.array_equal(ca, ca.transpose(0, 2, 1))
    done = last[capi.BUF_DONE].astype(bool)
    col = ca.reshape(B, -1).any(1) | last[capi.BUF_COL_FLAGS][..., 0].any(1)
    assert np.array_equal(done, col | (last[capi.BUF_TIMER][:, 0] == cfg.max_steps - 1))
    # nearest neighbours really are the two smallest entries of the distance row
    near = last[capi.BUF_NEARING]
    srt = np.sort(da, axis=-1)
    picked = np.take_along_axis(da, near.astype(np.int64), axis=-1)
    assert np.array_equal(picked, srt[..., : near.shape[-1]])
    # full-size oracle parity (the C oracle finishes this in seconds)
    ora = ob.OracleEnv(cfg, mp)
    ora.get(capi.BUF_DONE, copy=False)[:] = 1
    ora.auto_reset(9, 0, pf, pc)
    for t, a in enumerate(acts):
        ora.step(a)
        for w in INT_BUFS:
            assert np.array_equal(o1[t][w], ora.get(w)), f"full-size mismatch in buffer {w} at step {t}"
        for w in FLT_BUFS:
            assert np.abs(o1[t][w] - ora.get(w)).max() <= FTOL
        ora.auto_reset(9, t + 1, pf, pc)
    ora.close()


def test_config4_onramp_32_agents_8192_envs():
    """BASELINE config 4 on its own map: on_ramp_1, 32 agents x 8192 envs, injected start (the reference cannot place 32 agents there:
    SURVEY.md section 7), non-loop paths with entry / exit segments.  One launch per step incl. the bounded device-side resets (finished envs
    and agents that left through an exit); HIP == oracle on EVERY env, masks / indices bit-exact."""
    from sigmarl_amd.maps import injected_start

    N, B = 32, 8192
    mp = load_map("on_ramp_1")
    idx, st = injected_start(mp, N)
    p = Parameters(n_agents=N, scenario_type="on_ramp_1", is_use_mtv_distance=False, rew_method="distance", is_apply_mask=False, is_obs_noise=False,
                   dt=0.05, predefined_ref_path_idx=idx, init_state=st)
    cfg = make_config(p, mp, B)
    assert cfg.has_entry_exit
    pf, pc = mp.list_first[0], mp.list_count[0]
    dev = _hip_env(cfg, mp)
    ora = ob.OracleEnv(cfg, mp)
    ids = np.zeros((B, N, 4), np.int32)
    ids[..., 0] = np.asarray([mp.global_path(0, q) for q in idx], np.int32)[None, :]
    ids[..., 2] = np.asarray(idx, np.int32)[None, :]
    st8 = np.zeros((B, N, 8), np.float32)
    st8[..., 0:3] = np.asarray(st, np.float32)[None, :, :]
    ei, ai = np.repeat(np.arange(B, dtype=np.int32), N), np.tile(np.arange(N, dtype=np.int32), B)
    for e in (dev, ora):
        e.reset(ei, ai, ids.reshape(-1, 4), st8.reshape(-1, 8), 1)
        e.observe()
    _compare_all(dev, ora, "injected start")
    rng = np.random.default_rng(3)
    n_exit = n_req = n_done = 0
    for t in range(12):
        act = np.stack([rng.uniform(0, 1, (B, N)), rng.uniform(-0.25, 0.25, (B, N))], axis=-1).astype(np.float32)
        dev.step_autoreset(act, 5, t, pf, pc)
        ora.step(act)
        cf = ora.get(capi.BUF_COL_FLAGS)
        n_exit += int(cf[..., 2].sum()); n_req += int(cf[..., 3].sum()); n_done += int(ora.get(capi.BUF_DONE).sum())
        ora.auto_reset(5, t, pf, pc)
        _compare_all(dev, ora, f"config 4 step {t}")
    assert n_done > 0  # 32 vehicles on this map overlap: envs finish and restart through the bounded sampler
    dev.close()
    ora.close()


def test_injected_start_rule_matches_the_golden_generator():
    """sigmarl_amd.maps.injected_start == the start tests/golden/gen/gen_golden.py injected into the reference for traj_onramp32_c2c."""
    import traj_replay as tr
    from sigmarl_amd.maps import injected_start

    z, meta = tr.load_fixture("onramp32_c2c")
    idx, st = injected_start(load_map("on_ramp_1"), 32)
    assert list(meta["predefined_ref_path_idx"]) == idx
    assert np.abs(np.asarray(meta["init_state"]) - np.asarray(st)).max() <= 1e-6


@pytest.mark.parametrize("tag,testing", [("train", False), ("test", True)])
def test_device_sampler_matches_the_reference_distribution(tag, testing):
    """The HIP reset sampler's (path, point, speed) marginals == the reference's torch-RNG sampler's (chi-square, tests/golden/reset_distribution.npz;
    world_state_rt_sim.py:215-311 incl. the testing-mode range that grows with the tries), minimum spacing respected in 65536 placed agents."""
    import reset_distribution_check as rdc

    mp = load_map("cpm_entire")
    p = Parameters(n_agents=16, scenario_type="cpm_entire", is_apply_mask=False, is_obs_noise=False, is_testing_mode=testing)
    dev = _hip_env(make_config(p, mp, 2048), mp)
    got = rdc.sample_histograms(dev, mp, rounds=2)
    dev.close()
    rdc.compare(tag, got)


def test_adversarial_collinear_configurations_pruned_scan_equals_full_scan():
    """The collision PRUNING under the configurations built to break it (tests/golden/adversarial.npz, generated by the reference): rectangle
    edges exactly collinear with long straight boundary stretches and a few ulps around touching; vehicles in line with collinear side edges
    at centre distances around and far beyond the circumcircle sum.  Every pose becomes an env at rest (zero action: the pose is kept bit for
    bit); the HIP kernels (pruned boundary scan, circumcircle pre-test of pairs) must give the oracle's flags (full scan), and -- wherever
    the vertices computed from the pose equal the reference's bit for bit -- the reference's."""
    z = np.load(os.path.join(tr.GOLDEN_DIR, "adversarial.npz"))
    mp = load_map("cpm_entire")
    first = mp.list_first[0]
    p = Parameters(n_agents=2, scenario_type="cpm_entire", is_use_mtv_distance=False, rew_method="distance", is_apply_mask=False, is_obs_noise=False, dt=0.05)
    # (1) rectangle x boundaries: agent 0 carries the adversarial pose, agent 1 is parked elsewhere on the same path
    pose, pid = z["b_pose"], z["b_path"].astype(np.int64)
    B = len(pose)
    cfg = make_config(p, mp, B)
    dev, ora = _hip_env(cfg, mp), ob.OracleEnv(cfg, mp)
    st8 = np.zeros((B, 2, 8), np.float32)
    st8[:, 0, 0:3] = pose
    gp = first + pid
    far = np.minimum(mp.n_center[gp] - 5, 60)
    st8[:, 1, 0:2] = mp.center[gp, far]
    st8[:, 1, 2] = mp.yaw[gp, np.minimum(far, mp.n_yaw[gp] - 1)]
    ids = np.zeros((B, 2, 4), np.int32)
    ids[..., 0] = gp[:, None]
    ids[..., 2] = pid[:, None]
    ids[:, 1, 3] = far
    ei, ai = np.repeat(np.arange(B, dtype=np.int32), 2), np.tile(np.arange(2, dtype=np.int32), B)
    act = np.zeros((B, 2, 2), np.float32)
    for e in (dev, ora):
        e.reset(ei, ai, ids.reshape(-1, 4), st8.reshape(-1, 8), 1)
        e.step(act)
    _compare_all(dev, ora, "adversarial boundary poses")
    assert np.array_equal(ora.get(capi.BUF_STATE)[:, 0, 0:3], pose)  # at rest the step keeps the pose bit for bit
    same_v = (ora.get(capi.BUF_VERTICES)[:, 0].view(np.uint32) == z["b_vertices"].view(np.uint32)).all(axis=(1, 2))
    want = z["b_hit_left"] | z["b_hit_right"]
    got = ora.get(capi.BUF_COL_FLAGS)[:, 0, 0].astype(bool)
    assert same_v.sum() > 0.8 * B and np.array_equal(got[same_v], want[same_v])
    assert np.array_equal(dev.get(capi.BUF_COL_FLAGS)[:, 0, 0].astype(bool)[same_v], want[same_v])
    dev.close()
    ora.close()
    # (2) rectangle x rectangle: the two vehicles of an env are the pair
    pa, pb = z["r_pose_a"], z["r_pose_b"]
    B = len(pa)
    cfg = make_config(p, mp, B)
    dev, ora = _hip_env(cfg, mp), ob.OracleEnv(cfg, mp)
    st8 = np.zeros((B, 2, 8), np.float32)
    st8[:, 0, 0:3], st8[:, 1, 0:3] = pa, pb
    ids = np.zeros((B, 2, 4), np.int32)
    ids[..., 0] = first
    ei, ai = np.repeat(np.arange(B, dtype=np.int32), 2), np.tile(np.arange(2, dtype=np.int32), B)
    act = np.zeros((B, 2, 2), np.float32)
    for e in (dev, ora):
        e.reset(ei, ai, ids.reshape(-1, 4), st8.reshape(-1, 8), 1)
        e.step(act)
    _compare_all(dev, ora, "adversarial pairs")
    vo = ora.get(capi.BUF_VERTICES)
    same_v = (vo[:, 0].view(np.uint32) == z["r_vertices_a"].view(np.uint32)).all(axis=(1, 2)) & (vo[:, 1].view(np.uint32) == z["r_vertices_b"].view(np.uint32)).all(axis=(1, 2))
    got_o, got_d = ora.get(capi.BUF_COL_AGENTS)[:, 0, 1].astype(bool), dev.get(capi.BUF_COL_AGENTS)[:, 0, 1].astype(bool)
    assert same_v.sum() > 0.7 * B and np.array_equal(got_o[same_v], z["r_hit"][same_v]) and np.array_equal(got_d[same_v], z["r_hit"][same_v])
    dev.close()
    ora.close()


def test_rollout_slab_is_written_by_the_step_kernel():
    """sigmaenv_set_slab: the per-step record [obs | reward | done] equals the individual buffers (ragged tile: N=5, B=33)."""
    import torch
    from sigmarl_amd.shard import slab_width, unpack_slab

    for N, B in ((16, 64), (5, 33)):
        p = Parameters(n_agents=N, scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False)
        mp = load_map("cpm_entire")
        dev = _hip_env(make_config(p, mp, B), mp)
        env = dev.env
        env.reset_random(seed=2)
        chunk = torch.full((3, B, slab_width(N, env.D)), float("nan"), device="cuda")
        gen = torch.Generator(device="cuda").manual_seed(0)
        for t in range(3):
            env.set_slab(chunk[t])
            act = torch.rand((B, N, 2), generator=gen, device="cuda") - torch.tensor([0.0, 0.5], device="cuda")
            env.step(act)
            env.sync()
            obs, rew, done = unpack_slab(chunk[t], N, env.D)
            assert torch.equal(obs, env.obs) and torch.equal(rew, env.reward) and torch.equal(done, env.done.bool())
            env.auto_reset(seed=2)
        env.set_slab(None)
        before = chunk.clone()
        env.step(act)
        env.sync()
        assert torch.equal(before, chunk)
        dev.close()


@pytest.mark.parametrize("scen", ["intersection_1", "on_ramp_1"])
def test_device_side_agent_resets_on_exit(scen):
    """Non-loop maps: agents injected just before the end of their path leave through the exit segment; the device-side reset
    re-places exactly those agents (shared RNG specification) -- HIP == oracle through the whole episode."""
    N, B = 4, 6
    p = Parameters(n_agents=N, scenario_type=scen, is_use_mtv_distance=False, rew_method="distance", dt=0.1, is_apply_mask=False,
                   is_obs_noise=False, max_steps=1000)
    mp = load_map(scen)
    cfg = make_config(p, mp, B)
    dev, ora = _hip_env(cfg, mp), ob.OracleEnv(cfg, mp)
    ids, st = [], []
    for b in range(B):
        for i in range(N):
            gp = mp.list_first[0] + ((i + b) % mp.list_count[0])
            k = int(mp.n_center[gp]) - 4 - (b % 2)
            x, y = mp.center[gp, k]
            yaw = float(mp.yaw[gp, min(k, int(mp.n_yaw[gp]) - 1)])
            ids.append((gp, 0, gp - mp.list_first[0], k))
            st.append((x, y, yaw, 0.8, 0.0, 0.8 * np.cos(yaw), 0.8 * np.sin(yaw), 0.0))
    for e in (dev, ora):
        e.reset(np.repeat(np.arange(B), N), np.tile(np.arange(N), B), np.asarray(ids, np.int32), np.asarray(st, np.float32), 1)
        e.observe()
    act = np.zeros((B, N, 2), np.float32)
    act[..., 0] = 1.0
    served = exits = 0
    pf, pc = mp.list_first[0], mp.list_count[0]
    for t in range(10):
        dev.step(act)
        ora.step(act)
        _compare_all(dev, ora, f"{scen} step {t}")
        fl = ora.get(capi.BUF_COL_FLAGS)
        exits += int(fl[..., 2].sum())
        served += int(fl[..., 3].sum())
        before = ora.get(capi.BUF_STATE).copy()
        was_done = ora.get(capi.BUF_DONE).astype(bool)
        dev.auto_reset(11, t, pf, pc)
        ora.auto_reset(11, t, pf, pc)
        _compare_all(dev, ora, f"{scen} reset {t}")
        moved = (before[..., 0:2] != ora.get(capi.BUF_STATE)[..., 0:2]).any(-1)
        # in an unfinished env exactly the requesting agents were re-placed; a finished env is reset as a whole
        assert np.array_equal(moved[~was_done], fl[..., 3].astype(bool)[~was_done])
        assert not ora.get(capi.BUF_COL_FLAGS)[..., 3].any()
    assert exits > 0 and served > 0
    dev.close()
    ora.close()


@pytest.mark.parametrize("ns,scen,N,B,mtv,rew", [(5, "cpm_entire", 16, 96, False, "distance"), (2, "cpm_entire", 16, 64, True, "ttc"), (5, "intersection_1", 4, 64, False, "distance"),
                                                 (2, "cpm_entire", 5, 33, False, "sparse")])
def test_short_term_path_length_variants_hip_vs_oracle(ns, scen, N, B, mtv, rew):
    """n_points_short_term != 3 (road_traffic.py:316, :536-543; helper_scenario.py:892-957) is a build constant: libsigmaenv_ns<k>.so from the same
    sources.  The variant reports its constant, refuses a configuration for another one, and equals the oracle built for the same constant (pinned to the
    reference on traj_cpm8_ns5 / traj_intersection4_ns2) through fused step + reset launches, the in-kernel step loop and the rollout record."""
    import torch
    from sigmarl_amd.env import SigmaEnv

    p = Parameters(n_agents=N, scenario_type=scen, is_use_mtv_distance=mtv, rew_method=rew, dt=0.05, is_apply_mask=False, is_obs_noise=False, max_steps=10,
                   n_points_short_term=ns)
    mp = load_map(scen)
    cfg = make_config(p, mp, B)
    dev, ora = _hip_env(cfg, mp), ob.OracleEnv(cfg, mp)
    K = cfg.n_nearing
    assert dev.env.lib.path.endswith(f"libsigmaenv_ns{ns}.so") and dev.env.lib.n_short_term() == ns and ora.lib.n_short_term() == ns
    assert dev.D == ora.D == 4 + 2 * ns + 11 * K and dev.get(capi.BUF_SHORT_TERM).shape == (B, N, ns, 2)
    with pytest.raises(RuntimeError):  # the default build refuses this configuration instead of running with 3 points
        SigmaEnv(cfg=cfg, map_table=mp, device="cuda:0", lib_path=capi.DEFAULT_LIB)
    pf, pc = mp.list_first[0], mp.list_count[0]
    dev.env.buffer(capi.BUF_DONE).fill_(1)
    ora.get(capi.BUF_DONE, copy=False)[:] = 1
    dev.auto_reset(4, 0, pf, pc)
    ora.auto_reset(4, 0, pf, pc)
    _compare_all(dev, ora, "initial reset")
    rng = np.random.default_rng(ns)
    T = 16
    acts = np.stack([rng.uniform(0.0, 1.2, (T, B, N)), rng.uniform(-0.5, 0.5, (T, B, N))], axis=-1).astype(np.float32)
    W = N * (dev.D + 1) + 1
    slab = torch.zeros((B, W), device="cuda")
    dev.env.set_slab(slab)
    for t in range(T // 2):
        dev.step_autoreset(acts[t], 4, t + 1, pf, pc)
        ora.step(acts[t])
        rec_obs, rec_rew, rec_done = ora.get(capi.BUF_OBS).copy(), ora.get(capi.BUF_REWARD).copy(), ora.get(capi.BUF_DONE).copy()
        ora.auto_reset(4, t + 1, pf, pc)
        _compare_all(dev, ora, f"ns={ns} step {t}")
        row = slab.cpu().numpy()
        assert np.abs(row[:, :N * dev.D].reshape(B, N, dev.D) - rec_obs).max() <= FTOL
        np.testing.assert_array_equal(row[:, N * dev.D:N * dev.D + N], rec_rew)
        np.testing.assert_array_equal(row[:, -1] != 0, rec_done != 0)
    dev.env.set_slab(None)
    a = torch.as_tensor(acts[T // 2:]).to("cuda").contiguous()
    dev.env.step_autoreset_n(a, seed=4, counter0=50, path_first=pf, path_count=pc)
    dev.env.sync()
    for t in range(T // 2, T):
        ora.step(acts[t])
        ora.auto_reset(4, 50 + t - T // 2, pf, pc)
    _compare_all(dev, ora, f"ns={ns} after the step loop")
    dev.close()
    ora.close()


@pytest.mark.parametrize("testing", [False, True])
def test_mixed_scenario_lists_device_resets(testing):
    """cpm_mixed with device-side resets (world_state_rt_sim.py:313-358): every finished env draws its sub-scenario from cpm_scenario_probabilities
    and its agents' paths from that list; per-agent resets (exits; collisions in testing mode) keep the env's sub-scenario.  HIP == oracle on every
    buffer through fused step + reset launches (one launch per step, and the in-kernel step loop), and the HIP sampler's draws match the
    reference's (chi-square, tests/golden/reset_distribution.npz mixed_*)."""
    import torch
    import reset_distribution_check as rdc

    N, B, T = 4, 512, 24
    probs = [0.5, 0.3, 0.2]
    p = Parameters(n_agents=N, scenario_type="cpm_mixed", is_use_mtv_distance=False, rew_method="distance", dt=0.1, is_apply_mask=False, is_obs_noise=False,
                   max_steps=12, is_testing_mode=testing, cpm_scenario_probabilities=probs)
    mp = load_map("cpm_mixed")
    cfg = make_config(p, mp, B)
    dev, ora = _hip_env(cfg, mp), ob.OracleEnv(cfg, mp)
    dev.set_scenario_lists(probs)
    ora.set_scenario_lists(probs)
    dev.env.buffer(capi.BUF_DONE).fill_(1)
    ora.get(capi.BUF_DONE, copy=False)[:] = 1
    dev.auto_reset(9, 0, 0, capi.SCENARIO_LISTS)
    ora.auto_reset(9, 0, 0, capi.SCENARIO_LISTS)
    _compare_all(dev, ora, "initial reset")
    rng = np.random.default_rng(12)
    acts = np.stack([rng.uniform(0.3, 1.2, (T, B, N)), rng.uniform(-0.4, 0.4, (T, B, N))], axis=-1).astype(np.float32)
    full = agent = 0
    for t in range(T // 2):
        dev.step_autoreset(acts[t], 9, t + 1, 0, capi.SCENARIO_LISTS)
        sid_before = ora.get(capi.BUF_PATH)[..., 1].copy()
        ora.step(acts[t])
        done = ora.get(capi.BUF_DONE).astype(bool)
        req = ora.get(capi.BUF_COL_FLAGS)[..., 3].astype(bool) & ~done[:, None]
        ora.auto_reset(9, t + 1, 0, capi.SCENARIO_LISTS)
        _compare_all(dev, ora, f"step {t}")
        pa = ora.get(capi.BUF_PATH)
        assert (pa[..., 1] == pa[:, :1, 1]).all() and pa[..., 1].min() >= 1
        assert np.array_equal(pa[..., 1][~done], sid_before[~done])                # only a finished env redraws its sub-scenario
        full += int(done.sum())
        agent += int(req.sum())
    assert full > 0 and (agent > 0 or not testing)  # (per-agent requests within 12 steps: the colliders of testing mode)
    # the in-kernel step loop takes the lists as well
    a = torch.as_tensor(acts[T // 2:]).to(dev.env.device).contiguous()
    dev.env.step_autoreset_n(a, seed=9, counter0=100, path_first=0, path_count=capi.SCENARIO_LISTS)
    dev.env.sync()
    for t in range(T // 2, T):
        ora.step(acts[t])
        ora.auto_reset(9, 100 + t - T // 2, 0, capi.SCENARIO_LISTS)
    _compare_all(dev, ora, "after the step loop")
    if not testing:
        p2 = Parameters(n_agents=2, scenario_type="cpm_mixed", is_apply_mask=False, is_obs_noise=False, cpm_scenario_probabilities=probs)  # (the fixture's agent count)
        dev2 = _hip_env(make_config(p2, mp, 2048), mp)
        rdc.compare_mixed(rdc.sample_mixed(dev2, mp, rounds=2, probabilities=probs))
        dev2.close()
    dev.close()
    ora.close()


@pytest.mark.parametrize("scen,N,B,mtv,rew,dt,testing", [
    ("cpm_entire", 16, 200, False, "distance", 0.05, False),       # whole tiles of 4 envs with 0..4 finished envs each
    ("cpm_entire", 5, 33, True, "ttc_sparse", 0.1, False),         # ragged tile
    ("cpm_entire", 8, 24, True, "sparse", 0.1, True),              # testing mode: per-agent requests inside the fused tail
    ("intersection_1", 4, 40, False, "distance", 0.1, False),      # entry / exit requests
])
def test_fused_step_autoreset_equals_step_then_auto_reset(scen, N, B, mtv, rew, dt, testing):
    """sigmaenv_step_autoreset == sigmaenv_step; sigmaenv_auto_reset -- every buffer bit-identical after every step, and the slab
    row written by the fused launch holds the terminal observation / reward / done flag of the step (HIP separate == oracle is
    covered above, so the fused launch is tied to the oracle through it)."""
    import torch
    from sigmarl_amd.shard import slab_width, unpack_slab

    p = Parameters(n_agents=N, scenario_type=scen, is_use_mtv_distance=mtv, rew_method=rew, dt=dt, is_testing_mode=testing,
                   is_apply_mask=False, is_obs_noise=False, max_steps=9)
    mp = load_map(scen)
    cfg = make_config(p, mp, B)
    pf, pc = mp.list_first[0], mp.list_count[0]
    sep, fus = _hip_env(cfg, mp), _hip_env(cfg, mp)
    for d in (sep, fus):
        d.env.buffer(capi.BUF_DONE).fill_(1)
        d.auto_reset(5, 0, pf, pc)
    W = slab_width(N, fus.env.D)
    rng = np.random.default_rng(7)
    total_done = 0
    for t in range(14):
        act = np.stack([rng.uniform(-0.2, 1.3, (B, N)), rng.uniform(-0.7, 0.7, (B, N))], axis=-1).astype(np.float32)
        if t % 3 == 2:
            act = np.stack([rng.uniform(0.0, 0.3, (B, N)), rng.uniform(-0.05, 0.05, (B, N))], axis=-1).astype(np.float32)
        sep.step(act)
        term = {w: sep.get(w) for w in (capi.BUF_OBS, capi.BUF_REWARD, capi.BUF_DONE)}
        total_done += int(term[capi.BUF_DONE].sum())
        sep.auto_reset(5, t + 1, pf, pc)
        row = torch.full((B, W), float("nan"), device="cuda")
        fus.env.set_slab(row)
        fus.step_autoreset(act, 5, t + 1, pf, pc)
        obs, r, dn = unpack_slab(row, N, fus.env.D)
        assert np.array_equal(obs.cpu().numpy(), term[capi.BUF_OBS]) and np.array_equal(r.cpu().numpy(), term[capi.BUF_REWARD])
        assert np.array_equal(dn.cpu().numpy(), term[capi.BUF_DONE].astype(bool))
        for w in INT_BUFS + FLT_BUFS:
            a, b = sep.get(w), fus.get(w)
            assert a.tobytes() == b.tobytes(), f"step {t}: buffer {w} differs between the fused and the separate launches"
    assert total_done > 0
    sep.close()
    fus.close()


ALL_MAPS = ["cpm_mixed", "interchange_1", "interchange_2", "interchange_3", "intersection_2", "intersection_3", "intersection_4",
            "intersection_5", "intersection_6", "intersection_7", "intersection_8", "on_ramp_2_multilane", "roundabout_1", "roundabout_2"]


@pytest.mark.parametrize("scen", ALL_MAPS)
def test_every_shipped_map_hip_vs_oracle(scen):
    """Every scenario table the package ships (the three used above are covered there): a short seeded episode with device-side
    resets through the HIP path and the oracle, every buffer compared after every call."""
    N, B = 3, 10
    p = Parameters(n_agents=N, scenario_type=scen, is_use_mtv_distance=(len(scen) % 2 == 0), rew_method="distance_sparse", dt=0.1,
                   is_apply_mask=False, is_obs_noise=False, max_steps=7)
    mp = load_map(scen)
    cfg = make_config(p, mp, B)
    dev, ora = _hip_env(cfg, mp), ob.OracleEnv(cfg, mp)
    dev.env.buffer(capi.BUF_DONE).fill_(1)
    ora.get(capi.BUF_DONE, copy=False)[:] = 1
    lid = 1 if scen == "cpm_mixed" else 0
    pf, pc = mp.list_first[lid], mp.list_count[lid]
    dev.auto_reset(21, 0, pf, pc)
    ora.auto_reset(21, 0, pf, pc)
    _compare_all(dev, ora, f"{scen} initial reset")
    rng = np.random.default_rng(len(scen))
    n_diff = 0
    for t in range(10):
        act = np.stack([rng.uniform(0.0, 1.2, (B, N)), rng.uniform(-0.5, 0.5, (B, N))], axis=-1).astype(np.float32)
        dev.step(act)
        ora.step(act)
        n_diff += _compare_all(dev, ora, f"{scen} step {t}")
        dev.auto_reset(21, t + 1, pf, pc)
        ora.auto_reset(21, t + 1, pf, pc)
        n_diff += _compare_all(dev, ora, f"{scen} reset {t}")
    assert n_diff <= 16
    dev.close()
    ora.close()


def test_sixty_four_agents_one_env_per_workgroup():
    """N = 64: the largest agent count of the layout (one env fills the 64 agent slots of a workgroup, 64-bit agent masks)."""
    scen, N, B = "cpm_entire", 64, 6
    p = Parameters(n_agents=N, scenario_type=scen, is_use_mtv_distance=False, rew_method="distance", is_apply_mask=False, is_obs_noise=False,
                   max_steps=6)
    mp = load_map(scen)
    cfg = make_config(p, mp, B)
    dev, ora = _hip_env(cfg, mp), ob.OracleEnv(cfg, mp)
    dev.env.buffer(capi.BUF_DONE).fill_(1)
    ora.get(capi.BUF_DONE, copy=False)[:] = 1
    pf, pc = mp.list_first[0], mp.list_count[0]
    dev.auto_reset(4, 0, pf, pc)
    ora.auto_reset(4, 0, pf, pc)
    _compare_all(dev, ora, "N=64 initial reset")
    rng = np.random.default_rng(64)
    for t in range(6):
        act = np.stack([rng.uniform(0.0, 1.0, (B, N)), rng.uniform(-0.3, 0.3, (B, N))], axis=-1).astype(np.float32)
        dev.step_autoreset(act, 4, t + 1, pf, pc)
        ora.step(act)
        ora.auto_reset(4, t + 1, pf, pc)
        _compare_all(dev, ora, f"N=64 fused step {t}")
    dev.close()
    ora.close()


def test_compiled_custom_map_runs_through_both_paths():
    """A table compiled by sigmarl_amd.mapc (not one of the shipped reference-parser outputs) drives the HIP path and the oracle:
    interchange_2 compiled with a different lane width (boundaries and coordinates shift), seeded episode with device-side resets."""
    from sigmarl_amd import mapc
    from sigmarl_amd.maps import MapTable

    mp = MapTable("interchange_2", table=mapc.compile_scenario("interchange_2", lane_width=0.3))
    assert not np.array_equal(mp.left, load_map("interchange_2").left)
    N, B = 4, 12
    p = Parameters(n_agents=N, scenario_type="interchange_2", is_use_mtv_distance=False, rew_method="distance", dt=0.1, is_apply_mask=False,
                   is_obs_noise=False, max_steps=8)
    cfg = make_config(p, mp, B)
    dev, ora = _hip_env(cfg, mp), ob.OracleEnv(cfg, mp)
    dev.env.buffer(capi.BUF_DONE).fill_(1)
    ora.get(capi.BUF_DONE, copy=False)[:] = 1
    pf, pc = mp.list_first[0], mp.list_count[0]
    dev.auto_reset(2, 0, pf, pc)
    ora.auto_reset(2, 0, pf, pc)
    rng = np.random.default_rng(5)
    for t in range(10):
        act = np.stack([rng.uniform(0.0, 1.2, (B, N)), rng.uniform(-0.5, 0.5, (B, N))], axis=-1).astype(np.float32)
        dev.step_autoreset(act, 2, t + 1, pf, pc)
        ora.step(act)
        ora.auto_reset(2, t + 1, pf, pc)
        _compare_all(dev, ora, f"compiled map step {t}")
    dev.close()
    ora.close()


@pytest.mark.parametrize("scen,N,B,T,mtv,rew,testing", [
    ("intersection_1", 4, 768, 120, False, "distance", False),   # 4 x 4 tiles (fixed-shape instantiation), entry / exit requests
    ("cpm_entire", 8, 512, 100, True, "ttc", True),              # 8 x 2 tiles, testing mode: colliders re-placed one by one
    ("cpm_entire", 32, 96, 60, False, "distance_sparse", False),  # 32 x 1 tiles
    ("on_ramp_1", 6, 300, 100, True, "distance", False),         # generic instantiation, ragged tiles
])
def test_soak_other_tile_shapes(scen, N, B, T, mtv, rew, testing):
    """The one-launch path at the other tile shapes (fixed-shape instantiations 4 x 4, 8 x 2, 32 x 1 and the generic kernel) against the
    oracle over long mixed-action runs, every buffer after every step.  At these batch sizes the library's own rule gives one env per wavefront, so the
    4 x 4 / 8 x 2 / 32 x 1 tiles are asked for through cfg.envs_per_group, and every row asserts with launch_shape() the instantiation it names."""
    p = Parameters(n_agents=N, scenario_type=scen, is_use_mtv_distance=mtv, rew_method=rew, dt=0.05, is_apply_mask=False, is_obs_noise=False, max_steps=30,
                   is_testing_mode=testing)
    mp = load_map(scen)
    cfg = make_config(p, mp, B)
    wave_g = {4: 4, 8: 2, 32: 1}.get(N, 0)
    cfg.envs_per_group = wave_g
    dev, ora = _hip_env(cfg, mp), ob.OracleEnv(cfg, mp)
    ls = dev.env.launch_shape()
    print(f"soak {scen} N={N}: launch_shape {ls}")
    if wave_g:
        assert (ls["wave_G"], ls["wave_spec"], ls["instantiation"]) == (wave_g, N * 256 + wave_g, (True, True, N, wave_g, False, False)), ls
    else:  # the generic kernel
        assert (ls["wave_spec"], ls["instantiation"]) == (0, (True, 2 * ls["wave_G"] * N <= 64, 0, 0, False, False)), ls
    dev.env.buffer(capi.BUF_DONE).fill_(1)
    ora.get(capi.BUF_DONE, copy=False)[:] = 1
    pf, pc = mp.list_first[0], mp.list_count[0]
    dev.auto_reset(23, 0, pf, pc)
    ora.auto_reset(23, 0, pf, pc)
    rng = np.random.default_rng(99)
    n_diff = n_done = n_req = 0
    for t in range(T):
        mode = t % 3
        if mode == 0:
            act = np.stack([rng.uniform(0, 1, (B, N)), rng.uniform(-0.25, 0.25, (B, N))], axis=-1)
        elif mode == 1:
            act = np.stack([rng.uniform(0.1, 0.4, (B, N)), rng.uniform(-0.03, 0.03, (B, N))], axis=-1)
        else:
            act = np.stack([rng.uniform(-0.5, 1.6, (B, N)), rng.uniform(-0.9, 0.9, (B, N))], axis=-1)
        act = act.astype(np.float32)
        dev.step_autoreset(act, 23, t + 1, pf, pc)
        ora.step(act)
        n_done += int(ora.get(capi.BUF_DONE).sum())
        n_req += int(ora.get(capi.BUF_COL_FLAGS)[..., 3].sum())
        ora.auto_reset(23, t + 1, pf, pc)
        n_diff += _compare_all(dev, ora, f"soak {scen} N={N} step {t}")
    assert n_done > B // 2
    print(f"soak {scen} N={N}: {n_done} finished episodes, {n_req} per-agent requests, differing non-observation fp32 words: {n_diff}")
    assert n_diff <= 64
    dev.close()
    ora.close()


@pytest.mark.parametrize("mtv,rew", [(False, "distance"), (True, "ttc_sparse")])
def test_soak_fused_launch_vs_oracle(mtv, rew):
    """2.4 million agent-steps through the ONE-launch path (fused step + record + device resets) against the brute-force oracle, every
    buffer compared after every step: episodes of every length up to max_steps, collisions of both kinds, agents far off their path
    (two-level candidate search), stale-corner lanes, reset storms.  Masks / indices bit-exact, fp32 within 1e-5, and -- since both sides
    share the arithmetic contract -- (almost) no differing non-observation word at all."""
    scen, N, B, T = "cpm_entire", 16, 512, 300
    p = Parameters(n_agents=N, scenario_type=scen, is_use_mtv_distance=mtv, rew_method=rew, dt=0.05, is_apply_mask=False, is_obs_noise=False,
                   max_steps=40)
    mp = load_map(scen)
    cfg = make_config(p, mp, B)
    dev, ora = _hip_env(cfg, mp), ob.OracleEnv(cfg, mp)
    dev.env.buffer(capi.BUF_DONE).fill_(1)
    ora.get(capi.BUF_DONE, copy=False)[:] = 1
    pf, pc = mp.list_first[0], mp.list_count[0]
    dev.auto_reset(17, 0, pf, pc)
    ora.auto_reset(17, 0, pf, pc)
    rng = np.random.default_rng(2024)
    n_diff = n_done = 0
    for t in range(T):
        mode = t % 4
        if mode == 0:    # bench-like
            act = np.stack([rng.uniform(0, 1, (B, N)), rng.uniform(-0.25, 0.25, (B, N))], axis=-1)
        elif mode == 1:  # careful drivers: long episodes, max_steps terminations
            act = np.stack([rng.uniform(0.1, 0.4, (B, N)), rng.uniform(-0.03, 0.03, (B, N))], axis=-1)
        elif mode == 2:  # beyond the clamps, hard steering: off the road quickly
            act = np.stack([rng.uniform(-0.5, 1.6, (B, N)), rng.uniform(-0.9, 0.9, (B, N))], axis=-1)
        else:            # stop and go
            act = np.stack([rng.choice([0.0, 1.0], (B, N)), rng.uniform(-0.1, 0.1, (B, N))], axis=-1)
        act = act.astype(np.float32)
        dev.step_autoreset(act, 17, t + 1, pf, pc)
        ora.step(act)
        n_done += int(ora.get(capi.BUF_DONE).sum())
        ora.auto_reset(17, t + 1, pf, pc)
        n_diff += _compare_all(dev, ora, f"soak step {t}")
    assert n_done > B  # every env finished more than once on average
    print(f"soak mtv={mtv}: {n_done} finished episodes, differing non-observation fp32 words: {n_diff}")
    assert n_diff <= 64
    dev.close()
    ora.close()


@pytest.mark.parametrize("scen,N", [("pseudo_distance_example", 1), ("cpm_entire", 1), ("cpm_entire", 3)])
def test_single_agent_and_odd_observation_width(scen, N):
    """N = 1: no neighbours (K = 0, obs_dim = 10: the scalar row-store path), 64 envs per workgroup, no agent pairs at all."""
    B = 9
    p = Parameters(n_agents=N, scenario_type=scen, is_use_mtv_distance=False, rew_method="distance", dt=0.1, is_apply_mask=False, is_obs_noise=False,
                   max_steps=6, n_nearing_agents_observed=min(2, N - 1))
    mp = load_map(scen)
    cfg = make_config(p, mp, B)
    dev, ora = _hip_env(cfg, mp), ob.OracleEnv(cfg, mp)
    dev.env.buffer(capi.BUF_DONE).fill_(1)
    ora.get(capi.BUF_DONE, copy=False)[:] = 1
    pf, pc = mp.list_first[0], mp.list_count[0]
    dev.auto_reset(2, 0, pf, pc)
    ora.auto_reset(2, 0, pf, pc)
    rng = np.random.default_rng(1)
    for t in range(10):
        act = np.stack([rng.uniform(0, 1.2, (B, N)), rng.uniform(-0.5, 0.5, (B, N))], -1).astype(np.float32)
        dev.step_autoreset(act, 2, t + 1, pf, pc)
        ora.step(act)
        ora.auto_reset(2, t + 1, pf, pc)
        _compare_all(dev, ora, f"{scen} N={N} step {t}")
    assert dev.env.D == 4 + 6 + 11 * min(2, N - 1)
    dev.close()
    ora.close()


OBS_VARIANTS = [
    dict(is_obs_steering=True),
    dict(is_observe_ref_path_other_agents=True, is_apply_mask=True),
    dict(is_observe_vertices=False),
    dict(is_observe_distance_to_agents=False, is_observe_distance_to_center_line=False),
    dict(is_obs_steering=True, is_observe_ref_path_other_agents=True, is_observe_vertices=False, is_observe_distance_to_agents=False,
         is_observe_distance_to_center_line=False, is_apply_mask=True),
    dict(is_ego_view=False),
    dict(is_observe_distance_to_boundaries=False),
    dict(is_observe_distance_to_boundaries=False, is_ego_view=False, is_obs_steering=True),
    dict(is_ego_view=False, is_obs_steering=True, is_observe_vertices=False, is_observe_ref_path_other_agents=True),
    dict(is_using_opponent_modeling=True),
    dict(is_using_opponent_modeling=True, is_ego_view=False, is_obs_steering=True),
    dict(n_points_short_term=5, is_observe_ref_path_other_agents=True, is_obs_steering=True),        # the switches in another build variant (libsigmaenv_ns5.so)
    dict(n_points_short_term=2, is_ego_view=False, is_observe_distance_to_boundaries=False, is_using_opponent_modeling=True),
    # full observation (is_partial_observation=False; bird view only): ALL agents' features in every row, observation_provider_rt.py:756-851
    dict(is_ego_view=False, is_partial_observation=False),
    dict(is_ego_view=False, is_partial_observation=False, is_observe_vertices=False, is_obs_steering=True, is_observe_ref_path_other_agents=True, is_apply_mask=True),
    dict(is_ego_view=False, is_partial_observation=False, is_observe_distance_to_agents=False, is_observe_distance_to_boundaries=False, is_using_opponent_modeling=True,
         n_nearing_agents_observed=4),
]


@pytest.mark.parametrize("kw", OBS_VARIANTS)
def test_observation_variants_hip_vs_oracle(kw):
    """Non-default observation switches (capi.OBS_*, observation_provider_rt.py:803-925): the public observation buffer has
    sigmaenv_obs_dim_full columns and equals the oracle's row (pinned on the reference's trajectories, tests/golden) through steps, device-side
    resets and sigmaenv_observe; every other buffer is unaffected; the rollout record carries the same row."""
    import torch

    N, B = 8, 40
    base = dict(n_agents=N, scenario_type="cpm_entire", is_use_mtv_distance=False, rew_method="distance", dt=0.05, is_apply_mask=False, is_obs_noise=False,
                max_steps=9)
    base.update(kw)
    p = Parameters(**base)
    mp = load_map("cpm_entire")
    cfg = make_config(p, mp, B)
    assert cfg.obs_flags != 0
    dev, ora = _hip_env(cfg, mp), ob.OracleEnv(cfg, mp)
    D = capi.obs_dim(cfg.n_nearing, cfg.obs_flags, p.n_points_short_term, N)
    assert dev.D == D == ora.D and dev.env.lib.obs_dim_full(N, cfg.n_nearing, cfg.obs_flags) == D and D != 32
    if not (cfg.obs_flags & capi.OBS_FULL):
        assert dev.env.lib.obs_dim_ex(cfg.n_nearing, cfg.obs_flags) == D
    dev.env.buffer(capi.BUF_DONE).fill_(1)
    ora.get(capi.BUF_DONE, copy=False)[:] = 1
    pf, pc = mp.list_first[0], mp.list_count[0]
    dev.auto_reset(7, 0, pf, pc)
    ora.auto_reset(7, 0, pf, pc)
    _compare_all(dev, ora, "after initial reset")
    rng = np.random.default_rng(77)
    for t in range(8):
        act = np.stack([rng.uniform(-0.2, 1.3, (B, N)), rng.uniform(-0.7, 0.7, (B, N))], axis=-1).astype(np.float32)
        dev.step(act)
        ora.step(act)
        _compare_all(dev, ora, f"step {t}")
        assert dev.get(capi.BUF_OBS).shape == (B, N, D)
        dev.auto_reset(7, t + 1, pf, pc)
        ora.auto_reset(7, t + 1, pf, pc)
        _compare_all(dev, ora, f"reset after step {t}")
    dev.env.observe()
    ora.observe() if hasattr(ora, "observe") else None
    _compare_all(dev, ora, "observe")
    slab = torch.full((B, N * (D + 1) + 1), float("nan"), device="cuda")
    dev.env.set_slab(slab)
    act = np.stack([rng.uniform(0, 1, (B, N)), rng.uniform(-0.3, 0.3, (B, N))], axis=-1).astype(np.float32)
    dev.step(act)
    ora.step(act)
    got = slab[:, : N * D].reshape(B, N, D).cpu().numpy()
    assert np.array_equal(got, dev.get(capi.BUF_OBS)) and np.abs(got - ora.get(capi.BUF_OBS)).max() <= 1e-5
    dev.close()
    ora.close()


def test_full_observation_16_agents_hip_vs_oracle_and_refusals():
    """SURVEY row a12, is_partial_observation=False at the metric's agent count (16 agents, sensor noise on): the row is 14 + 16 x (8 + 2 + 16) = 430 wide,
    HIP == oracle on every buffer through steps and device-side resets (the oracle is pinned on four reference trajectories, tests/golden/traj_*full_bird*),
    its distance block is zero before the noise, SIGMAENV_BUF_NEARING stays zero; the shapes the reference's reshape refuses are refused."""
    N, B = 16, 48
    p = Parameters(n_agents=N, scenario_type="cpm_entire", is_use_mtv_distance=True, rew_method="ttc", dt=0.05, is_apply_mask=True, is_obs_noise=True,
                   obs_noise_level=0.05, random_seed=11, max_steps=9, is_ego_view=False, is_partial_observation=False)
    mp = load_map("cpm_entire")
    cfg = make_config(p, mp, B)
    assert cfg.obs_flags & capi.OBS_FULL
    dev, ora = _hip_env(cfg, mp), ob.OracleEnv(cfg, mp)
    assert dev.D == ora.D == 5 + 6 + 3 + N * (8 + 2 + N) == 430
    dev.env.buffer(capi.BUF_DONE).fill_(1)
    ora.get(capi.BUF_DONE, copy=False)[:] = 1
    pf, pc = mp.list_first[0], mp.list_count[0]
    dev.auto_reset(4, 0, pf, pc)
    ora.auto_reset(4, 0, pf, pc)
    _compare_all(dev, ora, "after initial reset")
    rng = np.random.default_rng(8)
    for t in range(8):
        act = np.stack([rng.uniform(-0.2, 1.3, (B, N)), rng.uniform(-0.7, 0.7, (B, N))], axis=-1).astype(np.float32)
        dev.step(act)
        ora.step(act)
        _compare_all(dev, ora, f"step {t}")
        dev.auto_reset(4, t + 1, pf, pc)
        ora.auto_reset(4, t + 1, pf, pc)
        _compare_all(dev, ora, f"reset after step {t}")
    obs = dev.get(capi.BUF_OBS)
    assert not dev.get(capi.BUF_NEARING).any()
    others = obs[..., 14:].reshape(B, N, 2, -1)          # K = 2 chunks of [8 agents' vertices | their velocities | 8 rows of the zeroed distance matrix]
    dist = others[..., 8 * 8 + 8 * 2:]
    assert dist.shape[-1] == 8 * N and (dist >= 0).all() and (dist < cfg.obs_noise_level).all()   # zero + noise in [0, level)
    dev.close()
    ora.close()
    for kw in (dict(is_ego_view=True), dict(is_ego_view=False, n_agents=5, n_nearing_agents_observed=2), dict(is_ego_view=False, n_agents=6, n_nearing_agents_observed=4, is_obs_steering=True),
               dict(is_ego_view=False, n_agents=6, n_nearing_agents_observed=4)):  # (vertices 48, velocities 12, distances 36 all split into 4 chunks -- the reference still raises: it reshapes
                                                                                   # the six rotations / lengths / widths / steering angles to [B, 4, -1] whether or not the row uses them)
        with pytest.raises(NotImplementedError):
            make_config(Parameters(**dict(dict(n_agents=4, scenario_type="cpm_entire", is_partial_observation=False), **kw)), mp, 4)
    lib = capi.load_library()
    assert lib.obs_dim_full(5, 2, capi.OBS_FULL | capi.OBS_BIRD_VIEW) < 0 and lib.obs_dim_full(4, 2, capi.OBS_FULL) < 0
    assert lib.obs_dim_full(4, 2, capi.OBS_FULL | capi.OBS_BIRD_VIEW) == 70 and lib.obs_dim_full(6, 4, capi.OBS_FULL | capi.OBS_BIRD_VIEW) < 0


@pytest.mark.parametrize("noise", [False, True])
def test_opponent_modeling_placeholders_and_fill(noise):
    """is_using_opponent_modeling: the row ends with n_nearing x 2 placeholder columns (observation_provider_rt.py:606-611; zero, or pure sensor noise when
    is_obs_noise -- the pad precedes the noise), and sigmaenv_opponent_fill gathers the tentative actions of the observed neighbours into them exactly as
    opponent_modeling's loops do (helper_training.py:1117-1137, restated in numpy here).  HIP == oracle on every buffer before and after the fill."""
    N, B, K = 8, 64, 2
    p = Parameters(n_agents=N, scenario_type="cpm_entire", is_use_mtv_distance=False, rew_method="distance", dt=0.05, is_obs_noise=noise, max_steps=9,
                   is_using_opponent_modeling=True)
    mp = load_map("cpm_entire")
    cfg = make_config(p, mp, B)
    dev, ora = _hip_env(cfg, mp), ob.OracleEnv(cfg, mp)
    D = capi.obs_dim(K, cfg.obs_flags)
    assert D == 32 + 2 * K == dev.D == ora.D
    dev.env.buffer(capi.BUF_DONE).fill_(1)
    ora.get(capi.BUF_DONE, copy=False)[:] = 1
    pf, pc = mp.list_first[0], mp.list_count[0]
    dev.auto_reset(3, 0, pf, pc)
    ora.auto_reset(3, 0, pf, pc)
    rng = np.random.default_rng(5)
    for t in range(6):
        act = np.stack([rng.uniform(0, 1.0, (B, N)), rng.uniform(-0.4, 0.4, (B, N))], axis=-1).astype(np.float32)
        dev.step(act)
        ora.step(act)
        _compare_all(dev, ora, f"step {t}")
        obs = dev.get(capi.BUF_OBS)
        tail = obs[..., D - 2 * K:]
        if noise:
            assert (tail >= 0).all() and (tail < cfg.obs_noise_level).all() and tail.std() > 0
        else:
            assert (tail == 0).all()
        tentative = rng.normal(size=(B, N, 2)).astype(np.float32)
        dev.opponent_fill(tentative)
        ora.opponent_fill(tentative)
        _compare_all(dev, ora, f"fill after step {t}")
        near = dev.get(capi.BUF_NEARING).astype(np.int64)
        want = obs.copy()
        for ego in range(N):               # the reference's loops
            for j in range(K):
                sur = near[:, ego, j]
                start = -(K - j) * 2
                end = start + 2
                want[:, ego, start:(end if end != 0 else None)] = tentative[np.arange(B), sur]
        np.testing.assert_array_equal(dev.get(capi.BUF_OBS), want)
        dev.auto_reset(3, t + 1, pf, pc)
        ora.auto_reset(3, t + 1, pf, pc)
    with pytest.raises(RuntimeError):      # no placeholder columns in the default layout
        plain = _hip_env(make_config(Parameters(n_agents=N, scenario_type="cpm_entire", is_obs_noise=False), mp, 4), mp)
        try:
            plain.opponent_fill(np.zeros((4, N, 2), np.float32))
        finally:
            plain.close()
    dev.close()
    ora.close()


@pytest.mark.parametrize("scen,N", [("roundabout_2", 6), ("intersection_4", 8), ("cpm_entire", 8)])
def test_birdview_lanelet_mask_hip_vs_oracle(scen, N):
    """Bird view + is_apply_mask: the lanelet-relation mask (current lanelet of every vehicle from the map's lanelet centre lines, neighbour table of the
    map's parser; observation_provider_rt.py:577-665, map_manager.py:41-118) -- HIP == oracle on seeded episodes, and on the OSM maps the mask really
    masks neighbours the distance criterion alone would show.  (The oracle is pinned to the reference on three goldens, tests/test_oracle_golden.py.)"""
    B = 40
    p = Parameters(n_agents=N, scenario_type=scen, is_use_mtv_distance=False, rew_method="distance", dt=0.1, is_ego_view=False, is_apply_mask=True,
                   is_obs_noise=False, max_steps=9)
    mp = load_map(scen)
    cfg = make_config(p, mp, B)
    dev, ora = _hip_env(cfg, mp), ob.OracleEnv(cfg, mp)
    cfg_nomask = make_config(Parameters(n_agents=N, scenario_type=scen, is_use_mtv_distance=False, rew_method="distance", dt=0.1, is_ego_view=False,
                                        is_apply_mask=False, is_obs_noise=False, max_steps=9), mp, B)
    plain = ob.OracleEnv(cfg_nomask, mp)
    for e in (dev, ora, plain):
        if e is dev:
            e.env.buffer(capi.BUF_DONE).fill_(1)
        else:
            e.get(capi.BUF_DONE, copy=False)[:] = 1
        e.auto_reset(5, 0, mp.list_first[0], mp.list_count[0])
    rng = np.random.default_rng(3)
    masked_more = 0
    for t in range(10):
        act = np.stack([rng.uniform(0.0, 1.0, (B, N)), rng.uniform(-0.4, 0.4, (B, N))], axis=-1).astype(np.float32)
        for e in (dev, ora, plain):
            e.step(act)
        _compare_all(dev, ora, f"{scen} bird view + mask, step {t}")
        far = ora.get(capi.BUF_DIST_AGENTS) >= cfg.distance_mask_agents
        near_idx = ora.get(capi.BUF_NEARING).astype(np.int64)
        not_far = ~np.take_along_axis(far, near_idx, axis=-1)                      # neighbours the distance criterion leaves visible ...
        blk_m = ora.get(capi.BUF_OBS)[..., -2 * 11:].reshape(B, N, 2, 11)
        blk_p = plain.get(capi.BUF_OBS)[..., -2 * 11:].reshape(B, N, 2, 11)
        masked_more += int((not_far & (blk_m[..., 10] == 1.0) & (blk_p[..., 10] != 1.0)).sum())  # ... that the lanelet relation masks
        for e in (dev, ora, plain):
            e.auto_reset(5, t + 1, mp.list_first[0], mp.list_count[0])
    assert (masked_more > 0) == (scen != "cpm_entire"), masked_more
    for e in (dev, ora, plain):
        e.close()
