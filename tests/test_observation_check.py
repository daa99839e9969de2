"""tests/observation_check.py on the host (no GPU):
a. the oracle's BUF_OBS against the float64 restatement on the oracle's own buffers within bound(form="reference") -- validates the layout restatement against the
   side that is pinned to the reference's goldens, on every observation variant, three maps, mask / mtv on and off, noise on; rows after a full reset, after
   steps and after per-agent resets; no element left out;
b. a float32 twin of the KERNEL's formulas (rotation form, reciprocals) on the same buffers within the kernel's bound, every ratio <= 1 -- validates the derived
   constants without a GPU;
c. planted defects in the twin that pass the old flat 1e-5 and must fail ``compare``;  d. large defects, which must fail too.
"""
import functools

import numpy as np
import pytest

import observation_check as oc
import oracle_binding as ob
from sigmarl_amd import capi
from sigmarl_amd.maps import load_map
from sigmarl_amd.params import Parameters, make_config
from test_gpu_parity import OBS_VARIANTS

f32 = np.float32


# ---- the float32 twin of observe_tile_default / observe_tile_variant ---------------------------------------------------------------------------------------------------
def _cr(fn, x):
    """correctly rounded fp32 cos / sin of an fp32 argument"""
    return fn(np.asarray(x, f32).astype(np.float64)).astype(f32)


def _ulps(x, k):
    for _ in range(k):
        x = np.nextafter(x, f32(np.inf))
    return x


def _norm2(x, y):
    """sqrtf(fmaf(y, y, x * x))"""
    xx = (x * x).astype(f32)
    return np.sqrt((y.astype(np.float64) * y.astype(np.float64) + xx.astype(np.float64)).astype(f32))


class Twin32:
    """The arithmetic interface of observation_check.assemble in numpy float32, operation by operation as the kernels (sigmaenv.hip) have it; ``defect`` plants one."""

    def __init__(self, cfg, defect=None, prev=None, lane_width64=None):
        self.defect = defect
        self.prev = prev  # (x, y, moved-mask) of the agents' previous positions
        n = {k: f32(v) for k, v in oc.normalisers(cfg).items()}
        if defect == "n_pos_2e-6":
            n["pos"] = f32(float(n["pos"]) * (1.0 + 2e-6))
        if defect == "n_dl_unrounded":
            n["dl"] = f32(lane_width64 * 3.0)
        self.n = n
        self.r = {k: f32(1.0) / v for k, v in n.items()}

    def const(self, value, like):
        return np.full(like.shape, f32(value)), 0.0, oc.EXACT

    def scaled(self, x, which):
        if self.defect == "r_pos_for_distance" and which == "dl":
            which = "pos"
        return np.asarray(x, f32) * self.r[which], 0.0, oc.SCALED

    def scaled_const(self, x, which, like):
        return self.scaled(np.full(like.shape, f32(x)), which)

    def speed(self, vx, vy):
        return _norm2(vx, vy) * self.r["v"], 0.0, oc.SPEED

    def _cs(self, psi):
        c, s = _cr(np.cos, psi), _cr(np.sin, psi)
        if self.defect == "trig_4ulp":
            c, s = _ulps(c, 4), _ulps(s, 4)
        return c, s

    def ego(self, tx, ty, px, py, psi):
        if self.defect == "prev_pos":
            px, py = np.where(self.prev[2], self.prev[0], px), np.where(self.prev[2], self.prev[1], py)
        dx, dy = tx - px, ty - py
        c, s = self._cs(psi)
        ox, oy = (dx * c + dy * s) * self.r["pos"], (dy * c - dx * s) * self.r["pos"]
        if self.defect == "xy_exchanged":
            ox, oy = oy, ox
        return (ox, 0.0, oc.EGO), (oy, 0.0, oc.EGO)

    def relvel(self, vx, vy, psi_j, psi_i):
        va = _norm2(vx, vy)
        (cj, sj), (ci, si) = self._cs(psi_j), self._cs(psi_i)
        cr, sr = cj * ci + sj * si, sj * ci - cj * si
        return ((va * cr) * self.r["v"], 0.0, oc.RELVEL), ((va * sr) * self.r["v"], 0.0, oc.RELVEL)

    def _wrap(self, a, two_pi=f32(oc.TWO_PI32)):
        m = np.fmod(a, two_pi)
        m = np.where(m < 0, m + two_pi, m)
        return np.where(m > f32(oc.PI32), m - two_pi, m)

    def angle(self, a):
        return self._wrap(np.asarray(a, f32)) * self.r["rot"], 0.0, oc.ANGLE

    def relangle(self, psi_j, psi_i):
        a = np.asarray(psi_j, f32) - np.asarray(psi_i, f32)
        if self.defect == "wrap_2pi_f64":
            m = self._wrap(a.astype(np.float64), 2.0 * np.pi).astype(f32)
        else:
            m = self._wrap(a)
        return m * self.r["rot"], 0.0, oc.ANGLE


def twin_rows(cfg, mp, bufs, defect=None, **kw):
    if defect == "vertices_swapped":
        bufs = dict(bufs)
        v = bufs[capi.BUF_VERTICES].copy()
        v[..., [0, 1], :] = v[..., [1, 0], :]
        bufs[capi.BUF_VERTICES] = v
    cols = oc.assemble(cfg, mp, bufs, Twin32(cfg, defect, **kw))
    shape = bufs[capi.BUF_STATE].shape[:2]
    rows = np.stack([np.broadcast_to(np.asarray(c[0]), shape) for c in cols], axis=-1)
    assert rows.dtype == f32
    nz = oc.noise_draws(cfg, bufs, rows.shape[-1])
    if nz is not None:
        draw = (nz / float(f32(cfg.obs_noise_level))).astype(f32)
        rows = rows + f32(cfg.obs_noise_level) * draw
    return rows


# ---- seeded runs of the oracle, each taken once -----------------------------------------------------------------------------------------------------------------------
def _params(scen="cpm_entire", N=8, **kw):
    base = dict(n_agents=N, scenario_type=scen, is_use_mtv_distance=False, rew_method="distance", dt=0.05, is_apply_mask=False, is_obs_noise=False, max_steps=9)
    base.update(kw)
    return Parameters(**base)


CASES = {f"variant{k}": (dict(kw), 8, 40) for k, kw in enumerate(OBS_VARIANTS)}
for _scen in ("cpm_entire", "intersection_1", "on_ramp_1"):
    for _mask in (False, True):
        for _mtv in (False, True):
            CASES[f"default-{_scen}-mask{int(_mask)}-mtv{int(_mtv)}"] = (dict(scenario_type=_scen, is_apply_mask=_mask, is_use_mtv_distance=_mtv, dt=0.1), 6 if _scen != "intersection_1" else 4, 24)
CASES["default-noise"] = (dict(is_obs_noise=True, obs_noise_level=0.05, random_seed=11, is_apply_mask=True), 8, 24)
CASES["default-testing"] = (dict(is_testing_mode=True, is_use_mtv_distance=True, rew_method="sparse", dt=0.1), 8, 24)   # per-agent resets of colliders
CASES["boundary-points-testing"] = (dict(is_observe_distance_to_boundaries=False, is_testing_mode=True, dt=0.1), 8, 24)
CASES["boundary-points-intersection"] = (dict(scenario_type="intersection_1", is_observe_distance_to_boundaries=False, dt=0.1), 4, 24)
CASES["full-16-noise"] = (dict(is_use_mtv_distance=True, rew_method="ttc", is_apply_mask=True, is_obs_noise=True, obs_noise_level=0.05, random_seed=11, is_ego_view=False,
                               is_partial_observation=False), 16, 8)
CASES["variant2-noise"] = (dict(is_observe_vertices=False, is_obs_steering=True, is_obs_noise=True, obs_noise_level=0.05, random_seed=3), 8, 24)


@functools.lru_cache(maxsize=None)
def snapshots(case):
    """[(tag, cfg, map, bufs)] of a seeded run of the oracle: after the full reset, after each of 6 steps, after each auto_reset (whole envs and single agents)"""
    kw, N, B = CASES[case]
    p = _params(N=N, **kw)
    mp = load_map(p.scenario_type)
    cfg = make_config(p, mp, B)
    ora = ob.OracleEnv(cfg, mp)
    ora.get(capi.BUF_DONE, copy=False)[:] = 1
    pf, pc = mp.list_first[0], mp.list_count[0]
    fr = oc.FreshTracker(B, N)
    fr.before_auto_reset(ora)
    ora.auto_reset(7, 0, pf, pc)
    out = [("full reset", cfg, mp, oc.read_bufs(ora, fr.fresh))]
    rng = np.random.default_rng(77)
    single = 0
    for t in range(6):
        act = np.stack([rng.uniform(-0.2, 1.3, (B, N)), rng.uniform(-0.7, 0.7, (B, N))], axis=-1).astype(f32)
        ora.step(act)
        fr.step()
        out.append((f"step {t}", cfg, mp, oc.read_bufs(ora, fr.fresh)))
        fr.before_auto_reset(ora)
        single += int((fr.fresh.any(axis=1) & ~fr.fresh.all(axis=1)).sum())
        ora.auto_reset(7, t + 1, pf, pc)
        out.append((f"reset after step {t}", cfg, mp, oc.read_bufs(ora, fr.fresh)))
    ora.close()
    return out, single


@pytest.mark.parametrize("case", list(CASES))
def test_oracle_rows_within_the_reference_bound_and_twin_within_the_kernel_bound(case):
    snaps, single = snapshots(case)
    if "testing" in case:
        assert single > 0  # per-agent resets happened: rows with fresh and stepped agents side by side
    worst_ref, worst_twin = {}, {}
    for tag, cfg, mp, bufs in snaps:
        res = oc.compare(bufs[capi.BUF_OBS], cfg, mp, bufs, form="reference")           # a.
        assert res["ok"] and res["excluded"] == 0, f"{case}, {tag}: oracle vs float64: {oc.report(res)}"
        twin = twin_rows(cfg, mp, bufs)                                                 # b.
        rt = oc.compare(twin, cfg, mp, bufs)
        assert rt["ok"] and rt["excluded"] == 0, f"{case}, {tag}: float32 twin vs float64: {oc.report(rt)}"
        assert np.abs(twin.astype(np.float64) - bufs[capi.BUF_OBS]).max() <= 1e-5 + (1.0 if rt["count"]["angle"] else 0.0)  # (the twin is the kernel: inside the old bar, up to a wrap)
        for name in oc.CLASSES:
            worst_ref[name] = max(worst_ref.get(name, 0.0), res["worst"][name])
            worst_twin[name] = max(worst_twin.get(name, 0.0), rt["worst"][name])
    print(f"{case}: oracle / reference bound {worst_ref}; twin / kernel bound {worst_twin}")


def test_the_oracle_does_not_meet_the_kernel_bound():
    """The reference's atan2 formulation needs its own, wider bound: on the same rows it exceeds the kernel's (by the angle's rounding seen through the other component)."""
    snaps, _ = snapshots("default-cpm_entire-mask0-mtv0")
    assert not all(oc.compare(b[capi.BUF_OBS], c, m, b)["ok"] for _, c, m, b in snaps)


# ---- c. / d. planted defects ---------------------------------------------------------------------------------------------------------------------------------------------
def _edge_snapshot(**kw):
    p = _params(N=6, **kw)
    mp = load_map("cpm_entire")
    cfg = make_config(p, mp, len(oc.EDGE_ENVS))
    ora = ob.OracleEnv(cfg, mp)
    ora.reset(*oc.injected_edge_states(cfg, mp), 1)
    ora.observe()
    bufs = oc.read_bufs(ora, np.ones((cfg.n_envs, 6), bool))
    ora.close()
    return cfg, mp, bufs


def _old_bar(rows, bufs):
    return np.abs(rows.astype(np.float64) - bufs[capi.BUF_OBS]).max() <= 1e-5


def _verdicts(defect, snaps, **kw):
    """(passes the flat 1e-5 against the oracle's rows on every snapshot, passes compare on every snapshot)"""
    old = new = True
    for _, cfg, mp, bufs in snaps:
        rows = twin_rows(cfg, mp, bufs, defect, **kw)
        old = old and _old_bar(rows, bufs)
        new = new and oc.compare(rows, cfg, mp, bufs)["ok"]
    return old, new


@pytest.mark.parametrize("defect", ["n_pos_2e-6", "trig_4ulp"])
def test_small_defects_pass_the_flat_bar_and_fail_the_bound(defect):
    snaps, _ = snapshots("default-cpm_entire-mask0-mtv0")
    assert _verdicts(None, snaps) == (True, True)
    assert _verdicts(defect, snaps) == (True, False)


def test_lane_width_times_three_in_float_cannot_change_a_bit_but_the_unrounded_parameter_can():
    """``lane_width * 3.0f`` in float: 3 has two significant bits, so the double product of a float and 3.0 is exact and both forms round the SAME real number
    once -- no lane_width exists for which they differ (asserted over a sweep, the shipped widths among it).  The neighbouring defect that does exist: the
    normaliser formed from the parameter BEFORE it is rounded to the config's float, (float)(lane_width_double * 3.0).  It is an ulp of n_dl off where it
    differs, passes the flat bar and must fail the bound."""
    lw = np.concatenate([np.random.default_rng(0).uniform(0.05, 4.0, 200000), [0.15, 0.2, 0.3, 3.5]]).astype(f32)
    assert np.array_equal(lw * f32(3.0), (lw.astype(np.float64) * 3.0).astype(f32))
    snaps, _ = snapshots("default-cpm_entire-mask0-mtv0")
    cfg, mp = snaps[0][1], snaps[0][2]
    lw64 = next(w for w in (mp.lane_width, 0.151, 0.1507, 0.1493, 0.1511) if f32(w * 3.0) != f32(float(f32(w)) * 3.0))
    snaps = [(t, _with_lane_width(c, lw64), m, b) for t, c, m, b in snaps]
    assert _verdicts(None, snaps)[1]
    old, new = _verdicts("n_dl_unrounded", snaps, lane_width64=lw64)
    assert old and not new


def _with_lane_width(cfg, lw64):
    """the same buffers under a config whose lane_width is float(lw64): the distances are inputs, only their normaliser changes (compared against row64 only)"""
    import copy

    c = copy.copy(cfg)
    c.lane_width = lw64
    return c


def test_previous_position_defect():
    """dx from the position BEFORE the step for agents that moved less than 1e-5 (speed 1e-4, dt 0.05: 5e-6 per step)"""
    N, B = 6, 6
    p = _params(N=N)
    mp = load_map("cpm_entire")
    cfg = make_config(p, mp, B)
    ora = ob.OracleEnv(cfg, mp)
    env_idx, agent_idx, ids, st = oc.injected_edge_states(cfg, mp)
    st = st.copy()
    st[:, 3] = 1e-4
    st[:, 5], st[:, 6] = st[:, 3] * np.cos(st[:, 2]), st[:, 3] * np.sin(st[:, 2])
    ora.reset(env_idx, agent_idx, ids, st, 1)
    ora.observe()
    before = ora.get(capi.BUF_PREV_POS)
    ora.step(np.tile(f32([1e-4, 0.0]), (B, N, 1)))
    bufs = oc.read_bufs(ora, np.zeros((B, N), bool))
    ora.close()
    now = bufs[capi.BUF_STATE][..., :2]
    moved = np.abs(now - before).max(axis=-1)
    sel = (moved > 0) & (moved < 1e-5)
    assert sel.sum() > B * N // 2
    snaps = [("slow step", cfg, mp, bufs)]
    assert _verdicts(None, snaps)[1]
    old, new = _verdicts("prev_pos", snaps, prev=(before[..., 0], before[..., 1], sel))
    assert old and not new


def test_relative_rotation_wrapped_with_the_float64_two_pi():
    """|psi| around 100 rad: sixteen turns of the float64 2 pi instead of TWO_PI32 are 2.8e-6 rad off -- inside the flat bar (compared modulo 1), outside the bound"""
    cfg, mp, bufs = _edge_snapshot(is_observe_vertices=False)
    snaps = [("edge states", cfg, mp, bufs)]
    res = oc.compare(bufs[capi.BUF_OBS], cfg, mp, bufs, form="reference")
    assert res["ok"], oc.report(res)
    assert _verdicts(None, snaps)[1]
    rows = twin_rows(cfg, mp, bufs, "wrap_2pi_f64")
    d = np.abs(rows.astype(np.float64) - bufs[capi.BUF_OBS])
    assert np.minimum(d, np.abs(d - 1.0)).max() <= 1e-5
    assert not oc.compare(rows, cfg, mp, bufs)["ok"]


@pytest.mark.parametrize("defect", ["vertices_swapped", "xy_exchanged", "r_pos_for_distance"])
def test_large_defects_fail(defect):
    snaps, _ = snapshots("default-cpm_entire-mask0-mtv0")
    assert not _verdicts(defect, snaps)[1]
    for _, cfg, mp, bufs in snaps[:2]:
        assert not oc.compare(twin_rows(cfg, mp, bufs, defect), cfg, mp, bufs)["ok"]


# ---- the edges --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(is_apply_mask=True), dict(is_observe_vertices=False, is_obs_steering=True), dict(is_ego_view=False, is_obs_steering=True)],
                         ids=["default", "mask", "novert-steer", "bird"])
def test_injected_edge_states_oracle_and_twin(kw):
    cfg, mp, bufs = _edge_snapshot(**kw)
    res = oc.compare(bufs[capi.BUF_OBS], cfg, mp, bufs, form="reference")
    assert res["ok"], oc.report(res)
    rt = oc.compare(twin_rows(cfg, mp, bufs), cfg, mp, bufs)
    assert rt["ok"], oc.report(rt)
    e = oc.EDGE_ENVS.index
    want, bnd = oc.row64(cfg, mp, bufs), oc.bound(cfg, mp, bufs)
    if not kw:
        co = bufs[capi.BUF_NEARING][e("coincident"), 2]
        assert co[0] == 3 and (bnd[e("coincident"), 2, 10:18:2] > 0).all()  # the coincident neighbour is observed; its vertices are not at the ego's centre
        assert want[e("zero_speed"), :, 0].max() == 0 and bnd[e("zero_speed"), :, 0].max() == 0
    if kw.get("is_apply_mask"):
        d = bufs[capi.BUF_DIST_AGENTS][e("at_mask")]
        dm = f32(cfg.distance_mask_agents)
        assert d[0, 1] == dm and d[0, 2] == np.nextafter(dm, f32(0)) and set(bufs[capi.BUF_NEARING][e("at_mask"), 0]) == {1, 2}
        blk = bufs[capi.BUF_OBS][e("at_mask"), 0, 10:].reshape(2, 11)
        k1 = list(bufs[capi.BUF_NEARING][e("at_mask"), 0]).index(1)
        assert (blk[k1, :8] == 1).all() and blk[k1, 10] == 1 and (blk[k1, 8:10] == 0).all()   # exactly at the mask distance: masked
        assert blk[1 - k1, 10] != 1                                                              # an ulp nearer: not
