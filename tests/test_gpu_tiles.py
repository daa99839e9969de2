"""The step kernel at every tile shape it can launch with (run with -m gpu on an MI355X).

`sigmaenv_step_wave_kernel` is a template with fifteen instantiations; `sigmaenv_create` decides the tiling (wave_G envs per wavefront tile, wave_wpb tiles per
workgroup, a fixed-shape instantiation or the generic one) and `launch_step` picks the instantiation.  The rest of the suite runs it at one env per wavefront; here
every case FORCES a tiling -- through `cfg.envs_per_group` (the product path) or the diagnostic switches of README.md -- ASSERTS with `SigmaEnv.launch_shape()`
that it got the tiling and the instantiation it names, and then holds the kernel, after every launch,

  (a) to the C oracle (test_gpu_parity._compare_all: masks / indices / counters bit-exact, fp32 within FTOL), and
  (b) to a second HIP handle fed the same inputs at the baseline the rest of the suite covers (wave_G = 1, wave_wpb = 1, generic instantiation): EVERY buffer, the
      observation rows and the rollout slab included, byte for byte.  The arithmetic contract is per agent (-ffp-contract=off, fixed operation order) and the
      tile-level merges are order-independent min / max, so the tile shape may not change a single bit.  That covers the candidates for a deliberate difference too:
      the shared-reciprocal division is documented as bit-identical to `/` (sigmaenv_device.h, div_shared), the pruned scan as exact (DESIGN.md "Pruned scan"), and
      the MTVS instantiations stage the same per-rectangle records -- no exception is made for any of them.

The drivers alternate between `step_autoreset`, `step` + `auto_reset`, and `step_autoreset_n` chunks of 2 .. 32 steps (the in-kernel step loop: one wavefront walks all
envs of its tile through resets), with one host-driven partial `reset` + `observe` (the stand-alone kernels at G > 1).  What keeps a case from showing nothing is
asserted on the ORACLE's buffers (and therefore checked without a GPU, test_matrix_case_meets_its_conditions_on_the_oracle): an env finished; a finished env lay in
the ragged last tile; some step had a tile in which some envs finished and others did not; on entry / exit maps a per-agent exit request was served."""
import math
from collections import namedtuple

import numpy as np
import pytest

import oracle_binding as ob
import test_gpu_parity as tp
from sigmarl_amd import capi
from sigmarl_amd.maps import load_map
from sigmarl_amd.params import Parameters, make_config

gpu = pytest.mark.gpu

LDS_LIMIT = 64 * 1024  # what a workgroup may ask for on every device without the opt-in attribute: no case needs more
SWITCHES = ("SIGMAENV_WAVE_G", "SIGMAENV_WPB", "SIGMAENV_WAVE_SPEC", "SIGMAENV_FASTDIV", "SIGMAENV_PRUNE", "SIGMAENV_G", "SIGMAENV_BLOCK", "SIGMAENV_RESET_BLOCK")
ALL_BUFS = tp.INT_BUFS + tp.FLT_BUFS
CHUNKS = [(2, 9, 32), (3, 12, 27), (5, 16, 21)]  # step_autoreset_n chunk lengths of a run's three rounds

Case = namedtuple("Case", "name scen N G B wpb spec0 fixed mtv obs testing fastdiv prune via extra slab rew seed mtvs")


def R(name, N, G, B, scen="cpm_entire", wpb=1, spec0=False, fixed=False, mtv=False, obs=False, testing=False, fastdiv=True, prune=True, via="epg", extra=None,
      slab=True, rew="distance", seed=1, mtvs=False):
    return Case(name, scen, N, G, B, wpb, spec0, fixed, mtv, obs, testing, fastdiv, prune, via, dict(extra or {}), slab, rew, seed, mtvs)


# B is never a multiple of wave_G and the tile count never a multiple of wave_wpb (ragged last tile AND ragged last workgroup), except where a row says so
MATRIX = [
    # ---- the tile-shape rows ------------------------------------------------------------------------------------------------------------
    R("fixed_4x4", 4, 4, 39, fixed=True),
    R("fixed_8x2", 8, 2, 21, fixed=True, rew="ttc"),
    R("generic_4x4", 4, 4, 39, spec0=True),
    R("generic_8x2", 8, 2, 21, spec0=True, rew="ttc"),
    R("16x2_par", 16, 2, 13),
    R("16x4_64_lanes", 16, 4, 14, rew="distance_sparse"),
    R("5x3_default_rule_shape", 5, 3, 32),
    R("3x5", 3, 5, 23, rew="ttc_sparse"),
    R("7x2_by_switch", 7, 2, 17, via="env"),
    R("6x10_60_lanes", 6, 10, 47),
    R("21x3_63_lanes", 21, 3, 8),
    R("2x8", 2, 8, 43, rew="ttc"),
    R("2x32", 2, 32, 75),
    R("1x16", 1, 16, 55),
    R("1x64", 1, 64, 150, rew="sparse"),
    R("33x1_wpb2", 33, 1, 5, wpb=2),
    R("2x32_single_partial_tile", 2, 32, 19),        # B < wave_G
    R("fixed_4x4_exact_multiple", 4, 4, 40, fixed=True, wpb=2),  # B a multiple of wave_G, the tile count a multiple of wave_wpb
    # ---- fixed 4x4, fixed 8x2 and generic 5x3 crossed with tiles per workgroup, mtv, observation variant, testing mode, entry / exit map ---
    R("fixed_4x4_wpb2", 4, 4, 35, fixed=True, wpb=2, slab=False),
    R("fixed_4x4_wpb4", 4, 4, 39, fixed=True, wpb=4),
    R("fixed_8x2_wpb2", 8, 2, 21, fixed=True, wpb=2),
    R("fixed_8x2_wpb4", 8, 2, 21, fixed=True, wpb=4, slab=False),
    R("5x3_wpb2", 5, 3, 32, wpb=2, slab=False),
    R("5x3_wpb4", 5, 3, 32, wpb=4),
    R("fixed_4x4_mtv", 4, 4, 39, fixed=True, mtv=True, rew="ttc"),
    R("fixed_8x2_mtv", 8, 2, 21, fixed=True, mtv=True),
    R("5x3_mtv", 5, 3, 32, mtv=True, rew="ttc_sparse"),
    R("4x4_obs_variant", 4, 4, 39, obs=True),
    R("8x2_obs_variant", 8, 2, 21, obs=True, wpb=2),
    R("5x3_obs_variant", 5, 3, 32, obs=True),
    R("fixed_4x4_testing", 4, 4, 39, fixed=True, testing=True, rew="sparse"),
    R("fixed_8x2_testing", 8, 2, 21, fixed=True, testing=True, mtv=True, rew="ttc"),
    R("5x3_testing", 5, 3, 32, testing=True),
    R("fixed_4x4_intersection", 4, 4, 39, fixed=True, scen="intersection_1"),
    R("fixed_8x2_intersection", 8, 2, 21, fixed=True, scen="intersection_1", wpb=2),
    R("5x3_on_ramp", 5, 3, 32, scen="on_ramp_1", mtv=True),
    # ---- the other switches -----------------------------------------------------------------------------------------------------------------
    R("5x3_plain_division", 5, 3, 32, fastdiv=False),
    R("16x4_plain_division", 16, 4, 14, fastdiv=False),
    R("4x4_obs_plain_division", 4, 4, 39, obs=True, fastdiv=False),
    R("16x4_obs_plain_division", 16, 4, 14, obs=True, fastdiv=False),
    R("8x2_full_scan", 8, 2, 21, prune=False, fixed=True),
    R("8x2_standalone_kernel_switches", 8, 2, 21, fixed=True, extra={"SIGMAENV_G": 4, "SIGMAENV_BLOCK": 128, "SIGMAENV_RESET_BLOCK": 512}),
    # ---- the one-env-per-wavefront instantiations with more than one tile per workgroup, and the remaining observation-variant ones ---------
    R("fixed_16x1_wpb2", 16, 1, 7, fixed=True, wpb=2),
    R("fixed_16x1_obs_wpb4", 16, 1, 7, fixed=True, obs=True, wpb=4),
    R("fixed_16x1_mtv_wpb2", 16, 1, 7, fixed=True, mtv=True, mtvs=True, wpb=2),
    R("fixed_16x1_mtv_obs_wpb4", 16, 1, 7, fixed=True, mtv=True, mtvs=True, obs=True, wpb=4),
    R("fixed_32x1_wpb2", 32, 1, 5, fixed=True, wpb=2),
    R("33x1_obs_variant", 33, 1, 5, obs=True, wpb=2),
    R("16x4_obs_variant", 16, 4, 14, obs=True),
]
MATRIX = [c._replace(seed=i + 1) for i, c in enumerate(MATRIX)]

FIFTEEN = {  # <FASTDIV, PAR, SN, SG, VAR, MTVS> of every instantiation launch_step can select (sigmaenv.hip: select_step_kernel)
    (True, True, 0, 0, False, False), (True, False, 0, 0, False, False), (False, True, 0, 0, False, False), (False, False, 0, 0, False, False),
    (True, True, 16, 1, True, False), (True, True, 0, 0, True, False), (True, False, 0, 0, True, False), (False, True, 0, 0, True, False),
    (False, False, 0, 0, True, False), (True, True, 16, 1, False, False), (True, True, 16, 1, False, True), (True, True, 16, 1, True, True),
    (True, True, 32, 1, False, False), (True, True, 8, 2, False, False), (True, True, 4, 4, False, False),
}


def expected_instantiation(c):
    """The template arguments the case names: a fixed-shape instantiation exists with the shared-reciprocal division only; PAR = two lanes per agent fit a wavefront."""
    if c.fixed and not c.spec0:
        return (True, True, c.N, c.G, c.obs, c.mtvs)
    return (c.fastdiv, 2 * c.G * c.N <= 64, 0, 0, c.obs, False)


def baseline_instantiation(c):
    return (True, 2 * c.N <= 64, 0, 0, c.obs, False)


def _config(c):
    kw = dict(n_agents=c.N, scenario_type=c.scen, is_use_mtv_distance=c.mtv, rew_method=c.rew, dt=0.05, is_apply_mask=False, is_obs_noise=False, max_steps=11,
              is_testing_mode=c.testing)
    if c.obs:  # obs_flags != 0: the steering angle and the neighbours' short-term paths join the row (the VAR instantiations)
        kw.update(is_obs_steering=True, is_observe_ref_path_other_agents=True)
    mp = load_map(c.scen)
    cfg = make_config(Parameters(**kw), mp, c.B)
    assert (cfg.obs_flags != 0) == c.obs
    return cfg, mp


def _handle(monkeypatch, cfg, mp, envs_per_group, switches):
    """A HIP handle created under exactly these diagnostic switches (they are read at sigmaenv_create) and this cfg.envs_per_group."""
    with monkeypatch.context() as m:
        for k in SWITCHES:
            m.delenv(k, raising=False)
        for k, v in switches.items():
            m.setenv(k, str(v))
        own = capi.Config.from_buffer_copy(cfg)
        own.envs_per_group = envs_per_group
        return tp._hip_env(own, mp)


def _where(which, a, b, bad, N, G):
    """(env, agent, tile, slot) of the first element of buffer `which` flagged in `bad`."""
    e = int(np.argmax(bad.reshape(bad.shape[0], -1).any(axis=1)))
    per_agent = which not in (capi.BUF_DONE, capi.BUF_TIMER) and a.ndim >= 2 and a.shape[1] == N
    i = int(np.argmax(bad[e].reshape(N, -1).any(axis=1))) if per_agent else None
    slot = (e % G) * N + (i or 0)
    return f"buffer {which}: first at (env {e}, agent {i}, tile {e // G}, slot {slot}): {a[e].reshape(-1)[:8] if i is None else a[e, i].reshape(-1)[:8]} vs " \
           f"{b[e].reshape(-1)[:8] if i is None else b[e, i].reshape(-1)[:8]}"


def _locate_oracle_mismatch(dev, ora, N, G):
    for which in tp.INT_BUFS:
        a, b = dev.get(which), ora.get(which)
        if not np.array_equal(a, b):
            return _where(which, a, b, a != b, N, G)
    for which in tp.FLT_BUFS:
        a, b = dev.get(which), ora.get(which)
        both_inf = np.isinf(a) & np.isinf(b) & (np.sign(a) == np.sign(b))
        bad = ~(np.where(both_inf, 0.0, np.abs(a.astype(np.float64) - b.astype(np.float64))) <= tp.FTOL)
        if bad.any():
            return _where(which, a, b, bad, N, G)
    return "no buffer located"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8 if a.dtype.itemsize == 1 else np.uint32)


def _assert_same_bits(tag, what, a, b, N, G, which=-1):
    if a.tobytes() != b.tobytes():
        bad = _bits(a) != _bits(b)
        raise AssertionError(f"{tag}: {what} differs between the tile shape under test and the one-env-per-wavefront baseline in {int(bad.sum())} words; "
                             + _where(which, a, b, bad, N, G))


class _Run:
    """One case: the oracle, and the HIP handles (the tile shape under test first, the baseline second; none on a machine without a GPU)."""

    def __init__(self, c, devs):
        self.c, self.devs = c, devs
        self.cfg, self.mp = _config(c)
        self.ora = ob.OracleEnv(self.cfg, self.mp)
        self.B, self.N, self.G, self.D = c.B, c.N, c.G, self.ora.D
        self.W = self.N * (self.D + 1) + 1
        self.pf, self.pc = int(self.mp.list_first[0]), int(self.mp.list_count[0])
        self.n_done = self.n_last_tile = self.n_mixed = self.n_req = 0
        self.rows = []
        if devs and c.slab:
            import torch

            self.rows = [torch.full((self.B, self.W), float("nan"), device="cuda") for _ in devs]
            for d, row in zip(devs, self.rows):
                d.env.set_slab(row)

    # -- the oracle side, and the conditions on its buffers -------------------------------------------------------------------------------
    def ora_step(self, act):
        self.ora.step(act)
        done = self.ora.get(capi.BUF_DONE).astype(bool)
        self.n_done += int(done.sum())
        self.n_last_tile += int(done[((self.B - 1) // self.G) * self.G:].sum())
        for k in range(0, self.B, self.G):
            tile = done[k:k + self.G]
            self.n_mixed += int(0 < tile.sum() < len(tile))
        self.n_req += int(self.ora.get(capi.BUF_COL_FLAGS)[..., 3].sum())
        return self.ora.get(capi.BUF_OBS).copy(), self.ora.get(capi.BUF_REWARD).copy(), done

    def actions(self, rng, t):
        B, N = self.B, self.N
        mode = t % 3
        if mode == 0:
            act = np.stack([rng.uniform(0, 1, (B, N)), rng.uniform(-0.25, 0.25, (B, N))], axis=-1)
        elif mode == 1:
            act = np.stack([rng.uniform(0.1, 0.4, (B, N)), rng.uniform(-0.03, 0.03, (B, N))], axis=-1)
        else:
            act = np.stack([rng.uniform(-0.5, 1.6, (B, N)), rng.uniform(-0.9, 0.9, (B, N))], axis=-1)
        return act.astype(np.float32)

    # -- the comparisons after a launch -------------------------------------------------------------------------------------------------
    def check(self, tag):
        tag = f"{self.c.name}: {tag}"
        for d in self.devs:
            try:
                tp._compare_all(d, self.ora, tag)
            except AssertionError as e:
                raise AssertionError(f"{e}; {'tile shape under test' if d is self.devs[0] else 'baseline'}: {_locate_oracle_mismatch(d, self.ora, self.N, self.G)}") from None
        if len(self.devs) == 2:
            for which in ALL_BUFS:
                _assert_same_bits(tag, f"buffer {which}", self.devs[0].get(which), self.devs[1].get(which), self.N, self.G, which)

    def check_record(self, tag, rows, rec):
        """The rollout record rows ([B, W] host arrays, one per handle) of a step whose oracle result is rec = (obs, reward, done)."""
        tag = f"{self.c.name}: {tag}"
        N, D, B = self.N, self.D, self.B
        for row in rows:
            obs, rew, done = row[:, :N * D].reshape(B, N, D), row[:, N * D:N * D + N], row[:, -1]
            assert np.abs(obs.astype(np.float64) - rec[0]).max() <= tp.FTOL, f"{tag}: record observation"
            assert np.abs(rew.astype(np.float64) - rec[1]).max() <= tp.FTOL, f"{tag}: record reward"
            assert np.array_equal(done != 0, rec[2]), f"{tag}: record done flags"
        if len(rows) == 2:
            _assert_same_bits(tag, "rollout record", rows[0].reshape(B, -1), rows[1].reshape(B, -1), 1, self.G)

    def slab_rows(self):
        for d in self.devs:
            d.env.sync()
        return [r.cpu().numpy() for r in self.rows]

    # -- the drivers ---------------------------------------------------------------------------------------------------------------------
    def fused(self, act, t):
        for d in self.devs:
            d.step_autoreset(act, self.c.seed, t + 1, self.pf, self.pc)
        rec = self.ora_step(act)
        self.ora.auto_reset(self.c.seed, t + 1, self.pf, self.pc)
        self.check(f"step_autoreset, step {t}")
        if self.rows:
            self.check_record(f"step_autoreset, step {t}", self.slab_rows(), rec)

    def separate(self, act, t):
        for d in self.devs:
            d.step(act)
        rec = self.ora_step(act)
        self.check(f"step {t}")
        if self.rows:  # the record of a plain step IS the individual buffers
            rows = self.slab_rows()
            self.check_record(f"step {t}", rows, rec)
            for d, row in zip(self.devs, rows):
                N, D, B = self.N, self.D, self.B
                assert np.array_equal(row[:, :N * D].reshape(B, N, D), d.get(capi.BUF_OBS)) and np.array_equal(row[:, N * D:N * D + N], d.get(capi.BUF_REWARD))
                assert np.array_equal(row[:, -1] != 0, d.get(capi.BUF_DONE) != 0)
        for d in self.devs:
            d.auto_reset(self.c.seed, t + 1, self.pf, self.pc)
        self.ora.auto_reset(self.c.seed, t + 1, self.pf, self.pc)
        self.check(f"auto_reset after step {t}")

    def chunk(self, acts, t):
        n = len(acts)
        recs = []
        slabs = []
        for d in self.devs:
            import torch

            a = torch.as_tensor(acts).to(d.env.device).contiguous()
            slab = torch.full((n, self.B, self.W), float("nan"), device="cuda") if self.c.slab else None
            d.env.step_autoreset_n(a, slab, seed=self.c.seed, counter0=t + 1, path_first=self.pf, path_count=self.pc)
            d.env.sync()
            slabs.append(slab)
        for k in range(n):
            recs.append(self.ora_step(acts[k]))
            self.ora.auto_reset(self.c.seed, t + 1 + k, self.pf, self.pc)
        self.check(f"step_autoreset_n, steps {t} .. {t + n - 1}")
        if self.devs and self.c.slab:
            host = [s.cpu().numpy() for s in slabs]
            for k in range(n):
                self.check_record(f"step_autoreset_n, step {t + k} of the chunk from {t}", [h[k] for h in host], recs[k])

    def host_resets(self, rng):
        """sigmaenv_reset + sigmaenv_observe (the stand-alone kernels, G envs per workgroup): every third env as a whole (its neighbours in the tile are not touched),
        then single agents of a few other envs, onto random centre-line points (as tools/fuzz_parity.one_case places them)."""
        mp, pf, pc, B, N = self.mp, self.pf, self.pc, self.B, self.N
        whole = list(range(0, B, 3))
        some = [int(e) for e in rng.choice([e for e in range(B) if e % 3], size=min(4, B - len(whole)), replace=False)] if B > len(whole) else []
        for full, envs in ((True, whole), (False, some)):
            ei, ai, ids, st8 = [], [], [], []
            for e in envs:
                agents = range(N) if full else rng.choice(N, size=int(rng.integers(1, N + 1)), replace=False)
                for i in agents:
                    gp = pf + int(rng.integers(pc))
                    pt = int(rng.integers(1, max(2, int(mp.n_center[gp]) - 2)))
                    x, y = [float(v) for v in mp.center[gp, pt]]
                    yaw = float(mp.yaw[gp, min(pt, int(mp.n_yaw[gp]) - 1)])
                    sp = float(rng.uniform(0, 1))
                    ei.append(int(e)); ai.append(int(i)); ids.append((gp, 0, gp - pf, pt))
                    st8.append((x, y, yaw, sp, 0.0, sp * np.cos(np.float32(yaw)), sp * np.sin(np.float32(yaw)), 0.0))
            if not ei:
                continue
            for env_ in self.devs + [self.ora]:
                env_.reset(np.asarray(ei, np.int32), np.asarray(ai, np.int32), np.asarray(ids, np.int32), np.asarray(st8, np.float32), int(full))
                env_.observe()
            self.check(f"host reset ({'whole envs' if full else 'single agents'})")

    def run(self):
        c = self.c
        for d in self.devs:
            d.env.buffer(capi.BUF_DONE).fill_(1)
            d.auto_reset(c.seed, 0, self.pf, self.pc)
        self.ora.get(capi.BUF_DONE, copy=False)[:] = 1
        self.ora.auto_reset(c.seed, 0, self.pf, self.pc)
        self.check("initial reset of every env")
        rng = np.random.default_rng(7000 + c.seed)
        t = 0
        for rnd, n in enumerate(CHUNKS[c.seed % 3]):
            self.fused(self.actions(rng, t), t)
            t += 1
            self.separate(self.actions(rng, t), t)
            t += 1
            if rnd == 0:
                self.host_resets(rng)
            self.chunk(np.stack([self.actions(rng, t + k) for k in range(n)]), t)
            t += n
        self.ora.close()
        # the conditions, on the oracle's buffers
        assert self.n_done > 0, f"{c.name}: no env finished"
        assert self.n_last_tile > 0, f"{c.name}: no finished env in the last tile (envs {((self.B - 1) // self.G) * self.G} .. {self.B - 1})"
        if c.G > 1 and c.B > 1:
            assert self.n_mixed > 0, f"{c.name}: no step with a tile in which some envs finished and others did not"
        if self.cfg.has_entry_exit:
            assert self.n_req > 0, f"{c.name}: no per-agent exit request on an entry / exit map"
        return t


def test_the_matrix_names_all_fifteen_instantiations_and_ragged_sizes():
    """Every case asserts at run time that it launched the instantiation it names (expected_instantiation); together the cases name all fifteen of launch_step.
    And the sizes are what the module's docstring says: ragged last tile and ragged last workgroup, one single partial tile, one exact multiple."""
    assert {expected_instantiation(c) for c in MATRIX} == FIFTEEN
    assert len({c.name for c in MATRIX}) == len(MATRIX)
    exact = [c for c in MATRIX if c.G > 1 and c.B % c.G == 0]
    assert [c.name for c in exact] == ["fixed_4x4_exact_multiple"]
    assert any(c.B < c.G for c in MATRIX)
    for c in MATRIX:
        tiles = (c.B + c.G - 1) // c.G
        assert c.G * c.N <= 64 and c.wpb in (1, 2, 4)
        if c not in exact and c.wpb > 1:
            assert tiles % c.wpb != 0, c.name
    for g in {c.G for c in MATRIX}:
        assert any(c.slab for c in MATRIX if c.G == g), g  # the rollout record is compared on at least one row per distinct wave_G


@pytest.mark.parametrize("c", MATRIX, ids=[c.name for c in MATRIX])
def test_matrix_case_meets_its_conditions_on_the_oracle(c):
    """No GPU: the case's workload alone, on the oracle -- finished envs, one of them in the ragged last tile, a tile with finished and unfinished envs in the
    same step, exit requests on entry / exit maps.  (The GPU test asserts the same on the same run.)"""
    steps = _Run(c, []).run()
    assert 40 <= steps <= 52


@gpu
@pytest.mark.parametrize("c", MATRIX, ids=[c.name for c in MATRIX])
def test_tile_shape_against_oracle_and_against_one_env_per_wavefront(c, monkeypatch):
    cfg, mp = _config(c)
    sw = dict(c.extra)
    if c.via == "env":
        sw["SIGMAENV_WAVE_G"] = c.G
    if c.wpb != 1:
        sw["SIGMAENV_WPB"] = c.wpb
    if c.spec0:
        sw["SIGMAENV_WAVE_SPEC"] = 0
    if not c.fastdiv:
        sw["SIGMAENV_FASTDIV"] = 0
    if not c.prune:
        sw["SIGMAENV_PRUNE"] = 0
    dev = _handle(monkeypatch, cfg, mp, c.G if c.via == "epg" else 0, sw)
    base = _handle(monkeypatch, cfg, mp, 1, {"SIGMAENV_WAVE_SPEC": 0, "SIGMAENV_WPB": 1})
    try:
        ls, lb = dev.env.launch_shape(), base.env.launch_shape()
        tiles = (c.B + c.G - 1) // c.G
        print(f"{c.name}: N={c.N} B={c.B} launch_shape: instantiation <FASTDIV, PAR, SN, SG, VAR, MTVS> = {ls['instantiation']}, wave_G {ls['wave_G']}, "
              f"wave_wpb {ls['wave_wpb']}, wave_grid {ls['wave_grid']}, wave_spec {ls['wave_spec']}, LDS {ls['wave_lds_bytes']} B; stand-alone kernels G {ls['G']}, "
              f"block {ls['block']}, grid {ls['grid']}, reset_block {ls['reset_block']}, LDS {ls['smem_bytes']} B")
        assert (ls["wave_G"], ls["wave_wpb"], ls["wave_grid"]) == (c.G, c.wpb, (tiles + c.wpb - 1) // c.wpb), ls
        assert ls["wave_spec"] == (c.N * 256 + c.G if c.fixed and not c.spec0 else 0), ls
        assert ls["instantiation"] == expected_instantiation(c), ls
        assert (ls["map_fast_div"], ls["pruned_scan"]) == (int(c.fastdiv), int(c.prune)), ls
        assert ls["wave_lds_bytes"] <= LDS_LIMIT and ls["smem_bytes"] <= LDS_LIMIT, ls
        want_g = int(c.extra.get("SIGMAENV_G", c.G if c.via == "epg" else ls["G"]))
        assert (ls["G"], ls["block"], ls["reset_block"]) == (want_g, int(c.extra.get("SIGMAENV_BLOCK", 256)), int(c.extra.get("SIGMAENV_RESET_BLOCK", 256))), ls
        assert ls["grid"] == (c.B + ls["G"] - 1) // ls["G"]
        assert (lb["wave_G"], lb["wave_wpb"], lb["wave_grid"], lb["wave_spec"], lb["G"]) == (1, 1, c.B, 0, 1), lb
        assert lb["instantiation"] == baseline_instantiation(c) and lb["map_fast_div"] == 1 and lb["pruned_scan"] == 1, lb
        _Run(c, [dev, base]).run()
    finally:
        dev.close()
        base.close()


# ---- the default rule at the sizes where it switches -----------------------------------------------------------------------------------------
def _odd_not_multiple(b, wg, step):
    while b % 2 == 0 or (wg > 1 and b % wg == 0):
        b += step
    return b


@gpu
@pytest.mark.parametrize("N,wg,above", [(4, 4, True), (8, 2, True), (5, 3, True), (4, 4, False), (8, 2, False), (5, 3, False)])
def test_default_rule_at_its_thresholds(N, wg, above, monkeypatch):
    """No override at all: sigmaenv_create starts from 16 / N envs per wavefront and halves while there are fewer than 16 tiles per compute unit.  Just above
    wg * 16 * n_cu envs the library must launch 4 x 4 / 8 x 2 / the generic kernel at 3 envs per wavefront, just below it the tile the halving gives (2 / 1 / 1) --
    and six steps (fused and separate launches in turn) equal the oracle on EVERY env."""
    import torch

    thr = 16 * torch.cuda.get_device_properties(0).multi_processor_count
    B = _odd_not_multiple(wg * thr + 1, wg, 1) if above else _odd_not_multiple(wg * (thr - 1) - 1, wg, -1)
    half = wg >> 1
    assert (B + wg - 1) // wg >= thr if above else ((B + wg - 1) // wg < thr and (half <= 1 or (B + half - 1) // half >= thr))
    want_g = wg if above else max(half, 1)
    p = Parameters(n_agents=N, scenario_type="cpm_entire", is_use_mtv_distance=False, rew_method="distance", is_apply_mask=False, is_obs_noise=False, max_steps=5)
    mp = load_map("cpm_entire")
    cfg = make_config(p, mp, B)
    dev, ora = _handle(monkeypatch, cfg, mp, 0, {}), ob.OracleEnv(cfg, mp)
    try:
        ls = dev.env.launch_shape()
        print(f"default rule N={N} B={B} ({'above' if above else 'below'} {wg} x {thr}): wave_G {ls['wave_G']}, wave_spec {ls['wave_spec']}, instantiation {ls['instantiation']}")
        assert B % want_g != 0 or want_g == 1
        assert ls["wave_G"] == want_g and ls["wave_wpb"] == 1 and ls["wave_grid"] == (B + want_g - 1) // want_g, ls
        fixed = (N, want_g) in ((4, 4), (8, 2))
        assert ls["wave_spec"] == (N * 256 + want_g if fixed else 0), ls
        assert ls["instantiation"] == ((True, True, N, want_g, False, False) if fixed else (True, True, 0, 0, False, False)), ls
        pf, pc = mp.list_first[0], mp.list_count[0]
        dev.env.buffer(capi.BUF_DONE).fill_(1)
        ora.get(capi.BUF_DONE, copy=False)[:] = 1
        dev.auto_reset(9, 0, pf, pc)
        ora.auto_reset(9, 0, pf, pc)
        tp._compare_all(dev, ora, "initial reset")
        rng = np.random.default_rng(N)
        n_done = 0
        for t in range(6):
            act = np.stack([rng.uniform(-0.2, 1.3, (B, N)), rng.uniform(-0.7, 0.7, (B, N))], axis=-1).astype(np.float32)
            try:
                if t % 2:
                    dev.step(act)
                    ora.step(act)
                    tp._compare_all(dev, ora, f"N={N} B={B} step {t}")
                    dev.auto_reset(9, t + 1, pf, pc)
                else:
                    dev.step_autoreset(act, 9, t + 1, pf, pc)
                    ora.step(act)
                n_done += int(ora.get(capi.BUF_DONE).sum())
                ora.auto_reset(9, t + 1, pf, pc)
                tp._compare_all(dev, ora, f"N={N} B={B} after step {t} and its resets")
            except AssertionError as e:
                raise AssertionError(f"{e}; {_locate_oracle_mismatch(dev, ora, N, want_g)}") from None
        assert n_done > 0
    finally:
        dev.close()
        ora.close()


def test_thresholds_of_the_default_rule_are_odd_and_ragged():
    for thr in (16 * 256, 16 * 304, 16 * 64):
        for wg in (4, 2, 3):
            a, b = _odd_not_multiple(wg * thr + 1, wg, 1), _odd_not_multiple(wg * (thr - 1) - 1, wg, -1)
            assert a % 2 and a % wg and (a + wg - 1) // wg >= thr and a - wg * thr < 8
            assert b % 2 and b % wg and (b + wg - 1) // wg < thr and wg * thr - b < 16
            assert math.ceil(b / max(wg >> 1, 1)) >= thr or wg >> 1 <= 1
