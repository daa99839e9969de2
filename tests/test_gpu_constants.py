"""The env kernels away from the default vehicle and reward constants (run with -m gpu): the HIP path against the reference goldens generated at the perturbed
constants, and against the CPU oracle on seeded runs whose configs went through tests/perturbed_constants.py -- every field pair that coincides at the defaults
(l_f / l_r, min_acc / -max_acc, the two near penalties, the two collision penalties, the two CBF deviation penalties, the three lower thresholds, max_speed = 1,
reward_reach_goal = 1, distance_mask_agents = 5 * length) holds two different values here.

Bar: that of test_gpu_parity.py -- masks / indices / counters bit-exact, NO differing fp32 word outside the observation rows, observation rows within 1e-5."""
import numpy as np
import pytest

import constants_run as cr
import perturbed_constants as pc_
import oracle_binding as ob
import test_cbf_qp  # noqa: F401  (the bodies reused below are imported HERE, before the hook can be active: a module first imported under it would keep its names)
import test_constants_host as host
import test_gpu_cbf  # noqa: F401
import test_gpu_eval  # noqa: F401
import test_gpu_observation  # noqa: F401
import test_gpu_render  # noqa: F401
import test_gpu_reset_core  # noqa: F401
import test_gpu_parity as tp
import traj_replay as tr
from sigmarl_amd import capi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", tr.TRAJ_NAMES_PERTURBED)
def test_hip_vs_reference_goldens_perturbed(name):
    tp.test_hip_vs_reference_goldens(name)


def _pair(cfg, mp):
    return tp._hip_env(cfg, mp), ob.OracleEnv(cfg, mp)


def _lockstep(case, cfg=None):
    """device and oracle through cr.drive (single-step launches, auto_reset after each), every buffer compared after every launch; returns the device's record"""
    cfg0, cc, mp = cr.build(case)
    dev, ora = _pair(cfg0 if cfg is None else cfg, mp)
    n = [0]
    by = {}
    rec = cr.drive([ora, dev], cc, mp, case,
                   after_step=lambda t: n.__setitem__(0, n[0] + tp._compare_all(dev, ora, f"{case} step {t}", by)),
                   after_reset=lambda t: n.__setitem__(0, n[0] + tp._compare_all(dev, ora, f"{case} reset after step {t}", by)))
    dev.close()
    ora.close()
    assert n[0] == 0, f"{n[0]} differing fp32 words, by buffer id: {by}"
    return rec


# scenario, N, B, rew_method, mtv, testing, n_points_short_term, launch.  Every rew_method of the parity fuzzer, both distance types, N in {1, 3, 4, 16, 17}
# (proximity penalty staged / unstaged, collision rows word-aligned / bytes), the three launch forms (the T-step launch has its own copy of the action clamp)
SEEDED = [
    ("cpm_entire", 1, 5, "distance", False, False, 3, "single"),
    ("cpm_entire", 3, 33, "distance", True, False, 3, "fused"),
    ("cpm_entire", 4, 40, "ttc", False, False, 3, "tstep"),
    ("cpm_entire", 16, 12, "distance", False, False, 3, "single"),
    ("cpm_entire", 17, 9, "distance", False, False, 3, "fused"),
    ("cpm_entire", 17, 6, "distance_sparse", True, False, 3, "tstep"),
    ("cpm_entire", 16, 8, "ttc_sparse", True, False, 3, "single"),
    ("cpm_entire", 4, 24, "sparse", False, False, 3, "fused"),
    ("cpm_entire", 16, 7, "distance", True, False, 3, "tstep"),
    ("intersection_1", 3, 20, "distance_sparse", False, True, 3, "single"),
    ("cpm_entire", 4, 16, "ttc", True, False, 2, "fused"),
    ("cpm_entire", 16, 6, "distance", False, False, 5, "tstep"),
]


def test_seeded_cases_cover_what_they_claim():
    assert {c[3] for c in SEEDED} == {"distance", "ttc", "sparse", "distance_sparse", "ttc_sparse"}  # tools/fuzz_parity.py: REW
    assert {c[1] for c in SEEDED} == {1, 3, 4, 16, 17} and {c[4] for c in SEEDED} == {False, True}
    assert {c[7] for c in SEEDED} == {"single", "fused", "tstep"} and {c[6] for c in SEEDED} == {2, 3, 5} and any(c[5] for c in SEEDED)
    assert all(c[2] <= 40 for c in SEEDED)


@pytest.mark.parametrize("scen,N,B,rew,mtv,testing,ns,launch", SEEDED)
def test_hip_vs_oracle_seeded_perturbed(scen, N, B, rew, mtv, testing, ns, launch):
    import torch

    case = cr.Case(scen, N, B, rew, mtv=mtv, testing=testing, ns=ns, steps=24, dt=0.1 if scen != "cpm_entire" else 0.05)
    if launch == "single":
        rec = _lockstep(case)
    else:
        cfg, cc, mp = cr.build(case)
        dev, ora = _pair(cfg, mp)
        pf, pcn = int(mp.list_first[0]), int(mp.list_count[0])
        for e in (dev, ora):
            cr._mark_done(e)
            e.auto_reset(5, 0, pf, pcn)
        n_diff = tp._compare_all(dev, ora, "initial reset")
        rng = np.random.default_rng(case.seed)
        chunk = 1 if launch == "fused" else 4
        rewards = []
        for t0 in range(0, case.steps, chunk):
            acts = np.stack([cr.actions(rng, t0 + k, B, N) for k in range(chunk)])
            if launch == "fused":
                dev.step_autoreset(acts[0], 5, t0 + 1, pf, pcn)
            else:
                dev.env.step_autoreset_n(torch.as_tensor(acts).to(dev.env.device).contiguous(), seed=5, counter0=t0 + 1, path_first=pf, path_count=pcn)
                dev.env.sync()
            for k in range(chunk):
                ora.step(acts[k])
                ora.auto_reset(5, t0 + k + 1, pf, pcn)
            by = {}
            n_diff += tp._compare_all(dev, ora, f"{launch} launch at step {t0}", by)
            assert n_diff == 0, by
            rewards.append(ora.get(capi.BUF_REWARD))
        dev.close()
        ora.close()
        rec = {capi.BUF_REWARD: np.stack(rewards)}
    if not testing:
        assert (np.abs(rec[capi.BUF_REWARD]) < 1.0).mean() > 0.5  # the step reward is not on its final clamp in most entries


def test_auto_reset_alone_at_the_perturbed_constants():
    """The device-side sampler by itself: start speeds scale with max_speed (1.3), the minimum start distance with length and width."""
    for case in (cr.Case("cpm_entire", 16, 40, "distance"), cr.Case("intersection_1", 3, 33, "distance", testing=True, dt=0.1)):
        cfg, _, mp = cr.build(case)
        dev, ora = _pair(cfg, mp)
        pf, pcn = int(mp.list_first[0]), int(mp.list_count[0])
        for counter in range(3):
            for e in (dev, ora):
                cr._mark_done(e)
                e.auto_reset(11, counter, pf, pcn)
            assert tp._compare_all(dev, ora, f"{case} auto_reset {counter}") == 0
        st = ora.get(capi.BUF_STATE)
        if not case.testing:
            assert st[..., 3].max() > 1.0  # a start speed the default max_speed cannot produce
        d = np.linalg.norm(st[:, :, None, :2] - st[:, None, :, :2], axis=-1) + 10.0 * np.eye(case.N)
        assert d.min() >= 1.5 * np.hypot(cfg.length, cfg.width) * (1 - 1e-6) > 1.5 * np.hypot(0.22, 0.107)
        dev.close()
        ora.close()


def test_cbf_qp_deviation_reward_at_the_perturbed_constants():
    """rew_method "cbf" with is_solve_qp=True: the CBF-QP (asymmetric acceleration box: min_acc = -6, max_acc = 4; perturbed l_r, l_wb, speed / steering minima,
    covering circles of the longer vehicle) before every step, then the step's deviation penalty with two different weights and max_speed != 1 -- every buffer
    after every launch against the oracle, N = 3 and N = 16."""
    for N, B, steps in ((3, 6, 8), (16, 2, 4)):
        _lockstep(cr.Case("cpm_entire", N, B, "cbf", qp=True, steps=steps))


@pytest.mark.parametrize("name", list(cr.SWAP_CASES) + list(cr.REPLACE_CASES))
def test_mutant_on_the_device(name):
    """The CPU swap check's cases on the device: at the perturbed config and at the mutated one the device equals the oracle at that config, and the buffers named
    for the pair differ between the two device runs -- the device reads the member the oracle reads."""
    case, cfg, mut, what = cr.mutant_config(name)
    a, b = _lockstep(case, cfg), _lockstep(case, mut)
    n = cr.n_differing(a, b, what)
    assert all(k > 0 for k in n), (name, n)


@pytest.mark.parametrize("which", ["near_other_agents", "near_boundary", "ttc"])
def test_degenerate_thresholds_device_equals_oracle_word_for_word(which):
    """threshold_high == threshold_low (include/sigmaenv.h): NaN penalty channel, step reward -1 -- the same words on both sides, NaNs in the same places."""
    case = cr.Case("cpm_entire", 4, 3, "ttc" if which == "ttc" else "distance", steps=3)
    cfg, cc, mp = cr.build(case)
    cfg = host.degenerate_config(case, which)
    dev, ora = _pair(cfg, mp)

    def same(t):
        for w in tp.INT_BUFS + [x for x in tp.FLT_BUFS if x != capi.BUF_OBS]:
            x, y = dev.get(w), ora.get(w)
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (which, t, w)
        assert np.abs(dev.get(capi.BUF_OBS) - ora.get(capi.BUF_OBS)).max() <= tp.FTOL

    rec = cr.drive([ora, dev], cc, mp, case, after_step=same, after_reset=same)
    assert (rec[capi.BUF_REWARD] == -1.0).all()
    dev.close()
    ora.close()


# ---- the other device test bodies at the perturbed constants -----------------------------------------------------------------------------------------------------
# Those bodies build their configs with ``make_config`` / ``cbf.make_cbf_config`` and nothing else.  The hook below puts the perturbed set behind these two names
# for the duration of one test, in every module that bound them, so the bodies -- and their default-point tests -- stay as they are.
@pytest.fixture
def perturbed(monkeypatch):
    import sys

    import perturbed_constants as pc
    import sigmarl_amd.cbf as scbf
    import sigmarl_amd.params as sparams

    make_config, make_cbf_config = sparams.make_config, scbf.make_cbf_config
    made = []

    def perturbed_make_config(*a, **kw):
        cfg = pc.apply(make_config(*a, **kw))
        made.append(cfg)
        return cfg

    made_cbf = []

    def perturbed_make_cbf_config(*a, **kw):
        cc = make_cbf_config(*a, **kw)
        pc.apply_agents(None, pc.AGENTS, cc)
        made_cbf.append(cc)
        return cc

    for mod in list(sys.modules.values()):
        if getattr(mod, "make_config", None) is make_config:
            monkeypatch.setattr(mod, "make_config", perturbed_make_config)
    monkeypatch.setattr(scbf, "make_cbf_config", perturbed_make_cbf_config)
    yield made, made_cbf
    assert made and all(c.l_f != c.l_r and c.max_speed == np.float32(pc.AGENTS["max_speed"]) for c in made)  # the body did run at the perturbed set


@pytest.mark.parametrize("N,B", [(16, 33), (5, 33)])
def test_observation_fp64_bars_default_row(N, B, perturbed, monkeypatch):
    """test_gpu_observation's float64 bars (the normalisers r_pos, r_v, r_dl formed from cfg): n_nearing 1 / 2 / 4, the distance mask on (distance_mask_agents
    = 0.9, not 5 * length) and off, mtv on and off."""
    import test_gpu_observation as tobs

    tobs.test_step_kernel_default_row(N, B, False, monkeypatch)


@pytest.mark.parametrize("kw", [dict(is_ego_view=False), dict(is_ego_view=False, is_obs_steering=True, is_observe_vertices=False, is_observe_ref_path_other_agents=True)],
                         ids=["bird", "bird_novert_ref"])
def test_observation_fp64_bars_bird_view(kw, perturbed):
    import test_gpu_observation as tobs

    assert kw in tp.OBS_VARIANTS
    tobs.test_observation_variants(kw)


def test_restart_from_registers(perturbed, monkeypatch):
    """test_gpu_reset_core's chunk against single launches and the oracle at one of its cases: the sampler's minimum start distance from the perturbed length and
    width, its start speeds from max_speed = 1.3.  The case's own conditions (restarts before and in the last step, mixed tiles) are asserted by its body."""
    import test_gpu_reset_core as trc

    c = next(c for c in trc.CASES if c.name == "fixed_4x4")
    trc.test_restart_from_registers_chunk_against_single_launches_and_oracle(c, monkeypatch)


@pytest.mark.parametrize("N", [3, 16])
def test_cbf_qp_vs_oracle_and_kkt(N, perturbed):
    """test_gpu_cbf's body: minimiser, safe action and convergence against the oracle, and the KKT conditions of the original problem in numpy -- the oracle-independent
    check that the asymmetric acceleration box (-6, 4) is respected -- at the perturbed env config and perturbed l_r, l_wb, min_speed, min_steering, steering_rate_max."""
    import test_gpu_cbf as tcbf

    tcbf.test_cbf_qp_vs_oracle_and_kkt("rl", False, N)
    made, made_cbf = perturbed
    assert made_cbf and all(cc.l_r == pc_.AGENTS["l_r"] and cc.min_speed == np.float32(pc_.AGENTS["min_speed"]) for cc in made_cbf)


@pytest.mark.parametrize("case", [0, 2], ids=["cpm16", "intersection4_four_circles"])
def test_cbf_rollout_vs_oracle(case, perturbed):
    """test_gpu_cbf's margin rollout (is_solve_qp=False): margins, the three reward channels and the states after every step against the oracle."""
    import test_gpu_cbf as tcbf

    tcbf.test_cbf_rollout_vs_oracle(*tcbf.CASES[case])


def test_eval_planted_frames(perturbed):
    """One planted-frame case of test_gpu_eval on a handle created at the perturbed config.  (The evaluation kernels read the frames and no vehicle constant of the
    config -- the speed percentage divides by max_speed on the host, evaluate.summarize -- so this holds that the handle's config does not leak into them.)"""
    import test_gpu_eval as tev

    tev.test_planted_frames_equal_the_twin_and_hold_the_bars(*tev.vc.SHAPES[2])


def test_render_planted_frame(perturbed):
    """One planted frame of test_gpu_render against its twin on a handle created at the perturbed config (the renderer draws the vertices it is given)."""
    import test_gpu_render as trn

    trn.test_planted_frames_equal_the_twin_as_bytes("bracket")
