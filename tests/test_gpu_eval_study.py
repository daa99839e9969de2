"""The study metrics on the device (sigmaenv_eval_accumulate_study / sigmaenv_eval_study_finish, ``Evaluator(study=True)``, ``evaluate(study=True)``) held to
tests/eval_study_check.py.

1. planted frames through the overrides at (N, B, F) = (1,1,1), (3,5,2), (3,5,3), (6,3,37), (16,257,5), (33,2,4), (64,3,4) -- a group of one; padding lanes (3 -> 4,
   6 -> 8, 33 -> 64); G = 64; B off the envs per wavefront and per workgroup (257 = 64 x 4 + 1 at N = 16); F = 1, 2, 3: the initial frame only, the first difference
   only, the first jerk with a non-zero a_prev: accumulators, carry, metrics and counts equal the twin bit for bit and hold the derived bars of float64; the four old
   metrics of the same evaluator equal tests/eval_check.py's twin; a second pass after a reset gives the same bits (the carry is cleared).
2. frames with applied == nominal: degree and rate exactly 0.  After a reset and frames that are not initial, the task counters' snapshot is the reset's own.
3. a study evaluator and a plain one fed the same frames agree bit for bit on the four old metrics and their accumulators.
4. end to end, 4 agents x 8 envs x 6 frames and 16 x 64 x 4, with the CBF-QP attached under both values of is_apply_cbf_action (from an injected start), without
   CBF, and under wrapper="prioritized": ``evaluate(study=True)`` equals the composition written out (step, copy the buffers, the twin on the copies, auto-reset)
   bit for bit; records, trace and the four old metrics equal those of ``study=False`` bit for bit, and so does the state once that env takes the last step too; the
   task counters equal the timer buffer's differences; with the QP, activated and non-activated (env, agent, frame) both occur.  ``noise_sweep(study=True)``
   equals, group by group, the study evaluation of a handle of the group's envs alone.
5. the refusals on the device path."""
import ctypes as C

import numpy as np
import pytest

import eval_check as vc
import eval_study_check as sc

pytestmark = pytest.mark.gpu

LOW, HIGH = [-1.0, -0.6], [1.0, 0.6]
KW = dict(scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False)
PLAIN = ("state", "dist_ref", "col_agents", "col_flags")


def _env(N, B, **kw):
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters

    p = dict(KW, n_agents=N)
    p.update(kw)
    return SigmaEnv(Parameters(**p), n_envs=B, device="cuda:0")


def _got(ev, out):
    acc = ev.study_accumulators()
    return dict(sums=acc["sums"], n_act=acc["n_act"], carry=acc["carry"], frames=ev.accumulators()["frames"], metrics=out["metrics"].cpu().numpy(),
                counts=out["counts"].cpu().numpy().astype(np.uint32))


def _feed(env, ev, case, plain=None):
    """the case's frames through the overrides, each an allocation of its own; frame 0 as the initial one with the case's timer0; the env's timer set to timer1"""
    import torch
    from sigmarl_amd import capi

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    for f in range(case["F"]):
        kw = dict(applied=dev(case["applied"][f]), nominal=dev(case["nominal"][f]), reward_info=dev(case["reward_info"][f]))
        if plain is not None:
            kw.update({k: dev(plain[k][f]) for k in PLAIN})
        if f == 0:
            kw.update(timer=dev(case["timer0"]), initial=True)
        ev.accumulate(**kw)
    env.buffer(capi.BUF_TIMER).copy_(dev(case["timer1"]))


# ---- 1. planted frames ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B,F", sc.SHAPES)
def test_planted_frames_equal_the_twin_and_hold_the_bars(N, B, F):
    import torch
    from sigmarl_amd import capi
    from sigmarl_amd.evaluate import Evaluator

    env = _env(N, B)  # lends its handle: B, N and the launch; of its own buffers only the timer is read, at the finish
    case, plain = sc.make_case(N, B, F, seed=700 + N), vc.make_case(N, B, F, seed=500 + N)
    tw, ref = sc.twin(case), sc.reference64(case)
    ev = Evaluator(env, study=True)
    for rep in range(2):  # the second pass after a reset: the same bits
        ev.reset()
        _feed(env, ev, case, plain)
        out = ev.finish_study()
        got = _got(ev, out)
        bars = sc.check(got, case, ref=ref, tw=tw)
        print((N, B, F), bars, sc.figures(got, case))
        assert all(bars.values()), bars
        assert out["frames"] == F and out["count_names"] == capi.EVAL_STUDY_COUNTS
        for k, name in enumerate(capi.EVAL_STUDY_METRICS):
            assert torch.equal(out[name], out["metrics"][:, k])
        old = ev.accumulators()
        old["metrics"] = ev.finish()["metrics"].cpu().numpy()
        assert all(vc.check(old, plain).values())
        t0 = ev.study_accumulators()["timer0"]
        assert np.array_equal(t0, case["timer0"][:, 1:3])
    ev.close()
    env.close()


# ---- 2. applied == nominal ---------------------------------------------------------------------------------------------------------------------------
def test_applied_equal_to_nominal_gives_degree_and_rate_zero():
    from sigmarl_amd.evaluate import Evaluator

    N, B, F = 6, 5, 4
    env = _env(N, B)
    case = sc.make_case(N, B, F, seed=41, equal=True)
    ev = Evaluator(env, study=True)
    _feed(env, ev, case)
    out = ev.finish_study()
    m, c = out["metrics"].cpu().numpy(), out["counts"].cpu().numpy()
    assert (m[:, 3] == 0.0).all() and (m[:, 4] == 0.0).all() and (c[:, 0] == 0).all() and (c[:, 3] == F).all()
    assert (m[:, 2] < 0.0).all() and np.isfinite(m[:, :5]).all()
    assert all(sc.check(_got(ev, out), case).values())
    # without a nominal override and without the QP in the chain, the nominal action is the frame's applied action: the same result
    ev.reset()
    import torch

    for f in range(F):
        ev.accumulate(applied=torch.from_numpy(case["applied"][f]).cuda(), reward_info=torch.from_numpy(np.ascontiguousarray(case["reward_info"][f])).cuda(), initial=f == 0)
    out2 = ev.finish_study()
    assert vc.same_bits(out2["metrics"].cpu().numpy()[:, :5], m[:, :5])
    ev.close()
    env.close()


def test_the_reset_takes_the_snapshot_of_the_task_counters():
    """reset, then frames that are NOT initial: the snapshot is the one ``sigmaenv_eval_reset`` took from the env's timer buffer (columns 1 and 2, not 0 or 3), and
    tries / success are the buffer's differences against it at the finish"""
    import torch
    from sigmarl_amd import capi
    from sigmarl_amd.evaluate import Evaluator

    N, B, F = 3, 300, 2  # 300 envs: a second workgroup of the snapshot's launch (256 envs each)
    env = _env(N, B)
    case = sc.make_case(N, B, F, seed=77)
    timer = env.buffer(capi.BUF_TIMER)
    ev = Evaluator(env, study=True)
    timer.copy_(torch.from_numpy(case["timer0"]).cuda())
    ev.reset()
    timer.copy_(torch.from_numpy(case["timer0"] + 1000).cuda())  # later writes do not reach the snapshot
    for f in range(F):
        ev.accumulate(applied=torch.from_numpy(case["applied"][f]).cuda(), nominal=torch.from_numpy(case["nominal"][f]).cuda(),
                      reward_info=torch.from_numpy(np.ascontiguousarray(case["reward_info"][f])).cuda())
    timer.copy_(torch.from_numpy(case["timer1"]).cuda())
    out = ev.finish_study()
    acc, counts, m = ev.study_accumulators(), out["counts"].cpu().numpy(), out["metrics"].cpu().numpy()
    ref = sc.reference64(case)
    assert np.array_equal(acc["timer0"], case["timer0"][:, 1:3])
    assert not np.array_equal(case["timer0"][:, 1:3], case["timer0"][:, 0:2]) and not np.array_equal(case["timer0"][:, 1:3], case["timer0"][:, 2:4])
    assert np.array_equal(counts[:, 1], ref["tries"].astype(np.int32)) and np.array_equal(counts[:, 2], ref["success"].astype(np.int32)) and (counts[:, 3] == F).all()
    assert vc.same_bits(m[:, 5], ref["task_success_rate"]) and (ref["tries"] > 0).any() and (ref["tries"] == 0).any()
    assert (acc["carry"][..., 0] == case["applied"][F - 1][..., 0]).all()  # no initial frame: frame 0's command counted and carried
    ev.close()
    env.close()


# ---- 3. the plain evaluator is what it was -----------------------------------------------------------------------------------------------------------------
def test_a_study_evaluator_and_a_plain_one_agree_on_the_four_old_metrics():
    import torch
    from sigmarl_amd.evaluate import Evaluator

    N, B, F = 16, 70, 5
    env = _env(N, B)
    plain, case = vc.make_case(N, B, F, seed=9), sc.make_case(N, B, F, seed=10)
    a, b = Evaluator(env, study=True, trace_frames=F), Evaluator(env, trace_frames=F)
    _feed(env, a, case, plain)
    for f in range(F):
        b.accumulate(**{k: torch.from_numpy(np.ascontiguousarray(plain[k][f])).cuda() for k in PLAIN})
    fa, fb = a.finish(), b.finish()
    for k in ("metrics", "counts"):
        assert torch.equal(fa[k].view(torch.uint8), fb[k].view(torch.uint8)), k
    acc_a, acc_b = a.accumulators(), b.accumulators()
    for k in acc_a:
        assert vc.same_bits(acc_a[k], acc_b[k]), k
    assert torch.equal(a.trace().view(torch.uint8), b.trace().view(torch.uint8)) and all(vc.check(dict(acc_b, metrics=fb["metrics"].cpu().numpy()), plain).values())
    with pytest.raises(RuntimeError, match="without study"):
        b.finish_study()
    with pytest.raises(TypeError, match="study evaluator"):
        b.accumulate(initial=True)
    for x in (a, b, env):
        x.close()


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------------------------
CBF = dict(rew_method="cbf", is_solve_qp=True, is_using_cbf_training=True, dt=0.05, max_steps=5)
KINDS = {
    "cbf_applied": dict(pkw=dict(CBF, is_apply_cbf_action=True), roll=dict(), cbf=True, apply=True),
    "cbf_not_applied": dict(pkw=dict(CBF, is_apply_cbf_action=False), roll=dict(), cbf=True, apply=False),
    "no_cbf": dict(pkw=dict(is_testing_mode=True, max_steps=5), roll=dict()),
    "prioritized": dict(pkw=dict(is_using_prioritized_marl=True, max_steps=5), roll=dict(wrapper="prioritized", priority="random"), in_extra=True),
}


@pytest.mark.parametrize("N,B,T", [(4, 8, 6), (16, 64, 4)])
@pytest.mark.parametrize("kind", list(KINDS))
def test_evaluate_study_equals_the_composition_written_out(kind, N, B, T):
    import torch
    from sigmarl_amd import capi
    from sigmarl_amd.actor import Actor, make_mlp
    from sigmarl_amd.env import _buf_layout
    from sigmarl_amd.evaluate import evaluate, study_summary
    from sigmarl_amd.maps import injected_start

    c = KINDS[kind]
    seed, counter0 = 5, 40
    envs = [_env(N, B, **c["pkw"]) for _ in range(3)]  # study, plain, by hand
    if c.get("cbf"):
        for e in envs:
            e.cbf_attach()
    reset = (lambda e: e.reset_injected(*injected_start(e.map, e.N))) if c.get("cbf") else None
    torch.manual_seed(1)
    mlp = make_mlp(envs[0].D + (2 * envs[0].K if c.get("in_extra") else 0))
    with torch.no_grad():
        for m in mlp:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(1.7)
                m.bias.uniform_(-0.3, 0.3)
    actor = Actor(mlp, low=LOW, high=HIGH)
    W = N * (envs[0].D + 1) + 1
    rec = [dict(slab=torch.zeros(T - 1, B, W, device="cuda"), log_prob=torch.zeros(T - 1, B, N, device="cuda"), actions=torch.zeros(T - 1, B, N, 2, device="cuda")) for _ in range(2)]
    a = evaluate(envs[0], actor, n_steps=T, seed=seed, counter0=counter0, trace=True, study=True, reset=reset, **rec[0], **c["roll"])
    b = evaluate(envs[1], actor, n_steps=T, seed=seed, counter0=counter0, trace=True, reset=reset, **rec[1], **c["roll"])
    bits = lambda t: t.contiguous().view(torch.uint8)  # noqa: E731
    # study=False: records, trace and the four old metrics, and -- once that env takes the last step too -- the state
    assert "study" not in b and a["frames"] == b["frames"] == T
    for k in ("metrics", "counts", "trace"):
        assert torch.equal(bits(a[k]), bits(b[k])), k
    for k in rec[0]:
        assert torch.equal(bits(rec[0][k]), bits(rec[1][k])), k
    assert rec[0]["actions"].abs().max() > 0
    actor.rollout(envs[1], 1, seed=seed, counter0=counter0 + T, deterministic=True, **c["roll"])
    envs[0].sync()
    envs[1].sync()
    for which in _buf_layout(B, N, envs[0].K, envs[0].D):
        assert torch.equal(bits(envs[0].buffer(which)), bits(envs[1].buffer(which))), which
    # the composition written out: step, copy the buffers, auto-reset; the twin accumulates the copies on the host
    h = envs[2]
    if reset is not None:
        reset(h)
    else:
        h.reset_random(seed, counter=counter0 + T - 1)
    host = lambda which: h.buffer(which).cpu().numpy().copy()  # noqa: E731
    timer0 = host(capi.BUF_TIMER)
    qp = capi.nominal_from_cbf(h.parameters)
    assert qp == bool(c.get("cbf"))
    frames = dict(applied=[], nominal=[], reward_info=[])

    def take():
        frames["applied"].append(host(capi.BUF_ACTION))
        frames["nominal"].append(host(capi.BUF_CBF_NOMINAL if qp else capi.BUF_ACTION))
        frames["reward_info"].append(host(capi.BUF_REWARD_INFO))

    take()  # frame 0: whatever the buffers hold
    for t in range(T - 1):
        act = rec[0]["actions"][t].contiguous()
        if c.get("cbf"):
            safe = h.cbf_qp(act)
            act = safe if c["apply"] else act
        h.step(act)
        take()
        h.auto_reset(seed=seed, counter=counter0 + t)
    timer1 = envs[0].buffer(capi.BUF_TIMER).cpu().numpy()
    case = dict(N=N, B=B, F=T, timer0=timer0, timer1=timer1, replaced=np.zeros((T, B, N), bool), **{k: np.stack(v) for k, v in frames.items()})
    tw = sc.twin(case)
    st, acc = a["study"], a["study_accumulators"]
    got = dict(sums=acc["sums"], n_act=acc["n_act"], carry=acc["carry"], frames=np.full(B, T, np.uint32), metrics=st["metrics"].cpu().numpy(),
               counts=st["counts"].cpu().numpy().astype(np.uint32))
    print(kind, (N, B, T), "metrics[0]", got["metrics"][0].tolist(), "counts[0]", got["counts"][0].tolist())
    for k in got:
        assert vc.same_bits(got[k].astype(tw[k].dtype), tw[k]), k
    # the task counters are the timer buffer's differences over the whole rollout, its last (detached) step included
    assert np.array_equal(acc["timer0"], timer0[:, 1:3])
    assert np.array_equal(got["counts"][:, 1].astype(np.int64), (timer1[:, 1] - timer0[:, 1]).astype(np.int64))
    assert np.array_equal(got["counts"][:, 2].astype(np.int64), (timer1[:, 2] - timer0[:, 2]).astype(np.int64))
    M = T * N
    n_act = got["counts"][:, 0].astype(np.int64)
    if c.get("cbf"):  # both occur: the test cannot pass vacuously
        assert n_act.sum() > 0 and (M - n_act).sum() > 0, n_act
        assert (got["metrics"][:, 3] > 0).any()
    else:  # the nominal action is the applied one
        assert (n_act == 0).all() and (got["metrics"][:, 3] == 0).all() and (got["metrics"][:, 4] == 0).all()
    assert (got["metrics"][:, 2] < 0).all()  # the speed command moved: a comfort penalty
    s = study_summary(a)
    assert s["n_envs"] == B and s["frames"] == T and s["pooled"]["cbf_activation_rate"] == pytest.approx(100 * int(n_act.sum()) / (B * M))
    for x in (actor, *envs):
        x.close()


def test_noise_sweep_passes_study_through():
    """``noise_sweep(study=True)``: every group's study tensors and accumulators equal the study evaluation of a handle of those envs alone at the scalar level"""
    import torch
    from sigmarl_amd.actor import Actor, make_mlp
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.evaluate import evaluate, evaluation_parameters, noise_sweep, study_summary
    from sigmarl_amd.params import Parameters

    B, N, T, levels = 8, 4, 5, (0.05, 0.4)
    p = evaluation_parameters(Parameters(**dict(KW, n_agents=N, n_nearing_agents_observed=2, is_using_prioritized_marl=True)), simulation_steps=T + 1, num_envs=B)
    env = SigmaEnv(p, device="cuda:0")
    groups = [SigmaEnv(evaluation_parameters(p, num_envs=B // 2), device="cuda:0", env_index_base=b) for b in (0, B // 2)]
    torch.manual_seed(1)
    actor = Actor(make_mlp(env.D + 2 * env.K), low=LOW, high=HIGH)
    kw = dict(seed=7, counter0=30, wrapper="prioritized", priority="random", study=True)
    sweep = noise_sweep(env, actor, levels, **kw)
    for s, e, level in zip(sweep, groups, levels):
        one = evaluate(e, actor, communication_noise=level, **kw)
        for k in ("metrics", "counts"):
            assert vc.same_bits(s[k].cpu().numpy(), one[k].cpu().numpy()) and vc.same_bits(s["study"][k].cpu().numpy(), one["study"][k].cpu().numpy()), k
        for k, a in one["study_accumulators"].items():
            assert vc.same_bits(s["study_accumulators"][k], a), k
        assert vc.same_bits(s["study"]["comfort_reward"].cpu().numpy(), one["study"]["metrics"][:, 2].cpu().numpy()) and s["study"]["frames"] == T
        assert study_summary(s)["pooled"] == study_summary(one)["pooled"]
    assert not vc.same_bits(sweep[0]["study"]["metrics"].cpu().numpy(), sweep[1]["study"]["metrics"].cpu().numpy())
    for x in (actor, env, *groups):
        x.close()


# ---- 5. refusals on the device path ---------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device_path():
    from sigmarl_amd import capi
    from sigmarl_amd.evaluate import Evaluator

    N = 16
    env, other = _env(N, 3), _env(N, 3)
    ev, plain = Evaluator(env, study=True), Evaluator(env)
    lib = env.lib
    m = C.c_void_p(env.state.data_ptr())
    assert lib.eval_accumulate_study(other.h, ev.ev, None, None) == -22 and b"another handle" in lib.last_error(other.h)
    assert lib.eval_study_finish(other.h, ev.ev, m, None) == -22 and b"another handle" in lib.last_error(other.h)
    assert lib.eval_accumulate_study(None, ev.ev, None, None) == -22 and lib.eval_accumulate_study(env.h, None, None, None) == -22
    assert lib.eval_accumulate_study(env.h, plain.ev, None, None) == -22 and b"without study" in lib.last_error(env.h)
    assert lib.eval_study_finish(env.h, plain.ev, m, None) == -22 and b"without study" in lib.last_error(env.h)
    out = np.zeros(7 * 3)
    assert lib.eval_get(env.h, plain.ev, capi.EVAL_STUDY_SUMS, out.ctypes.data_as(C.c_void_p)) == -22 and b"without study" in lib.last_error(env.h)
    assert lib.eval_study_finish(env.h, ev.ev, None, None) == -22 and lib.eval_study_finish(env.h, ev.ev, C.c_void_p(env.state.data_ptr() + 2), None) == -22
    for field in ("applied", "nominal", "reward_info", "timer"):
        src = capi.EvalStudySrc()
        setattr(src, field, env.state.data_ptr() + 2)
        assert lib.eval_accumulate_study(env.h, ev.ev, None, C.byref(src)) == -22 and b"4-byte aligned" in lib.last_error(env.h), field
    src = capi.EvalStudySrc()
    src.initial = 2
    assert lib.eval_accumulate_study(env.h, ev.ev, None, C.byref(src)) == -22 and b"initial" in lib.last_error(env.h)
    args = capi.EvalArgs()
    args.study = 2
    p = C.c_void_p()
    assert lib.eval_create(env.h, C.byref(args), C.byref(p)) == -22 and not p.value
    assert ev.frames == 0 and plain.frames == 0
    # F N >= 2^24, through the reset's test hook
    limit = (1 << 24) // N
    full = Evaluator(env, _frames0=limit - 2, study=True)
    full.accumulate(initial=True)
    assert full.frames == limit - 1
    assert lib.eval_accumulate_study(env.h, full.ev, None, None) == -22 and b"2^24" in lib.last_error(env.h)
    with pytest.raises(ValueError, match="2\\^24"):
        full.accumulate()
    env.sync()
    for x in (full, ev, plain, env, other):
        x.close()
