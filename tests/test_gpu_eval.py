"""The evaluation metrics on the device (sigmaenv_eval_*, ``sigmarl_amd.evaluate``) held to tests/eval_check.py and to the reference's own trajectories.

1. planted frames through ``accumulate(overrides)`` + ``finish`` at (N, B, F) = (1,1,1), (3,5,2), (6,3,37), (16,257,5), (33,2,3), (64,3,4) -- one agent; lane groups
   with padding (3 -> 4, 6 -> 8, 33 -> 64); one env per wavefront (33, 64); B off the envs per wavefront and per workgroup (5 of 16 x 4, 3 of 8 x 4, 257 = 64 x 4 + 1
   at N = 16): accumulators and metrics equal the twin bit for bit and hold the derived bars, the trace equals the inputs word for word, frames beyond the trace's
   capacity are still accumulated.
2. the reference's trajectories replayed with ``accumulate()`` after the initial state and after every step, before the golden's reset events: counts and rates
   bit for bit against sigmarl/evaluation_base.py:205-217 in torch fp32 on the fixture's arrays, the two means within 1e-5 + F N 2^-24 max|term|.
3. ``Actor.rollout`` with an evaluator attached leaves what the fused rollout leaves, bit for bit, and accumulates what step / accumulate / auto_reset by hand do.
4. ``evaluate()``: repeatable, ``frames == T``, the metrics equal the float64 reduction of the trace within the bars, and sampling with another seed changes them.
5. the refusals on the device path."""
import ctypes as C

import numpy as np
import pytest

import eval_check as vc

pytestmark = pytest.mark.gpu

LOW, HIGH = [-1.0, -0.6], [1.0, 0.6]
KW = dict(scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False)


def _env(N, B, **kw):
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters

    p = dict(KW, n_agents=N)
    p.update(kw)
    return SigmaEnv(Parameters(**p), n_envs=B, device="cuda:0")


def _got(ev, out):
    got = ev.accumulators()
    got["metrics"] = out["metrics"].cpu().numpy()
    return got


# ---- 1. planted frames ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B,F", vc.SHAPES)
def test_planted_frames_equal_the_twin_and_hold_the_bars(N, B, F):
    import torch
    from sigmarl_amd.evaluate import Evaluator

    env = _env(N, B)  # lends its handle: B, N and the launch; its own buffers are never read
    case = vc.make_case(N, B, F, seed=500 + N)
    tw = vc.twin(case)
    # every frame an allocation of its own: an override is 4-byte aligned, which a frame sliced out of a stacked u8 tensor of odd size is not
    dev = {k: [torch.from_numpy(np.ascontiguousarray(case[k][f])).cuda() for f in range(F)] for k in ("state", "dist_ref", "col_agents", "col_flags")}
    cap = max(1, F - 1)  # the last frame lies beyond the trace's capacity (F >= 2)
    ev = Evaluator(env, trace_frames=cap)
    for rep in range(2):  # the second pass after a reset: the same bits
        ev.reset()
        for f in range(F):
            ev.accumulate(**{k: v[f] for k, v in dev.items()})
        out = ev.finish()
        got = _got(ev, out)
        bars = vc.check(got, case, tw=tw)
        print((N, B, F), bars, vc.figures(got, case))
        assert all(bars.values()), bars
        assert out["frames"] == F and (got["frames"] == F).all()
        counts = out["counts"].cpu().numpy()
        assert np.array_equal(counts[:, 0], tw["n_aa"]) and np.array_equal(counts[:, 1], tw["n_al"]) and (counts[:, 2] == F).all()
        for k, name in enumerate(("average_speed", "collision_rate_with_agents", "collision_rate_with_lanelets", "distance_ref_average")):
            assert torch.equal(out[name], out["metrics"][:, k])
        trace = ev.trace().numpy()
        assert trace.shape == (min(F, cap), B, N, 8) and vc.same_bits(trace, tw["trace"][:cap])
    ev.close()
    env.close()


# ---- 2. the reference's own trajectories ------------------------------------------------------------------------------------------------------------
class _Frames:
    """``traj_replay.replay``'s env with a frame taken after the initial state is set and after every step -- before the golden's reset events are applied"""

    def __init__(self, inner, ev):
        self._inner, self._ev, self._initial = inner, ev, True

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def observe(self):
        self._inner.observe()
        if self._initial:  # apply_initial_reset ends with observe(): the state after the initial reset
            self._initial = False
            self._ev.accumulate()

    def step(self, actions):
        self._inner.step(actions)
        self._ev.accumulate()


WINDOW_COUNTS = {"intersection5_6_testing": ([1, 1, 0], [6, 23, 5]), "onramp2_8_testing_mtv": ([0, 0, 0], [20, 26, 20]),
                 "intersection4_fixed_testing": ([1, 1, 2], [3, 12, 2]), "cpmmixed4_c2c": ([1, 0, 2, 0], [5, 8, 1, 5])}


@pytest.mark.parametrize("name", ["intersection5_6_testing", "intersection4_fixed_testing", "onramp2_8_testing_mtv", "cpmmixed4_c2c"])
def test_reference_trajectories(name):
    """Collision frames per env in the window init_*, post_*[0 : T - 1], counted on the CPU from the fixtures (agent-agent | agent-lanelet): intersection5_6_testing
    [1,1,0] | [6,23,5]; onramp2_8_testing_mtv [0,0,0] | [20,26,20]; intersection4_fixed_testing [1,1,2] | [3,12,2]; cpmmixed4_c2c [1,0,2,0] | [5,8,1,5].  (With the
    last step's outcome, which lies under ``next`` only and is NOT in the window, two fixtures would count one more: [6,23,6] and [20,27,21].)  The counts differ
    between envs, so a wrong window or a post-reset read shows."""
    import torch
    import oracle_binding as ob
    import traj_replay as tr
    from sigmarl_amd.env import NumpyAdapter, SigmaEnv
    from sigmarl_amd.evaluate import Evaluator

    z, meta = tr.load_fixture(name)
    cfg, mp = tr.config_from_meta(meta)
    T, B, N = int(meta["T"]), int(meta["B"]), int(cfg.n_agents)
    env = SigmaEnv(cfg=cfg, map_table=mp, device="cuda:0")
    ev = Evaluator(env)
    twin = ob.OracleEnv(cfg, mp)
    rep = tr.replay(_Frames(NumpyAdapter(env), ev), z, meta, mp, steps=T - 1, twin=twin)  # the initial state and the first T - 1 steps: T frames
    twin.close()
    out = ev.finish()
    metrics, counts = out["metrics"].cpu(), out["counts"].cpu().numpy()
    ev.close()
    env.close()
    assert rep.total_mismatch() == 0, str(rep)
    # evaluation_base.py:191-217 on the fixture's arrays: out_td's root entries are init_*, then post_*[0 : T - 1]
    stack = lambda k: torch.from_numpy(np.concatenate([z["init_" + k][None], z["post_" + k][: T - 1]])).transpose(0, 1)  # noqa: E731  [B, T, ..]
    velocities, distance_ref = stack("vel").float(), stack("dist_ref").float().unsqueeze(-1)
    with_agents, with_lanelets = stack("col_agents").bool().any(dim=-1, keepdim=True), stack("col_lane").bool().unsqueeze(-1)
    num_steps = velocities.shape[1]
    assert num_steps == T and out["frames"] == T
    want = torch.stack([velocities.norm(dim=-1).mean(dim=(-2, -1)), with_agents.squeeze(-1).any(dim=-1).sum(dim=-1) / num_steps,
                        with_lanelets.squeeze(-1).any(dim=-1).sum(dim=-1) / num_steps, distance_ref.squeeze(-1).mean(dim=(-2, -1))], dim=1)
    n_aa, n_al = with_agents.squeeze(-1).any(dim=-1).sum(dim=-1).numpy(), with_lanelets.squeeze(-1).any(dim=-1).sum(dim=-1).numpy()
    assert (n_aa.tolist(), n_al.tolist()) == WINDOW_COUNTS[name]  # the window is the one the docstring counts
    # The reference's env-0 reset quirk (traj_replay.replay) shows in the snapshot taken right AFTER a step's resets, which is never a frame: the frames are the
    # post-step states, and replay compares those in every env.  With the quirk-free oracle as its twin replay leaves no env unchecked; one that it did leave
    # unchecked would be hidden here too, and more than one fails.
    hidden = getattr(rep, "unchecked", 0)
    assert hidden == 0, hidden
    envs = list(range(B))
    print(name, "frames", T, "n_aa", n_aa, "n_al", n_al, "hidden", hidden, "metrics", metrics.numpy().tolist(), "want", want.numpy().tolist())
    assert np.array_equal(counts[envs, 0], n_aa[envs]) and np.array_equal(counts[envs, 1], n_al[envs]) and (counts[:, 2] == T).all()
    assert torch.equal(metrics[envs, 1].view(torch.int32), want[envs, 1].view(torch.int32)) and torch.equal(metrics[envs, 2].view(torch.int32), want[envs, 2].view(torch.int32))
    for col, terms in ((0, velocities.norm(dim=-1)), (3, distance_ref)):
        bar = 1e-5 + T * N * 2.0 ** -24 * float(terms.abs().max())
        err = (metrics[envs, col].double() - want[envs, col].double()).abs().max()
        print(name, "column", col, "err", float(err), "bar", bar)
        assert float(err) <= bar, (col, float(err), bar)
    if name != "onramp2_8_testing_mtv":
        assert n_aa.any() and len(set(n_al.tolist())) > 1  # counts that differ between envs: a wrong window or a post-reset read shows


# ---- 3. attached equals fused ------------------------------------------------------------------------------------------------------------------------
CASES = {
    "testing_4x6": dict(N=4, B=6, pkw=dict(scenario_type="intersection_1", is_testing_mode=True), roll=dict()),
    "training_16x5": dict(N=16, B=5, pkw=dict(max_steps=5), roll=dict()),
    "opponent": dict(N=16, B=5, pkw=dict(is_using_opponent_modeling=True, max_steps=5), roll=dict(wrapper="opponent")),
    "prioritized_random": dict(N=16, B=5, pkw=dict(is_using_prioritized_marl=True, max_steps=5), roll=dict(wrapper="prioritized", priority="random"), in_extra=True),
    "cbf_qp": dict(N=4, B=6, pkw=dict(rew_method="cbf", is_solve_qp=True, is_using_cbf_training=True, is_apply_cbf_action=True, dt=0.05, max_steps=5), roll=dict(), cbf=True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_attached_rollout_equals_the_fused_one_and_the_steps_by_hand(case):
    import torch
    from sigmarl_amd.actor import Actor, make_mlp
    from sigmarl_amd.env import _buf_layout
    from sigmarl_amd.evaluate import Evaluator

    c = CASES[case]
    N, B, T, seed, counter0 = c["N"], c["B"], 12, 5, 40
    envs = [_env(N, B, **c["pkw"]) for _ in range(3)]  # fused, attached, by hand
    for e in envs:
        e.reset_random(seed=3)
        if c.get("cbf"):
            e.cbf_attach()
    torch.manual_seed(1)
    mlp = make_mlp(envs[0].D + (2 * envs[0].K if c.get("in_extra") else 0))
    with torch.no_grad():
        for m in mlp:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(1.7)
                m.bias.uniform_(-0.3, 0.3)
    actor = Actor(mlp, low=LOW, high=HIGH)
    W, D = N * (envs[0].D + 1) + 1, envs[0].D
    rec = [dict(slab=torch.zeros(T, B, W, device="cuda"), log_prob=torch.zeros(T, B, N, device="cuda"), actions=torch.zeros(T, B, N, 2, device="cuda"),
                obs_rec=torch.zeros(T, B, N, D, device="cuda")) for _ in range(2)]
    actor.rollout(envs[0], T, seed=seed, counter0=counter0, **rec[0], **c["roll"])
    ev = Evaluator(envs[1])
    with ev.attached():
        actor.rollout(envs[1], T, seed=seed, counter0=counter0, **rec[1], **c["roll"])
    envs[0].sync()
    envs[1].sync()
    bits = lambda t: t.contiguous().view(torch.uint8)  # noqa: E731
    for k in rec[0]:
        assert torch.equal(bits(rec[0][k]), bits(rec[1][k])), k
    for which in _buf_layout(B, N, envs[0].K, D):
        assert torch.equal(bits(envs[0].buffer(which)), bits(envs[1].buffer(which))), which
    assert ev.frames == T
    # detached again: the next rollout takes no frame
    actor.rollout(envs[1], 1, seed=seed, counter0=counter0 + T, **c["roll"])
    assert ev.frames == T
    attached = ev.accumulators()
    # the same actions by hand: step, accumulate, auto_reset (the QP's safe action where the chain uses it)
    hand = Evaluator(envs[2])
    for t in range(T):
        act = rec[1]["actions"][t].contiguous()
        envs[2].step(envs[2].cbf_qp(act) if c.get("cbf") else act)
        hand.accumulate()
        envs[2].auto_reset(seed=seed, counter=counter0 + t)
    by_hand = hand.accumulators()
    print(case, attached)
    for k in attached:
        assert vc.same_bits(attached[k], by_hand[k]), k
    assert (attached["frames"] == T).all() and attached["sum_speed"].min() > 0.0
    m_a, m_h = ev.finish()["metrics"], hand.finish()["metrics"]
    assert torch.equal(bits(m_a), bits(m_h))
    for x in (ev, hand, actor, *envs):
        x.close()


# ---- 4. evaluate() -----------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_is_repeatable_counts_t_frames_and_equals_its_trace():
    import torch
    from sigmarl_amd import capi
    from sigmarl_amd.actor import Actor, make_mlp
    from sigmarl_amd.evaluate import evaluate, evaluation_parameters
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters

    N, B, T = 6, 9, 20
    p = evaluation_parameters(Parameters(**dict(KW, scenario_type="intersection_1", n_agents=4)), n_agents=N, simulation_steps=T + 1, num_envs=B)
    assert p.is_testing_mode and p.max_steps - 1 == T
    env = SigmaEnv(p, device="cuda:0")
    assert (env.B, env.N) == (B, N)
    torch.manual_seed(2)
    actor = Actor(make_mlp(env.D), low=LOW, high=HIGH)
    a = evaluate(env, actor, seed=7, trace=True)
    b = evaluate(env, actor, seed=7, trace=True)
    assert a["frames"] == b["frames"] == T and (a["counts"][:, 2] == T).all()
    for k in ("metrics", "counts", "trace"):
        assert torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)), k
    assert set(capi.EVAL_METRICS) <= set(a) and a["count_names"] == capi.EVAL_COUNTS and a["trace"].shape == (T, B, N, 8)
    # the float64 reduction of the trace, within the bars of the yardstick (the trace's speed column is the fp32 term: the reference is taken from vx, vy)
    tr = a["trace"].numpy()
    case = dict(N=N, B=B, F=T, state=np.zeros((T, B, N, 8), np.float32), dist_ref=tr[..., 4].copy(), col_agents=np.zeros((T, B, N, N), np.uint8),
                col_flags=np.zeros((T, B, N, 4), np.uint8))
    case["state"][..., 0:2], case["state"][..., 5], case["state"][..., 6] = tr[..., 0:2], tr[..., 2], tr[..., 3]
    case["col_agents"][..., 0] = tr[..., 6] != 0  # (which agent an agent collided with is not traced: any column gives the same frame flag)
    case["col_flags"][..., 0] = tr[..., 7] != 0
    ref = vc.reference64(case)
    m = a["metrics"].cpu().numpy()
    print("evaluate", m.tolist(), "n_aa", ref["n_aa"], "n_al", ref["n_al"])
    assert (np.abs(m[:, 0] - ref["m0"]) <= ref["bar0"]).all() and (np.abs(m[:, 3] - ref["m3"]) <= ref["bar3"]).all()
    assert vc.same_bits(m[:, 1], ref["m1"]) and vc.same_bits(m[:, 2], ref["m2"])
    assert np.array_equal(a["counts"].cpu().numpy()[:, :2], np.stack([ref["n_aa"], ref["n_al"]], axis=1).astype(np.int32))
    assert vc.same_bits(m, vc.twin(case)["metrics"])
    assert (m[:, 0] > 0).all() and np.isfinite(m).all()
    # sampling with another seed changes the metrics
    s = evaluate(env, actor, seed=8, deterministic=False)
    assert s["frames"] == T and not torch.equal(s["metrics"], a["metrics"])
    actor.close()
    env.close()


# ---- 5. refusals on the device path ---------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device_path():
    from sigmarl_amd.actor import Actor, make_mlp
    from sigmarl_amd.evaluate import Evaluator

    N = 16
    env, other = _env(N, 3), _env(N, 3)
    ev = Evaluator(env)
    lib = env.lib
    for call in (lambda: lib.eval_accumulate(other.h, ev.ev, None), lambda: lib.eval_attach(other.h, ev.ev), lambda: lib.eval_reset(other.h, ev.ev),
                 lambda: lib.eval_finish(other.h, ev.ev, C.c_void_p(env.state.data_ptr()), None)):
        assert call() == -22 and b"another handle" in lib.last_error(other.h)
    assert lib.eval_accumulate(None, ev.ev, None) == -22 and lib.eval_accumulate(env.h, None, None) == -22 and b"null evaluator" in lib.last_error(env.h)
    assert ev.frames == 0
    from sigmarl_amd import capi

    src = capi.EvalSrc()
    src.dist_ref = env.state.data_ptr() + 2
    assert lib.eval_accumulate(env.h, ev.ev, C.byref(src)) == -22 and b"4-byte aligned" in lib.last_error(env.h) and ev.frames == 0
    # a frame count that would reach 2^24 / N, set through the test hook of the reset
    limit = (1 << 24) // N
    full = Evaluator(env, _frames0=limit - 2)
    assert full.frames == limit - 2
    full.accumulate()                      # (limit - 1) * N < 2^24: the last frame that fits
    assert full.frames == limit - 1 and (full.accumulators()["frames"] == limit - 1).all()
    assert lib.eval_accumulate(env.h, full.ev, None) == -22 and b"2^24" in lib.last_error(env.h)
    with pytest.raises(ValueError, match="2\\^24"):
        full.accumulate()
    full.reset()
    assert full.frames == limit - 2
    env.reset_random(seed=1)
    actor = Actor(make_mlp(env.D), low=LOW, high=HIGH)
    with full.attached():                  # an attached rollout is refused before its first launch if it could not take all its frames
        with pytest.raises(RuntimeError, match="2\\^24"):
            actor.rollout(env, 2)
        assert full.frames == limit - 2
        actor.rollout(env, 1)
        assert full.frames == limit - 1
    env.sync()
    for x in (full, ev, actor, env, other):
        x.close()
