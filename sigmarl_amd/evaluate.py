"""Evaluation of a trained policy on the device: the reference's four metrics per env and their summary.

The reference evaluates a model in ``sigmarl/evaluation_base.py``: ``_adjust_parameters`` (:153-182) switches to testing mode with ``max_steps = simulation_steps``
and many parallel envs, ``_get_simulation_outputs`` (:271-282) makes ONE ``env.rollout(max_steps - 1, policy, break_when_any_done=False)``, ``_evaluate_model_i``
(:184-217) reduces five ``info`` entries of its output to four numbers per env, and ``compute_performance_metrics`` / ``_log`` (:670-760) summarise them.

Here ``Evaluator`` owns the per-env accumulators on the device (``sigmaenv_eval_*``, include/sigmaenv.h; the arithmetic: csrc/sigmaenv_eval.h), ``evaluate`` is the
rollout with the evaluator attached, ``noise_sweep`` is that rollout over a sweep of communication-noise levels, and ``summarize`` / ``composite_score`` are the
summary as host torch on ``[B]`` vectors.

The frame window of ``evaluate`` -- which moments are counted -- restates torchrl's rollout from its published behaviour (torchrl is third-party and absent, as for
GAE and ``RewardSum``): ``out_td["agents", "info", .]`` holds the ROOT entries of the ``T`` stacked tensordicts, and the root entries are the info after the reset,
then ``step_mdp(keep_other=True)`` of each step's ``next`` (``sigmarl/helper_training.py:271-279`` and its non-stop twin).  So the window is ``T`` frames: the initial
state, and the state after each of the first ``T - 1`` steps, taken BEFORE that step's re-placements (testing mode re-places collided agents inside ``done()``,
``road_traffic.py:1435-1447``, after ``info()`` was read).  The last step's outcome lies under ``next`` only and is not counted: ``evaluate`` does not run that step.
``num_steps = positions.shape[1] = T`` (:203).  ``Evaluator.accumulate`` itself takes no position on the window: a caller who wants another one composes it from
``env.step`` / ``accumulate`` / ``env.auto_reset``.

The study of a CBF-filtered policy (``study=True``; ``sigmarl/evaluation_itsc26.py``): the same window reduced to six more numbers per env --
``compute_total_reward`` (:926-992), ``compute_cbf_activation_percentage`` (:995-1035) and the task counters (:883-898, :1450-1458).  The reference runs it with
ONE env per process (:807-879); here every env of the batch is such a run (``finish_study``), and ``study_summary`` also gives what ONE reference run of all ``B``
envs would print.  Frame 0 is the reference's root info after the reset: the zeros of a fresh scenario (``road_traffic.py:670-675, 1522-1545``), whatever the
buffers hold.  The reference's ``rollout(max_steps - 1)`` runs ``T`` steps, of which the last counts for the task counters but not for ``out_td``:
``evaluate(study=True)`` runs that step too, detached.
"""
from __future__ import annotations

import contextlib
import copy
import ctypes as C

import numpy as np
import torch

from . import capi

MAX_TERMS = capi.EVL_MAX_TERMS


def group_lanes(n_agents: int) -> int:
    """``evl_group``: the lane group of an env, the smallest power of two >= N."""
    g = 1
    while g < int(n_agents):
        g <<= 1
    return g


def eval_src(env, frames: int, state_ptr=None, dist_ref_ptr=None, col_agents_ptr=None, col_flags_ptr=None):
    """The library's refusals of one more frame, made on the host before the call, and the ``sigmaenv_eval_src_t`` of the overrides (``None`` without any):
    raw device addresses, each 4-byte aligned; ``frames`` = the frames accumulated so far."""
    if (int(frames) + 1) * int(env.N) >= MAX_TERMS:
        raise ValueError(f"evaluation: (frames + 1) * n_agents = {(int(frames) + 1) * int(env.N)} would reach 2^24 (the counts are reported through floats): finish and reset first")
    ptrs = dict(state=state_ptr, dist_ref=dist_ref_ptr, col_agents=col_agents_ptr, col_flags=col_flags_ptr)
    if all(p is None for p in ptrs.values()):
        return None
    src = capi.EvalSrc()
    for name, p in ptrs.items():
        if p is None:
            continue
        if int(p) == 0 or int(p) & 3:
            raise ValueError(f"evaluation: the {name} override is null or not 4-byte aligned")
        setattr(src, name, int(p))
    return src


_RECORDS = ("slab", "log_prob", "actions", "slab_ptr", "tentative", "ranks", "scores", "score_log_prob", "obs_rec", "base_obs")  # Actor.rollout's record arguments


def eval_study_src(applied_ptr=None, nominal_ptr=None, reward_info_ptr=None, timer_ptr=None, initial: bool = False):
    """The ``sigmaenv_eval_study_src_t`` of a study frame's overrides and its ``initial`` flag (``None`` without any and not initial): raw device addresses, each
    4-byte aligned -- the library's refusals, made on the host before the call."""
    ptrs = dict(applied=applied_ptr, nominal=nominal_ptr, reward_info=reward_info_ptr, timer=timer_ptr)
    if all(p is None for p in ptrs.values()) and not initial:
        return None
    src = capi.EvalStudySrc()
    for name, p in ptrs.items():
        if p is None:
            continue
        if int(p) == 0 or int(p) & 3:
            raise ValueError(f"evaluation: the {name} override is null or not 4-byte aligned")
        setattr(src, name, int(p))
    src.initial = int(bool(initial))
    return src


class Evaluator:
    """The accumulators ``[B]`` of one env (``sigmaenv_eval_create``): two fp64 sums, two collision-frame counts and the frame count; with ``trace_frames > 0`` also
    a device trace ``[trace_frames, B, N, 8]`` (``capi.EVAL_TRACE_FIELDS``) of the first frames after a reset.  Nothing but ``trace()`` / ``accumulators()`` waits.
    ``study=True``: a study evaluator -- every frame also adds to seven more fp64 sums and the activation count, through a carry ``[B, N, 2]`` of the previous speed
    command and acceleration (``finish_study``); the four metrics and everything else are those of a plain evaluator, bit for bit."""

    def __init__(self, env, trace_frames: int = 0, _frames0: int = 0, study: bool = False):
        self.env, self.trace_frames, self.study = env, int(trace_frames), bool(study)
        self.ev = None
        args = capi.EvalArgs()
        args.trace_frames, args.debug_frames0 = self.trace_frames, int(_frames0)  # (_frames0: the library's test hook, see include/sigmaenv.h)
        args.study = int(self.study)
        ev = C.c_void_p()
        with torch.cuda.device(env.device):
            env._chk(env.lib.eval_create(env.h, C.byref(args), C.byref(ev)), "eval_create")
        self.ev = ev

    # ---- plumbing ---------------------------------------------------------------------------------------------
    def _check(self, t, dtype, shape, what):
        if t is None:
            return None
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
            raise TypeError(f"evaluation: {what} must be a contiguous {dtype} CUDA tensor {list(shape)}")
        return t.data_ptr()

    @property
    def frames(self) -> int:
        """frames accumulated since the last reset, as the host counts them (no wait)"""
        n = C.c_uint64()
        self.env._chk(self.env.lib.eval_get(self.env.h, self.ev, capi.EVAL_FRAMES_HOST, C.byref(n)), "eval_get")
        return int(n.value)

    def close(self):
        if getattr(self, "ev", None) and getattr(self.env, "h", None):
            self.env.lib.eval_destroy(self.ev)
        self.ev = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ---- the calls ----------------------------------------------------------------------------------------------
    def reset(self):
        self.env._chk(self.env.lib.eval_reset(self.env.h, self.ev), "eval_reset")

    def accumulate(self, state=None, dist_ref=None, col_agents=None, col_flags=None, applied=None, nominal=None, reward_info=None, timer=None, initial: bool = False):
        """One frame for every env, one launch: the env's buffers as they stand, or -- per argument -- a tensor of the same layout in their place
        (``state [B,N,8]`` f32, ``dist_ref [B,N]`` f32, ``col_agents [B,N,N]`` u8, ``col_flags [B,N,4]`` u8), each starting on a 4-byte boundary (a tensor of its
        own does; a frame sliced out of a stacked uint8 tensor of odd size may not).  A study evaluator only: ``applied`` / ``nominal [B,N,2]`` f32,
        ``reward_info [12,B,N]`` f32 (rows ``capi.EVL_REW_ROWS`` are read), ``timer [B,4]`` i32 in place of the env's buffers, and ``initial=True`` for the frame
        after the reset: zero actions and event reward whatever the buffers hold, a zero carry, and the task counters' snapshot retaken from the timer."""
        e = self.env
        if self.study:
            src = eval_src(e, self.frames, self._check(state, torch.float32, (e.B, e.N, 8), "state"), self._check(dist_ref, torch.float32, (e.B, e.N), "dist_ref"),
                           self._check(col_agents, torch.uint8, (e.B, e.N, e.N), "col_agents"), self._check(col_flags, torch.uint8, (e.B, e.N, 4), "col_flags"))
            ssrc = eval_study_src(self._check(applied, torch.float32, (e.B, e.N, 2), "applied"), self._check(nominal, torch.float32, (e.B, e.N, 2), "nominal"),
                                  self._check(reward_info, torch.float32, (len(capi.REWARD_INFO_FIELDS), e.B, e.N), "reward_info"),
                                  self._check(timer, torch.int32, (e.B, 4), "timer"), initial)
            e._chk(e.lib.eval_accumulate_study(e.h, self.ev, C.byref(src) if src is not None else None, C.byref(ssrc) if ssrc is not None else None), "eval_accumulate_study")
            return
        if applied is not None or nominal is not None or reward_info is not None or timer is not None or initial:
            raise TypeError("evaluation: applied / nominal / reward_info / timer / initial belong to a study evaluator (Evaluator(env, study=True))")
        src = eval_src(e, self.frames, self._check(state, torch.float32, (e.B, e.N, 8), "state"), self._check(dist_ref, torch.float32, (e.B, e.N), "dist_ref"),
                       self._check(col_agents, torch.uint8, (e.B, e.N, e.N), "col_agents"), self._check(col_flags, torch.uint8, (e.B, e.N, 4), "col_flags"))
        e._chk(e.lib.eval_accumulate(e.h, self.ev, C.byref(src) if src is not None else None), "eval_accumulate")

    @contextlib.contextmanager
    def attached(self):
        """While inside, every step of ``Actor.rollout`` on this env runs as step -> accumulate -> auto_reset (``sigmaenv_eval_attach``); always detaches."""
        self.env._chk(self.env.lib.eval_attach(self.env.h, self.ev), "eval_attach")
        try:
            yield self
        finally:
            self.env._chk(self.env.lib.eval_attach(self.env.h, None), "eval_attach")

    def finish(self) -> dict:
        """``metrics [B,4]`` float32 and its columns under the reference's attribute names (``capi.EVAL_METRICS``), ``counts [B,3]`` int32 (``capi.EVAL_COUNTS``)
        with ``count_names``, and ``frames`` (host int).  Device tensors; the accumulators stay as they are."""
        e = self.env
        metrics = torch.empty((e.B, 4), dtype=torch.float32, device=e.device)
        counts = torch.empty((e.B, 3), dtype=torch.int32, device=e.device)
        e._chk(e.lib.eval_finish(e.h, self.ev, C.c_void_p(metrics.data_ptr()), C.c_void_p(counts.data_ptr())), "eval_finish")
        out = {"metrics": metrics, "counts": counts, "count_names": capi.EVAL_COUNTS, "frames": self.frames}
        for k, name in enumerate(capi.EVAL_METRICS):
            out[name] = metrics[:, k]
        return out

    def finish_study(self) -> dict:
        """A study evaluator's ``metrics [B,6]`` float32 and its columns under ``capi.EVAL_STUDY_METRICS``, ``counts [B,4]`` int32 (``capi.EVAL_STUDY_COUNTS``) with
        ``count_names``, and ``frames``.  The task counters are read as the env's timer holds them when the launch runs.  Device tensors; nothing waits."""
        e = self.env
        if not self.study:
            raise RuntimeError("evaluation: the evaluator was created without study (Evaluator(env, study=True))")
        metrics = torch.empty((e.B, len(capi.EVAL_STUDY_METRICS)), dtype=torch.float32, device=e.device)
        counts = torch.empty((e.B, len(capi.EVAL_STUDY_COUNTS)), dtype=torch.int32, device=e.device)
        e._chk(e.lib.eval_study_finish(e.h, self.ev, C.c_void_p(metrics.data_ptr()), C.c_void_p(counts.data_ptr())), "eval_study_finish")
        out = {"metrics": metrics, "counts": counts, "count_names": capi.EVAL_STUDY_COUNTS, "frames": self.frames}
        for k, name in enumerate(capi.EVAL_STUDY_METRICS):
            out[name] = metrics[:, k]
        return out

    def study_accumulators(self) -> dict:
        """A study evaluator's own accumulators as host arrays (waits): ``sums`` float64 ``[7,B]`` and its rows under ``capi.EVAL_STUDY_SUM_NAMES``, ``n_act`` uint32
        ``[B]``, ``carry`` float32 ``[B,N,2]`` (v_prev, a_prev), ``timer0`` int32 ``[B,2]`` (the task counters' snapshot)."""
        e, out = self.env, {}
        if not self.study:
            raise RuntimeError("evaluation: the evaluator was created without study (Evaluator(env, study=True))")
        for name, what, dt, shape in (("sums", capi.EVAL_STUDY_SUMS, np.float64, (len(capi.EVAL_STUDY_SUM_NAMES), e.B)), ("n_act", capi.EVAL_STUDY_N_ACT, np.uint32, (e.B,)),
                                      ("carry", capi.EVAL_STUDY_CARRY, np.float32, (e.B, e.N, 2)), ("timer0", capi.EVAL_STUDY_TIMER0, np.int32, (e.B, 2))):
            a = np.zeros(shape, dt)
            e._chk(e.lib.eval_get(e.h, self.ev, what, a.ctypes.data_as(C.c_void_p)), "eval_get")
            out[name] = a
        for k, name in enumerate(capi.EVAL_STUDY_SUM_NAMES):
            out[name] = out["sums"][k]
        return out

    def accumulators(self) -> dict:
        """The accumulators as host arrays (waits): ``sum_speed`` / ``sum_dref`` float64 ``[B]``, ``n_aa`` / ``n_al`` / ``frames`` uint32 ``[B]``."""
        e, out = self.env, {}
        for name, what, dt in (("sum_speed", capi.EVAL_SUM_SPEED, np.float64), ("sum_dref", capi.EVAL_SUM_DREF, np.float64), ("n_aa", capi.EVAL_N_AA, np.uint32),
                               ("n_al", capi.EVAL_N_AL, np.uint32), ("frames", capi.EVAL_FRAMES, np.uint32)):
            a = np.zeros(e.B, dt)
            e._chk(e.lib.eval_get(e.h, self.ev, what, a.ctypes.data_as(C.c_void_p)), "eval_get")
            out[name] = a
        return out

    def trace(self) -> torch.Tensor:
        """The traced frames as a host tensor ``[min(frames, trace_frames), B, N, 8]`` (waits)."""
        e = self.env
        if self.trace_frames < 1:
            raise RuntimeError("evaluation: the evaluator was created without a trace (trace_frames=0)")
        a = np.zeros((self.trace_frames, e.B, e.N, capi.EVL_TRACE_COLS), np.float32)
        e._chk(e.lib.eval_get(e.h, self.ev, capi.EVAL_TRACE, a.ctypes.data_as(C.c_void_p)), "eval_get")
        return torch.from_numpy(a[: min(self.frames, self.trace_frames)])


def evaluation_parameters(p, n_agents: int | None = None, simulation_steps: int | None = None, num_envs: int | None = None):
    """A copy of ``p`` with the changes of ``_adjust_parameters`` (evaluation_base.py:153-182) that reach the env: testing mode, ``max_steps = simulation_steps``,
    ``num_vmas_envs``, ``n_agents``, and the two training-only switches off."""
    q = copy.deepcopy(p)
    q.is_testing_mode = True
    if n_agents is not None:
        q.n_agents = int(n_agents)
    if simulation_steps is not None:
        q.max_steps = int(simulation_steps)
    if num_envs is not None:
        q.num_vmas_envs = int(num_envs)
    q.is_prb = False
    q.is_challenging_initial_state_buffer = False
    return q


def evaluate(env, actor, params=None, n_steps: int | None = None, seed: int = 0, counter0: int = 0, deterministic: bool = True, trace: bool = False, study: bool = False,
             reset=None, render=None, render_every: int = 1, **rollout_kw) -> dict:
    """The reference's evaluation rollout on the device.  ``T = n_steps or params.max_steps - 1`` frames (``params`` defaults to ``env.parameters``): in this order
    ``env.reset_random(seed)`` -- its draws keyed by the counter ``counter0 + T - 1``, the first one the rollout's steps ``counter0 .. counter0 + T - 2`` do not use, so
    that the result is a function of the arguments alone --, ``Evaluator.reset()``, ``accumulate()`` of the state after the initial reset, ``actor.rollout`` of ``T - 1`` steps with the evaluator
    attached, ``finish()`` -- the window the module docstring derives.  The reference sets no exploration type for this rollout; ``deterministic=True`` is the default
    here and is passed through to ``Actor.rollout``, as is ``rollout_kw`` (``wrapper=``, ``priority=``, ``precision=``, ``communication_noise=`` ..; the noise is drawn
    although the actions are deterministic, as in the reference's evaluation rollout, helper_training.py:230-243).  Returns ``finish()``'s dict, plus ``trace``
    (host ``[T, B, N, 8]``) when asked for.  ``reset``: a callable ``reset(env)`` that makes the initial reset in place of ``env.reset_random`` (an injected start:
    ``lambda e: e.reset_injected(*maps.injected_start(e.map, e.N))``).

    ``study=True`` (evaluation_itsc26.py): a study evaluator takes the same ``T`` frames, the first as the initial one; then ONE more step runs, detached and without
    the caller's records (``rollout_kw`` less ``slab=``, ``actions=`` ..), keyed ``counter0 + T`` (``counter0 + T - 1`` is the reset's) -- the last step of the
    reference's ``rollout(max_steps - 1)``, which counts for ``num_task_tries`` / ``task_success_times`` but not for ``out_td``.  The result also holds ``study`` =
    ``finish_study()``'s dict and ``study_accumulators`` (host) for ``study_summary``.  Frames, records and the four metrics are those of ``study=False``, bit for
    bit; the env ends one step further.

    ``render``: a ``render.Renderer`` of this env with a ring; the rollout of the ``T - 1`` steps runs with it attached as well, so every ``render_every``-th of those
    steps is drawn into its ring after the evaluator's frame and before the resets (``renderer.video()`` afterwards).  The metrics do not change."""
    params = params if params is not None else env.parameters
    T = int(n_steps) if n_steps else int(params.max_steps) - 1
    if T < 1:
        raise ValueError("evaluation: at least one frame (n_steps, or params.max_steps - 1, must be >= 1)")
    if T * int(env.N) >= MAX_TERMS:
        raise ValueError(f"evaluation: T * n_agents = {T * int(env.N)} would reach 2^24 (the counts are reported through floats)")
    ev = Evaluator(env, trace_frames=T if trace else 0, study=study)
    try:
        if reset is not None:
            reset(env)
        else:
            env.reset_random(seed, counter=int(counter0) + T - 1)
        ev.reset()
        if study:
            ev.accumulate(initial=True)
        else:
            ev.accumulate()
        if T > 1:
            with ev.attached(), (render.attached(render_every) if render is not None else contextlib.nullcontext()):
                actor.rollout(env, T - 1, seed=seed, counter0=counter0, deterministic=deterministic, **rollout_kw)
        out = ev.finish()
        if study:
            last_kw = {k: v for k, v in rollout_kw.items() if k not in _RECORDS}
            actor.rollout(env, 1, seed=seed, counter0=int(counter0) + T, deterministic=deterministic, **last_kw)
            out["study"] = ev.finish_study()
            out["study_accumulators"] = ev.study_accumulators()
            out["n_agents"] = int(env.N)
        if trace:
            out["trace"] = ev.trace()
        return out
    finally:
        ev.close()


def noise_sweep(env, actor, levels, params=None, **evaluate_kw) -> list:
    """The reference's robustness study of prioritized action propagation -- the communication-noise level swept at evaluation -- as ONE evaluation rollout: the
    envs are split into ``len(levels)`` contiguous groups of ``B / len(levels)`` (``ValueError`` when that does not divide), group ``g`` runs at ``levels[g]``
    (``Actor.rollout(communication_noise=)`` with the per-env levels, formed in float64 so that a group computes what the scalar level computes), and
    ``evaluate``'s per-env results come back grouped: a list of dicts, one per level in order, each with ``level``, ``envs = (first, end)``, ``metrics [B / L, 4]``,
    ``counts``, the four named columns and ``frames`` -- each ready for ``summarize``.  ``evaluate_kw``: ``evaluate``'s arguments, with ``wrapper="prioritized"`` and
    ``priority=`` among them.  An env's draws are keyed by its index in the whole batch, so group ``g`` equals the evaluation of a handle of those envs alone
    (``env_index_base`` = its first env) at the scalar level."""
    levels = [float(v) for v in levels]
    n = len(levels)
    if n < 1 or int(env.B) % n:
        raise ValueError(f"noise_sweep: the {int(env.B)} envs do not split into {n} groups of equal size, one per level")
    if "communication_noise" in evaluate_kw:
        raise TypeError("noise_sweep: the levels are the communication noise")
    if "trace" in evaluate_kw:
        raise TypeError("noise_sweep: the trace is per evaluation, not per level: evaluate(trace=True, communication_noise=...)")
    g = int(env.B) // n
    per_env = torch.tensor(levels, dtype=torch.float64).repeat_interleave(g).to(env.device)
    out = evaluate(env, actor, params, communication_noise=per_env, **evaluate_kw)
    groups = []
    for k, level in enumerate(levels):
        r = {"level": level, "envs": (k * g, (k + 1) * g), "metrics": out["metrics"][k * g:(k + 1) * g], "counts": out["counts"][k * g:(k + 1) * g],
             "count_names": out["count_names"], "frames": out["frames"]}
        for c, name in enumerate(capi.EVAL_METRICS):
            r[name] = r["metrics"][:, c]
        if "study" in out:  # (study=True among evaluate_kw): the group's rows of the study's tensors and accumulators
            st, acc = out["study"], out["study_accumulators"]
            r["study"] = {"metrics": st["metrics"][k * g:(k + 1) * g], "counts": st["counts"][k * g:(k + 1) * g], "count_names": st["count_names"], "frames": st["frames"]}
            for c, name in enumerate(capi.EVAL_STUDY_METRICS):
                r["study"][name] = r["study"]["metrics"][:, c]
            r["study_accumulators"] = {name: a[..., k * g:(k + 1) * g] if name == "sums" or a.ndim == 1 else a[k * g:(k + 1) * g] for name, a in acc.items()}
            r["n_agents"] = out["n_agents"]
        groups.append(r)
    return groups


def study_summary(result) -> dict:
    """The study's numbers from ``evaluate(study=True)``'s result (or a ``noise_sweep`` group), on the host: ``per_env`` = ``finish_study``'s six columns as float32
    vectors ``[B]`` (every env one reference run with ``num_vmas_envs = 1``), their ``mean`` and ``median`` over the envs (NaN success rates -- envs without a try --
    left out of theirs; the median is torch's, as in ``summarize``: the LOWER of the two middle values of an even count, not their mean), and ``pooled`` = what ONE reference run of all ``B`` envs would print, formed in float64 from the accumulators: the event reward summed over
    the envs, the comfort penalty and the activation degree from the means over all ``B F N`` elements, the rate ``100 n_act / (B F N)``, the success rate
    ``100 sum(success) / sum(tries)`` (``None`` without a try, as the reference returns it)."""
    st, acc, N = result["study"], result["study_accumulators"], int(result["n_agents"])
    metrics = torch.as_tensor(st["metrics"]).detach().cpu().float()
    counts = np.asarray(torch.as_tensor(st["counts"]).detach().cpu()).astype(np.int64)
    B, F = metrics.shape[0], int(st["frames"])
    per_env = {name: metrics[:, k].clone() for k, name in enumerate(capi.EVAL_STUDY_METRICS)}
    mean, median = {}, {}
    for name, v in per_env.items():
        v = v[~torch.isnan(v)] if name == "task_success_rate" else v
        mean[name] = float(v.double().mean()) if v.numel() else None
        median[name] = float(v.median()) if v.numel() else None
    M = float(B * F * N)
    s = {name: float(np.sum(acc[name], dtype=np.float64)) for name in capi.EVAL_STUDY_SUM_NAMES}
    event = s["sum_event"]
    comfort = -0.2 * (s["sum_a2"] / M) + -0.2 * (s["sum_j2"] / M) if M else float("nan")
    degree = 100 * 0.5 * ((s["sum_dv"] / M) / (s["sum_av"] / M + 1e-9) + (s["sum_ds"] / M) / (s["sum_as"] / M + 1e-9)) if M else float("nan")
    tries, success = int(counts[:, 1].sum()), int(counts[:, 2].sum())
    pooled = {"total_reward": event + comfort, "event_reward": event, "comfort_reward": comfort, "cbf_activation_degree": degree,
              "cbf_activation_rate": 100 * int(counts[:, 0].sum()) / M if M else float("nan"), "task_success_rate": 100.0 * success / tries if tries > 0 else None,
              "num_task_tries": tries, "task_success_times": success}
    return {"per_env": per_env, "mean": mean, "median": median, "pooled": pooled, "frames": F, "n_envs": B, "n_agents": N}


# ---- the summary (host torch) ---------------------------------------------------------------------------------------------------------------------
def remove_max_min(t: torch.Tensor) -> torch.Tensor:
    """``remove_max_min`` (evaluation_base.py:771-809) on ``[a, b]``: every row loses its first maximum and its first minimum; a row whose first maximum and first
    minimum are the same entry -- all values equal -- loses columns 0 and 1.  ``[a, b - 2]``; the input is left as it is."""
    t = torch.as_tensor(t)
    if t.dim() != 2 or t.shape[1] < 2:
        raise ValueError("remove_max_min: a 2-D tensor with at least two columns")
    # the FIRST of equal values, the documented rule of the torch.max / torch.min(dim=) the reference calls, written out
    i_max = torch.tensor([int((row == row.max()).nonzero()[0]) for row in t], dtype=torch.long)
    i_min = torch.tensor([int((row == row.min()).nonzero()[0]) for row in t], dtype=torch.long)
    same = i_max == i_min
    i_max, i_min = torch.where(same, torch.zeros_like(i_max), i_max), torch.where(same, torch.ones_like(i_min), i_min)
    keep = torch.ones_like(t, dtype=torch.bool)
    rows = torch.arange(t.shape[0])
    keep[rows, i_max] = False
    keep[rows, i_min] = False
    return t[keep].view(t.shape[0], -1)


def summarize(metrics, agent_width: float, max_speed: float, is_remove_max_min: bool = True, is_relative_values: bool = True) -> dict:
    """``compute_performance_metrics`` / ``_log`` (evaluation_base.py:670-760) for ONE model: ``metrics`` = ``[B, 4]`` (``capi.EVAL_METRICS`` order) or a dict with
    those names (``evaluate``'s result).  The per-env vectors after ``remove_max_min`` (each metric on its own, as the reference does) and the scaling -- the rates
    x 100, the deviation / ``agent_width`` x 100, the speed / ``max_speed`` x 100 -- under the reference's names, ``collision_rate_sum``, the means ``CR_AA_avg``,
    ``CR_AL_avg``, ``CR_total_avg``, ``CD_avg``, ``AS_avg`` and the medians ``.._median`` (torch's: the lower of two middle values)."""
    if isinstance(metrics, dict):
        cols = [torch.as_tensor(metrics[name]).detach().cpu().float().reshape(1, -1).clone() for name in capi.EVAL_METRICS]
    else:
        m = torch.as_tensor(metrics).detach().cpu().float()
        cols = [m[:, k].reshape(1, -1).clone() for k in range(4)]
    speed, cr_aa, cr_al, dref = cols
    if is_remove_max_min:
        cr_aa, cr_al, dref, speed = remove_max_min(cr_aa), remove_max_min(cr_al), remove_max_min(dref), remove_max_min(speed)
    if is_relative_values:
        dref = dref / agent_width * 100
        speed = speed / max_speed * 100
    cr_aa = cr_aa * 100
    cr_al = cr_al * 100
    cr_sum = cr_aa + cr_al
    out = {"average_speed": speed[0], "collision_rate_with_agents": cr_aa[0], "collision_rate_with_lanelets": cr_al[0], "distance_ref_average": dref[0],
           "collision_rate_sum": cr_sum[0]}
    for key, v in (("CR_AA", cr_aa), ("CR_AL", cr_al), ("CR_total", cr_sum), ("CD", dref), ("AS", speed)):
        out[key + "_avg"] = v.mean(dim=-1)[0]
        out[key + "_median"] = v.median(dim=-1).values[0]
    return out


def composite_score(summaries) -> torch.Tensor:
    """The composite score across models (evaluation_base.py:715-722): ``- w1 CR_total_avg - w2 CD_avg + w3 AS_avg`` with the weights the reciprocals of the three
    quantities' means over the models.  ``summaries``: the ``summarize`` result of every model; ``[n_models]``."""
    cr = torch.stack([torch.as_tensor(s["CR_total_avg"]) for s in summaries])
    cd = torch.stack([torch.as_tensor(s["CD_avg"]) for s in summaries])
    sp = torch.stack([torch.as_tensor(s["AS_avg"]) for s in summaries])
    w1, w2, w3 = 1 / cr.mean(), 1 / cd.mean(), 1 / sp.mean()
    return -w1 * cr - w2 * cd + w3 * sp
