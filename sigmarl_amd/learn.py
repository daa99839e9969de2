"""From a device rollout to a batch a MAPPO learner can train from, without the host or a staging copy in between.

What the reference does right after ``collector.rollout()``: ``_compute_gae`` (``sigmarl/mappo_cavs.py:357-386``: torchrl ``GAE(gamma, lmbda, value_network=critic,
average_gae=False)``, ``sigmarl/modules/optimization_module.py:62-67``) and, with the prioritized replay buffer, ``compute_td_error``
(``sigmarl/helper_training.py:1029-1068``).  Here:
  ``Actor.rollout(obs_rec=...)``   records the observation every step's policy acted on (the record row of the previous step holds it only where nothing was re-placed)
  ``Critic.rollout_values``        the critic on both sides of every step, read from the records where they lie (``sigmaenv_mlp32_forward_rows``)
  ``gae``                          ``sigmaenv_gae``: advantage, value target and TD-error priorities from the record's rewards / done flags and those values
  ``collect``                      the three in a row; returns the batch under the keys of the reference's tensordict
This is the collector side of the boundary: no loss, no optimiser, no replay buffer.  torchrl is absent here: GAE's semantics are restated from its published
behaviour (the arithmetic contract is in ``include/sigmaenv.h``).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import capi
from .actor import check_record

TD_GAMMA = 0.9  # compute_td_error's discount as the trainer calls it (mappo_cavs.py:383, :454) -- not Parameters.gamma


def _values(t, T, B, what):
    if not isinstance(t, torch.Tensor) or not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == T * B and t.shape[0] == T):
        raise TypeError(f"{what} must be a contiguous float32 CUDA tensor [{T}, {B}]")
    return t


def gae(env, slab: torch.Tensor, state_value: torch.Tensor, next_state_value: torch.Tensor, gamma: float, lmbda: float, advantage: torch.Tensor | None = None,
        value_target: torch.Tensor | None = None, td_error=None, td_gamma: float = TD_GAMMA, env_first: int = 0):
    """``sigmaenv_gae`` on the records ``slab [T, Bt, W]`` of a rollout of ``env`` (``Bt >= env.B``: ``env`` owns the envs ``[env_first, env_first + env.B)`` of the
    buffer) with the critic's ``state_value`` / ``next_state_value [T, B]``: returns ``(advantage [T,B,N], value_target [T,B,N], td_error [T,B] or None)``.
    Rewards and done flags are read in place.  ``td_error``: ``None`` / ``False`` = not computed, ``True`` = a new tensor, or the tensor to fill --
    ``compute_td_error(gamma=td_gamma)`` normalised over THIS handle's ``[T, B]`` into [1e-3, 10].  Enqueued on the env's stream."""
    B, N, D = env.B, env.N, env.D
    W = N * (D + 1) + 1
    if not isinstance(slab, torch.Tensor) or not (slab.is_cuda and slab.dtype == torch.float32 and slab.is_contiguous() and slab.dim() == 3 and slab.shape[2] == W):
        raise TypeError(f"slab must be a contiguous float32 CUDA tensor [T, Bt, {W}]")
    T, Bt, e0 = slab.shape[0], slab.shape[1], int(env_first)
    if T < 1 or not 0 <= e0 <= Bt - B:
        raise ValueError(f"slab {list(slab.shape)}: at least one step, and envs [{e0}, {e0 + B}) inside its {Bt}")
    for g, name in ((gamma, "gamma"), (lmbda, "lmbda"), (td_gamma, "td_gamma")):
        if not 0.0 <= float(g) <= 1.0:
            raise ValueError(f"{name} = {g} is not in [0, 1]")
    sv, nv = _values(state_value, T, B, "state_value"), _values(next_state_value, T, B, "next_state_value")
    kw = dict(dtype=torch.float32, device=slab.device)
    adv = torch.empty((T, B, N), **kw) if advantage is None else check_record(advantage, (T, B, N), "advantage")
    vt = torch.empty((T, B, N), **kw) if value_target is None else check_record(value_target, (T, B, N), "value_target")
    td = None
    if td_error is True:
        td = torch.empty((T, B), **kw)
    elif td_error is not None and td_error is not False:
        td = check_record(td_error, (T, B), "td_error")
    a = capi.GaeArgs()
    a.n_steps, a.slab, a.slab_stride = T, slab.data_ptr() + 4 * e0 * W, Bt * W
    a.state_value, a.next_state_value, a.advantage, a.value_target = sv.data_ptr(), nv.data_ptr(), adv.data_ptr(), vt.data_ptr()
    a.td_priority = td.data_ptr() if td is not None else None
    a.gamma, a.lmbda, a.td_gamma = float(gamma), float(lmbda), float(td_gamma)
    rc = env.lib.gae(env.h, C.byref(a))
    if rc != 0:
        raise RuntimeError(f"sigmaenv_gae failed with code {rc}: {env.lib.last_error(env.h).decode()}")
    return adv, vt, td


def collect(env, actor, critic, T: int, params=None, gamma: float | None = None, lmbda: float | None = None, td_gamma: float = TD_GAMMA, td_error: bool = True,
            seed: int = 0, counter0: int = 0, **rollout_kw) -> dict:
    """One learner-ready batch: ``T`` steps of the device rollout (``Actor.rollout``, ``rollout_kw`` = its wrapper / path / precision arguments), the critic on
    both sides of every step, GAE and the TD-error priorities -- enqueued on the env's stream, nothing copied in between.  ``gamma`` / ``lmbda`` come from
    ``params`` (a ``Parameters``; default: the env's) unless given.  Returns device tensors under the reference tensordict's keys:
    ``observation [T,B,N,D]``, ``action [T,B,N,2]``, ``sample_log_prob [T,B,N]``, ``("next", "observation") [T,B,N,D]``, ``("next", "reward") [T,B,N]``,
    ``("next", "done") [T,B]`` (the record's float flag) -- the three zero-copy views of the record, which is returned whole as ``"slab"`` --, ``state_value`` /
    ``("next", "state_value") [T,B]`` (one value per env: every agent's), ``advantage`` / ``value_target [T,B,N]``, ``td_error [T,B]``."""
    p = params if params is not None else getattr(env, "parameters", None)
    if p is None and (gamma is None or lmbda is None):
        raise ValueError("collect(): gamma and lmbda, or a Parameters to take them from")
    gamma = float(gamma if gamma is not None else p.gamma)
    lmbda = float(lmbda if lmbda is not None else p.lmbda)
    for k in ("slab", "log_prob", "actions", "obs_rec", "slab_ptr"):
        if k in rollout_kw:
            raise TypeError(f"collect() makes the {k} record itself")
    T, B, N, D = int(T), env.B, env.N, env.D
    W = N * (D + 1) + 1
    kw = dict(dtype=torch.float32, device=env.device)
    slab, obs = torch.empty((T, B, W), **kw), torch.empty((T, B, N, D), **kw)
    act, logp = torch.empty((T, B, N, 2), **kw), torch.empty((T, B, N), **kw)
    actor.rollout(env, T, slab=slab, log_prob=logp, actions=act, obs_rec=obs, seed=seed, counter0=counter0, **rollout_kw)
    sv, nv = critic.rollout_values(env, slab, obs, T)
    adv, vt, td = gae(env, slab, sv, nv, gamma, lmbda, td_error=bool(td_error), td_gamma=td_gamma)
    out = {
        "observation": obs, "action": act, "sample_log_prob": logp, "slab": slab,
        ("next", "observation"): slab[:, :, : N * D].unflatten(2, (N, D)), ("next", "reward"): slab[:, :, N * D: N * D + N], ("next", "done"): slab[:, :, N * D + N],
        "state_value": sv, ("next", "state_value"): nv, "advantage": adv, "value_target": vt,
    }
    if td is not None:
        out["td_error"] = td
    return out
