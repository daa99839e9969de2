"""Which observation features a trained policy uses: the gradient of a network's raw outputs with respect to its input rows, on the device.

The reference answers the question by ablation -- its ``is_observe_*`` flags remove a feature group and a policy is trained again without it.  The gradient asks the
trained network itself: ``observation_saliency`` runs a network made with ``input_grad=True`` on the rows of a rollout record where they lie and reduces
``|d out_c / d x|`` over the rows, per raw output column ``c`` and input column.  The network kernels are the library's (``Mlp32.input_grad``:
one ``sigmaenv_mlp32_forward_save`` and one ``sigmaenv_mlp32_input_grad`` per output column); the reductions are plain torch -- this is the input gradient's first
consumer, not a hot path.
"""
from __future__ import annotations

import torch

from .actor import Actor, Mlp32
from .env import SigmaEnv


def observation_saliency(env: SigmaEnv, net, record: torch.Tensor, outputs=(0, 1)):
    """``(mean_abs, max_abs)``, each ``[len(outputs), in_dim]``: over the rows of ``record`` the mean and the largest ``|dx|``, ``dx`` the gradient of the raw output
    column ``outputs[i]`` with respect to the input row (``dout`` = that column's one-hot in every row).  ``net``: an ``Mlp32`` (``Critic``, ``PriorityNet``) or an
    ``Actor`` made with ``input_grad=True``; for the actor the raw columns 0, 1 are the two ``loc`` outputs.  ``record``: any contiguous float32 CUDA tensor
    ``[..., in_dim]`` -- ``obs_rec`` or ``base_obs`` of ``Actor.rollout``, for a critic an ``obs_rec`` viewed ``[T, B, N D]`` --, read in place.  No row: zeros."""
    m32 = net._mlp32 if isinstance(net, Actor) else net
    if not isinstance(m32, Mlp32):
        raise TypeError("observation_saliency: net must be an Mlp32 or an Actor")
    if not (isinstance(record, torch.Tensor) and record.is_cuda and record.dtype == torch.float32 and record.is_contiguous() and record.dim() >= 1
            and record.shape[-1] == m32.in_dim):
        raise TypeError(f"observation_saliency: record must be a contiguous float32 CUDA tensor [..., {m32.in_dim}]")
    outputs = [int(c) for c in outputs]
    if any(not 0 <= c < m32.out_dim for c in outputs):
        raise ValueError(f"observation_saliency: output columns {outputs} are not all inside the network's {m32.out_dim}")
    n = record.numel() // m32.in_dim
    mean_abs = torch.zeros((len(outputs), m32.in_dim), dtype=torch.float32, device=record.device)
    max_abs = torch.zeros_like(mean_abs)
    if n == 0:
        return mean_abs, max_abs
    rows = (record, 0, n, m32.in_dim, 1, 0)
    for i, c in enumerate(outputs):
        dout = torch.zeros((n, m32.out_dim), dtype=torch.float32, device=record.device)
        dout[:, c] = 1.0
        dx = m32.input_grad(env, rows=rows, dout=dout)[1].abs()
        mean_abs[i], max_abs[i] = dx.mean(0), dx.amax(0)
    return mean_abs, max_abs
