"""The policy (actor) forward pass and whole rollouts on the device.

``Actor`` wraps ``sigmaenv_actor_*`` / ``sigmaenv_rollout`` of the C-ABI: the actor network of
``sigmarl/modules/decision_making_module.py:34-82`` (torchrl ``MultiAgentMLP(depth=3, num_cells=256, activation=Tanh, share_params=True)``
+ ``NormalParamExtractor`` + ``TanhNormal``).  Two precisions:
  ``precision="fp32"`` (default)  the reference's fp32 network on the matrix cores (``sigmaenv_actor_forward_f32``); ``mode="split"`` (default) forms every fp32 product
                                  from three exact fp16 products, ``mode="exact"`` runs fp32 fma chains (2.7 x slower); both within 1e-5 of torch.nn
  ``precision="bf16"``            the fast inference variant: bf16 weights / activations, fp32 accumulation, one fused MFMA kernel; also what
                                  ``sigmaenv_rollout`` (policy + step without the host in the loop) runs
``Critic`` is the MAPPO critic of ``sigmarl/modules/optimization_module.py:16-32`` (centralised, shared parameters) in fp32 (same modes).
``PriorityNet`` is the priority actor of ``sigmarl/modules/priority_module.py`` (scores, log-probabilities and ranks); ``Actor.rollout(wrapper=...)`` runs the
collector's opponent-modelling or prioritized-propagation policy in the fp32 device rollout (``sigmaenv_rollout_f32_ex``).
``Actor.rollout(obs_rec=...)`` records the observation every step's policy acted on, ``Mlp32.forward_rows`` / ``Critic.rollout_values`` run a network on the
rollout's records where they lie (``sigmaenv_mlp32_forward_rows``); ``sigmarl_amd.learn`` builds the learner's batch from them.
Weights come from any ``torch.nn.Sequential`` of four ``Linear`` layers (the parameter layout torchrl's shared-parameter MLP has).
``Mlp32.load`` / ``Actor.load`` put a learner's updated CUDA parameters into the existing device networks (``sigmaenv_mlp32_load_device`` /
``sigmaenv_actor_load_device``: packed by a kernel, no weight visits the host), so that collect -> torch update -> load -> collect stays on the device.
``Mlp32.apply`` / ``Actor.apply`` / ``Critic.apply`` differentiate the fp32 networks on the device (``sigmaenv_mlp32_forward_save`` / ``sigmaenv_mlp32_backward``); with
``index=`` on a minibatch of frames picked out of the records (``*_indexed``), which ``sigmarl_amd.learn`` (``ppo_head``, ``update``) trains from.  Networks made with
``input_grad=True`` also give the gradient with respect to the input rows: ``apply`` on a dense ``x`` that requires one, ``Mlp32.input_grad`` without autograd
(``sigmaenv_mlp32_backward_dx`` / ``sigmaenv_mlp32_input_grad``); ``sigmarl_amd.saliency`` is its first consumer.

The distribution heads (actor, priority actor) and ``random_ranks``: the draw of every row -- the counter-based generator keyed by (seed, the low 32 bits of
counter, env_index_base + env, agent), Box-Muller with z0 the cosine and z1 the sine branch -- the action and the log-probability are pinned against fp64 on every
path (``tests/test_gpu_policy_head.py``, restated in ``tests/policy_head_check.py``).  The log-probability is that of the unclamped ``x = loc + scale z``, never
of ``atanh`` of the clamped action.  Whether torchrl's own ``TanhNormal.log_prob`` does the same for a saturated sample is not verified (torchrl is absent here).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import capi
from .env import SigmaEnv
from .params import check_initial_state_bank, check_rollout_wrapper


def make_mlp(obs_dim: int = 32, hidden: int = 256, n_out: int = 4) -> torch.nn.Sequential:
    """The reference's actor architecture in plain torch.nn (what ``MultiAgentMLP(share_params=True)`` applies to every agent row)."""
    return torch.nn.Sequential(torch.nn.Linear(obs_dim, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, hidden), torch.nn.Tanh(),
                               torch.nn.Linear(hidden, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, n_out))


def load_source(dims, source, device):
    """The parameters ``load`` takes, checked before any device call: ``source`` is a ``torch.nn.Module`` with the network's ``Linear`` stack or a sequence of
    ``(weight, bias)`` tensors; float32 CUDA tensors on ``device`` (``TypeError`` otherwise) of the shapes ``[dims[l + 1], dims[l]]`` / ``[dims[l + 1]]`` and
    ``len(dims) - 1`` layers (``ValueError`` otherwise).  Returns ``(weights, biases)``, detached."""
    if isinstance(source, torch.nn.Module):
        pairs = [(m.weight, m.bias) for m in source.modules() if isinstance(m, torch.nn.Linear)]
    else:
        try:
            pairs = [tuple(q) for q in source]
        except TypeError:
            raise TypeError("load: source must be a torch.nn.Module or a sequence of (weight, bias) tensors") from None
    n = len(dims) - 1
    if len(pairs) != n or any(len(q) != 2 for q in pairs):
        raise ValueError(f"load: the network has {n} Linear layers, the source {len(pairs)} (weight, bias) pairs")
    ws, bs = [], []
    for l, (w, b) in enumerate(pairs):
        for t, shape, what, to in ((w, (int(dims[l + 1]), int(dims[l])), "weight", ws), (b, (int(dims[l + 1]),), "bias", bs)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.device != device:
                raise TypeError(f"load: layer {l} {what} must be a float32 CUDA tensor on {device}")
            if tuple(t.shape) != shape:
                raise ValueError(f"load: layer {l} {what} has shape {list(t.shape)}, the network's is {list(shape)} (torch.nn.Linear layout)")
            to.append(t.detach())
    return ws, bs


def source_pairs(source):
    """The ``(weight, bias)`` tensors of a ``load`` source as they are (not detached): what ``apply`` credits the gradients to."""
    if isinstance(source, torch.nn.Module):
        return [(m.weight, m.bias) for m in source.modules() if isinstance(m, torch.nn.Linear)]
    return [tuple(q) for q in source]


def _save_forward(ctx, net, env, spec, shape):
    """The saving forward of both ``apply`` Functions, and what their backward needs of it: the row addressing, the activations, the weights' version."""
    y, acts = net._forward_save(env, spec)
    ctx.net, ctx.env, ctx.spec, ctx.acts, ctx.version = net, env, spec, acts, net._version
    return y.view(shape)


def _saved_net(ctx):
    if ctx.net._version != ctx.version:
        raise RuntimeError("Mlp32.apply: load() replaced the network's weights between this forward and its backward")
    return ctx.net


class _Mlp32Function(torch.autograd.Function):
    """``Mlp32.apply``: ``sigmaenv_mlp32_forward_save`` forwards, ``sigmaenv_mlp32_backward`` backwards; the inputs are the network's parameters (weight, bias per
    layer), the rows are a constant."""

    @staticmethod
    def forward(ctx, net, env, spec, shape, *params):
        return _save_forward(ctx, net, env, spec, shape)

    @staticmethod
    def backward(ctx, dy):
        gw, gb = _saved_net(ctx)._backward(ctx.env, ctx.spec, ctx.acts, dy)
        ctx.acts = None
        return (None, None, None, None, *[t for q in zip(gw, gb) for t in q])


class _Mlp32InputFunction(torch.autograd.Function):
    """``Mlp32.apply`` on a dense ``x`` that requires a gradient (a network made with ``input_grad=True``): ``x`` is a tensor input next to the parameters.
    Backwards, the parameters' gradients are computed only if one of them needs its own and ``dx`` only if ``x`` does (``sigmaenv_mlp32_backward_dx`` /
    ``sigmaenv_mlp32_input_grad`` / ``sigmaenv_mlp32_backward``); no double backward."""

    @staticmethod
    def forward(ctx, net, env, shape, x, *params):
        return _save_forward(ctx, net, env, (x.detach(), 0, x.numel() // net.in_dim, net.in_dim, 1, 0, None), shape)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        want_dx, want_params = ctx.needs_input_grad[3], any(ctx.needs_input_grad[4:])
        gw, gb, dx = _saved_net(ctx)._backward_dx(ctx.env, ctx.spec, ctx.acts, dy, want_params, want_dx)
        x = ctx.spec[0]
        ctx.acts = ctx.spec = None
        grads = [t for q in zip(gw, gb) for t in q] if want_params else [None] * (len(ctx.needs_input_grad) - 4)
        return (None, None, None, dx.view(x.shape) if want_dx else None, *grads)


def _env_list(env):
    envs = list(env) if isinstance(env, (list, tuple)) else [env]
    if not envs:
        raise ValueError("load: no env given")
    if any(e.device != envs[0].device for e in envs):
        raise ValueError("load: the envs must be on one device")
    return envs


def _by_library(envs):
    groups = {}
    for e in envs:
        groups.setdefault(e.lib.path, []).append(e)
    return list(groups.values())


class Mlp32:
    """``sigmaenv_mlp32_*``: a Tanh MLP with hidden width 256 in fp32 on the matrix cores; ``forward(env, x[rows, in_dim]) -> [rows, out_dim]``.
    ``mode``: ``"split"`` (default: every fp32 operand as two fp16 numbers, three exact-product MFMAs per fp32 product, 3/16 of the fp32 matrix time; falls back
    to exact when a weight is outside +-255 or the input is wider than 592) or ``"exact"`` (``v_mfma_f32_32x32x2_f32`` fma chains).  Input widths 1 to 4096.  Both are
    held to torch.nn in fp64 within the precision class of torch.nn in fp32 (tests/network_check.py)."""

    def __init__(self, mlp: torch.nn.Module, lib: capi.Library | None = None, mode: str = "split", input_grad: bool = False):
        if mode not in ("split", "exact"):
            raise ValueError("mode must be 'split' or 'exact'")
        self._input_grad = bool(input_grad)  # the handles also hold layer 0's transposed form (sigmaenv_mlp32_create_input_grad): ``apply`` differentiates through ``x``
        self.mode = mode          # the mode in force (after a ``load``: what the weights allow)
        self._requested = mode    # the mode asked for
        self._handles = {}
        self._handle_version = {}  # library path -> the version of the weights its handle holds (0: those of the constructor)
        self._version, self._loaded = 0, None  # ``load``: count, and (weights, biases, ready event, stream) of the device snapshot
        self._stepped_source = None  # after ``learn.Adam.step``: the (weights, biases) a snapshot is taken from when a handle of another library needs one
        lin = [m for m in mlp.modules() if isinstance(m, torch.nn.Linear)]
        if not (2 <= len(lin) <= 4) or any(m.out_features != 256 for m in lin[:-1]) or lin[-1].out_features > 32:
            raise ValueError("expected 2-4 Linear layers with hidden width 256 and at most 32 outputs")
        self.in_dim, self.out_dim = lin[0].in_features, lin[-1].out_features
        if not 1 <= self.in_dim <= 4096:
            raise ValueError(f"input width {self.in_dim}: sigmaenv_mlp32 takes 1 to 4096 inputs (include/sigmaenv.h)")
        # A handle belongs to the library that made it, and an env handle to the build of ITS n_points_short_term (libsigmaenv_ns<k>.so): every call
        # that takes ``env.h`` goes through ``env.lib`` with a network handle created by that same library (one per library, made on first use).
        self.lib = lib or capi.load_library()
        dims = np.asarray([self.in_dim] + [m.out_features for m in lin], np.int32)
        ws = [np.ascontiguousarray(m.weight.detach().cpu().numpy(), np.float32) for m in lin]
        bs = [np.ascontiguousarray(m.bias.detach().cpu().numpy(), np.float32) for m in lin]
        self._keep = (dims, ws, bs)
        self._remember([(m.weight, m.bias) for m in lin])
        self.h = self.handle(self.lib)

    def _remember(self, pairs):
        """The tensors ``apply`` differentiates with respect to -- those the packed weights were last made from -- and their versions then."""
        self._params = [t for q in pairs for t in q]
        self._param_versions = [t._version for t in self._params]

    def handle(self, lib: capi.Library, env: SigmaEnv | None = None):
        """The network's handle in ``lib`` (created on first use).  With ``env`` (an env of ``lib``, as every forward passes it): a handle that does not hold the
        weights of the last ``load`` yet -- one of another library, or one created after it -- is brought up to date on ``env``'s stream first."""
        ent = self._handles.get(lib.path)
        if ent is None:
            dims, ws, bs = self._keep
            PA = C.c_void_p * len(ws)
            wp, bp = PA(*[w.ctypes.data for w in ws]), PA(*[b.ctypes.data for b in bs])
            h = C.c_void_p()
            create = lib.mlp32_create_input_grad if self._input_grad else lib.mlp32_create
            rc = create(len(ws), dims.ctypes.data_as(C.c_void_p), wp, bp, C.byref(h))
            if rc != 0:
                raise RuntimeError(f"sigmaenv_mlp32_create{'_input_grad' if self._input_grad else ''} failed with code {rc}")
            if self._requested == "exact":
                lib.mlp32_set_mode(h, capi.MLP32_EXACT)
            ent = self._handles[lib.path] = (lib, h)
            self._handle_version[lib.path] = 0
        if env is not None and self._handle_version[lib.path] != self._version:
            self._pack([env])
        return ent[1]

    def _ordered_pack(self, group, call):
        """``call(env)`` enqueues pack kernels on ``group[0]``'s stream; the envs of ``group`` share the handle they rewrite.  Before: that stream waits for the
        snapshot and for what the other envs' streams hold (forwards that read the old weights).  After: the other streams wait for the pack."""
        ws, bs, ready, made_on = self._loaded
        first = group[0]
        with torch.cuda.device(first.device):
            first.stream.wait_event(ready)
            if first.stream != made_on:
                for t in ws + bs:
                    t.record_stream(first.stream)
            for e in group[1:]:
                first.stream.wait_stream(e.stream)
            call(first)
            for e in group[1:]:
                e.stream.wait_stream(first.stream)

    def _device_pointers(self):
        ws, bs = self._loaded[0], self._loaded[1]
        PA = C.c_void_p * len(ws)
        return PA(*[w.data_ptr() for w in ws]), PA(*[b.data_ptr() for b in bs])

    def _pack(self, group):
        """The snapshot of the last ``load`` into the handle of ``group``'s library."""
        self._ensure_snapshot(group[0])
        lib = group[0].lib
        h = self.handle(lib)
        wp, bp = self._device_pointers()
        self._ordered_pack(group, lambda env: env._chk(lib.mlp32_load_device(env.h, h, wp, bp), "mlp32_load_device"))
        self._handle_version[lib.path] = self._version

    def _snapshot(self, envs, ws, bs):
        """A device copy of the parameters (contiguous; ~1 MB) on the first env's stream, after what torch's current stream holds (the optimiser's kernels)."""
        self._take_snapshot(envs[0], ws, bs)
        self._version += 1

    def _ensure_snapshot(self, env):
        """``learn.Adam.step`` packs from the parameters themselves and leaves no snapshot: a handle of another library takes one when it is next used."""
        if self._loaded is None:
            self._take_snapshot(env, *self._stepped_source)

    def _stepped(self, env, pairs):
        """``learn.Adam.step`` has updated the parameters ``pairs`` in place and repacked this network's handle in ``env``'s library on ``env``'s stream: that
        handle holds the new version, every other one is stale until its next use (``handle``), the mode in force is exact until ``resolve`` (``learn.Adam``)."""
        self._version += 1
        self._loaded, self._stepped_source = None, ([w.detach() for w, _ in pairs], [b.detach() for _, b in pairs])
        self._handle_version[env.lib.path] = self._version
        self._remember(pairs)
        self.mode = "exact"

    def _take_snapshot(self, first, ws, bs):
        with torch.cuda.device(first.device):
            first.stream.wait_stream(torch.cuda.current_stream(first.device))
            with torch.cuda.stream(first.stream):
                ws = [w.clone(memory_format=torch.contiguous_format) for w in ws]
                bs = [b.clone(memory_format=torch.contiguous_format) for b in bs]
                ready = torch.cuda.Event()
                ready.record(first.stream)
        self._loaded = (ws, bs, ready, first.stream)

    def _mode_in_force(self, lib) -> str:
        return "split" if lib.mlp32_get_mode(self.handle(lib)) == capi.MLP32_SPLIT else "exact"

    def load(self, env, source) -> str:
        """New weights for the network, from the learner's tensors on the device: ``source`` is a ``torch.nn.Module`` with the same ``Linear`` stack or a sequence
        of ``(weight, bias)`` float32 CUDA tensors on the env's device, in ``torch.nn.Linear`` layout (a CPU tensor, another dtype: ``TypeError``; another layer
        count or shape: ``ValueError``; both before any device call; non-contiguous tensors are made contiguous on the device).  A kernel packs them into the
        network's buffers in place (``sigmaenv_mlp32_load_device``): no weight visits the host, no buffer is allocated or freed, every handle stays valid, and
        the network afterwards computes bit for bit what a new ``Mlp32`` made from the same numbers computes.  Returns the mode in force, which ``mode`` then
        holds too: a network asked to run ``"split"`` runs ``"exact"`` while a weight is outside +-255 (or is a NaN) and returns to ``"split"`` with the next
        load that is inside -- the call waits for the 4 bytes that say so, its only host wait.

        Every handle: the parameters are first copied on the device (a snapshot); the handle of each given env's library is created if there is none and
        rewritten now, a handle of another library -- or one made later -- when it is next used with an env of its library, on that env's stream.

        Streams: ``env`` is one env or a sequence of envs that share this network on their own streams (the shards of ``bench.py --policy``).  The parameters are
        read after everything torch's CURRENT stream holds at the call (the optimiser's kernels, in the common case where that is also the env's stream).  The
        pack runs on the first env's stream after everything the other given envs' streams hold, so a forward enqueued on any of them before the call reads the
        old weights whole; every forward enqueued on any of them after ``load`` returns reads the new ones.  A caller with FURTHER streams orders them itself:
        parameters produced on another stream -- make torch's current stream wait for it before ``load``; forwards of this network on a stream of an env that was
        not passed -- pass that env, or make that stream wait for ``envs[0].stream`` after ``load`` and ``envs[0].stream`` for it before."""
        envs = _env_list(env)
        ws, bs = load_source(self._keep[0], source, envs[0].device)
        mode = self._load(envs, ws, bs)
        self._remember(source_pairs(source))
        return mode

    def _load(self, envs, ws, bs) -> str:
        self._snapshot(envs, ws, bs)
        for group in _by_library(envs):
            self._pack(group)
        self.mode = self._mode_in_force(envs[0].lib)
        return self.mode

    def set_mode(self, mode: str) -> str:
        """Switch every handle to ``"split"`` / ``"exact"``; returns the mode in force (a network outside the split form's range stays exact)."""
        if mode not in ("split", "exact"):
            raise ValueError("mode must be 'split' or 'exact'")
        self.mode = self._requested = mode
        got = mode
        for lib, h in self._handles.values():
            lib.mlp32_set_mode(h, capi.MLP32_SPLIT if mode == "split" else capi.MLP32_EXACT)
            got = "split" if lib.mlp32_get_mode(h) == capi.MLP32_SPLIT else "exact"
        return got

    def close(self):
        for lib, h in getattr(self, "_handles", {}).values():
            lib.mlp32_destroy(h)
        self._handles, self._handle_version = {}, {}
        self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def forward(self, env: SigmaEnv, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.shape[-1] == self.in_dim):
            raise TypeError(f"input must be a contiguous float32 CUDA tensor [..., {self.in_dim}]")
        if x.data_ptr() % 16:  # (a view at a storage offset: the kernels read the rows with 16-byte loads, include/sigmaenv.h)
            x = x.clone()
        rows = x.numel() // self.in_dim
        if out is None:
            out = torch.empty((*x.shape[:-1], self.out_dim), dtype=torch.float32, device=x.device)
        if rows == 0:
            return out
        env._chk(env.lib.mlp32_forward(env.h, self.handle(env.lib, env), C.c_void_p(x.data_ptr()), rows, C.c_void_p(out.data_ptr())), "mlp32_forward")
        return out

    def _pad(self, pad, what):
        """``pad = (src, dst)`` checked: the network's input row is ``in_dim / dst`` segments of width ``dst``, the row in memory as many of width ``src <= dst``;
        returns ``(src, dst, the width of the row in memory)``.  ``None``: ``(0, 0, in_dim)``."""
        if pad is None:
            return 0, 0, self.in_dim
        try:
            src, dst = (int(v) for v in pad)
        except (TypeError, ValueError):
            raise TypeError(f"{what}: pad is (source segment width, destination segment width)") from None
        if src < 1 or dst < src or self.in_dim % dst:
            raise ValueError(f"{what}: pad = ({src}, {dst}) needs 1 <= src <= dst and dst a divisor of the input width {self.in_dim}")
        return src, dst, self.in_dim // dst * src

    def forward_rows(self, env: SigmaEnv, base: torch.Tensor, offset: int, rows_per_block: int, row_stride: int, n_blocks: int = 1, block_stride: int = 0,
                     out: torch.Tensor | None = None, pad=None) -> torch.Tensor:
        """``sigmaenv_mlp32_forward_rows``: the network on rows that lie inside ``base`` (any contiguous float32 CUDA tensor, read as flat floats) -- row
        ``t * rows_per_block + b`` starts at float ``offset + t * block_stride + b * row_stride`` -- without copying them out; 4-byte alignment suffices.  Returns
        ``[n_blocks, rows_per_block, out_dim]``, bit for bit what ``forward`` gives the same rows copied dense.  Enqueued on the env's stream.
        ``pad = (src, dst)`` (``sigmaenv_mlp32_forward_rows_pad``): the rows in memory are ``in_dim / dst`` segments of ``src`` floats, each read as ``dst`` columns
        of which the last ``dst - src`` are zero -- bit for bit ``forward`` on the rows copied dense and padded, without that copy."""
        if not (base.is_cuda and base.dtype == torch.float32 and base.is_contiguous()):
            raise TypeError("the rows must lie in a contiguous float32 CUDA tensor")
        offset, rpb, rs, nb, bs, src, dst = check_rows(self, base, offset, rows_per_block, row_stride, n_blocks, block_stride, pad, "forward_rows")
        if out is None:
            out = torch.empty((nb, rpb, self.out_dim), dtype=torch.float32, device=base.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == nb * rpb * self.out_dim):
            raise TypeError(f"out must be a contiguous float32 CUDA tensor of {nb * rpb * self.out_dim} elements")
        if rpb == 0 or nb == 0:
            return out
        rows = (env.h, self.handle(env.lib, env), C.c_void_p(base.data_ptr() + 4 * offset), rpb, rs, nb, bs)
        if pad is not None:
            env._chk(env.lib.mlp32_forward_rows_pad(*rows, src, dst, C.c_void_p(out.data_ptr())), "mlp32_forward_rows_pad")
        else:
            env._chk(env.lib.mlp32_forward_rows(*rows, C.c_void_p(out.data_ptr())), "mlp32_forward_rows")
        return out


    # ---- the network differentiated (sigmaenv_mlp32_forward_save / sigmaenv_mlp32_backward) ----
    def _index(self, env, index, n_blocks, in_range):
        """The minibatch's block indices, checked before any launch: ``check_index``'s tensor (``TypeError``) whose entries -- unless ``in_range`` is false --
        lie in ``[0, n_blocks)`` (``ValueError``; ``min`` / ``max`` on the device, one host wait)."""
        check_index(index, env, "apply")
        if in_range and index.numel():
            lo, hi = (int(v) for v in torch.stack((index.min(), index.max())).tolist())
            if lo < 0 or hi >= n_blocks:
                raise ValueError(f"apply: index entries in [{lo}, {hi}] are not all inside the record's {n_blocks} blocks")
        return index

    def _rows_spec(self, x, rows, env=None, index=None, check_index=True, pad=None):
        if pad is not None and index is None:
            raise TypeError("apply: pad (padded rows) is built for rows picked by index")
        if index is not None and rows is None:
            raise TypeError("apply: index picks blocks of rows = (base, offset, rows_per_block, row_stride, n_blocks, block_stride)")
        if (x is None) == (rows is None):
            raise TypeError("apply: either x [rows, in_dim] or rows = (base, offset, rows_per_block, row_stride, n_blocks, block_stride)")
        if x is not None:
            if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() >= 1 and x.shape[-1] == self.in_dim):
                raise TypeError(f"input must be a contiguous float32 CUDA tensor [..., {self.in_dim}]")
            if x.requires_grad:
                raise NotImplementedError("apply: the gradient with respect to the input is not built (x.requires_grad)")
            return (x, 0, x.numel() // self.in_dim, self.in_dim, 1, 0, None), (*x.shape[:-1], self.out_dim)
        base, offset, rpb, rs, nb, bs = rows
        if not (isinstance(base, torch.Tensor) and base.is_cuda and base.dtype == torch.float32 and base.is_contiguous()):
            raise TypeError("the rows must lie in a contiguous float32 CUDA tensor")
        if base.requires_grad:
            raise NotImplementedError("apply: the gradient with respect to the input is not built (rows base requires_grad)")
        offset, rpb, rs, nb, bs, src, dst = check_rows(self, base, offset, rpb, rs, nb, bs, pad, "apply")
        if index is not None:
            index = self._index(env, index, nb, check_index)
            if pad is not None:
                return (base, offset, rpb, rs, nb, bs, index, (src, dst)), (index.numel(), rpb, self.out_dim)
            return (base, offset, rpb, rs, nb, bs, index), (index.numel(), rpb, self.out_dim)
        return (base, offset, rpb, rs, nb, bs, None), (nb, rpb, self.out_dim)

    @staticmethod
    def _picked(index, pad):
        """Which of an entry point's three forms a row addressing takes -- plain, ``_indexed``, ``_indexed_pad`` -- and the arguments that form adds."""
        if index is None:
            return "", ()
        args = (C.c_void_p(index.data_ptr()), index.numel())
        return ("_indexed_pad", (*args, *pad[0])) if pad else ("_indexed", args)

    def _forward_save(self, env, spec):
        """(y [rows, out_dim], acts [n_layers - 1, rows, 256]) on the env's stream, ordered after and before torch's current stream (``SigmaEnv._on_stream``)."""
        base, offset, rpb, rs, nb, bs, index, *pad = spec  # (an eighth entry: (src, dst) of padded rows, with an index)
        n, dev = rpb * (nb if index is None else index.numel()), env.device
        y = torch.empty((n, self.out_dim), dtype=torch.float32, device=dev)
        acts = torch.empty((len(self._keep[1]) - 1, n, 256), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):  # a handle that is behind the last ``load`` is packed here, ahead of the first wait: on the env's stream, so before the kernel
            h = self.handle(env.lib, env)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        suffix, picked = self._picked(index, pad)
        what, args = "mlp32_forward_save" + suffix, (env.h, h, C.c_void_p(base.data_ptr() + 4 * offset), rpb, rs, nb, bs, *picked, p(y), p(acts))
        env._on_stream(what, lambda: getattr(env.lib, what)(*args), (base, y, acts) + (() if index is None else (index,)))
        return y, acts

    def _backward(self, env, spec, acts, dout):
        """(grad_w, grad_b) lists in ``torch.nn.Linear`` layout: ``sigmaenv_mlp32_backward`` on the env's stream, ordered as ``_forward_save``."""
        return self._backward_dx(env, spec, acts, dout, want_dx=False)[:2]

    def _backward_dx(self, env, spec, acts, dout, want_params=True, want_dx=True):
        """(grad_w, grad_b, dx [n, in_dim]) on the env's stream, ordered as ``_forward_save``; what is not wanted is ``None`` and is not computed:
        ``sigmaenv_mlp32_backward_dx`` for both, ``sigmaenv_mlp32_input_grad`` for ``dx`` alone (one launch, no input row read), ``sigmaenv_mlp32_backward`` /
        ``_indexed`` / ``_indexed_pad`` for the parameters alone, no launch for neither."""
        if not (want_params or want_dx):
            return None, None, None
        if want_dx and not self._input_grad:
            raise RuntimeError("the gradient with respect to the input needs a network made with input_grad=True")
        base, offset, rpb, rs, nb, bs, index, *pad = spec
        n, dev = rpb * (nb if index is None else index.numel()), env.device
        dims = [int(d) for d in self._keep[0]]
        dout = dout.reshape(n, self.out_dim).to(torch.float32).contiguous()
        nf = C.c_uint64()
        h = self.handle(env.lib)
        query = "backward" if want_params else "input_grad"
        rc = getattr(env.lib, f"mlp32_{query}_workspace")(h, n, C.byref(nf))
        if rc != 0:
            raise RuntimeError(f"sigmaenv_mlp32_{query}_workspace failed with code {rc}")
        ws = torch.empty((max(int(nf.value), 4),), dtype=torch.float32, device=dev)
        dx = torch.empty((n, self.in_dim), dtype=torch.float32, device=dev) if want_dx else None
        gw = [torch.empty((dims[l + 1], dims[l]), dtype=torch.float32, device=dev) for l in range(len(dims) - 1)] if want_params else None
        gb = [torch.empty((dims[l + 1],), dtype=torch.float32, device=dev) for l in range(len(dims) - 1)] if want_params else None
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        if not want_params:
            what, args = "mlp32_input_grad", (p(acts), p(dout), n, p(ws), p(dx))
        else:
            PA = C.c_void_p * len(gw)
            rows, tail = (C.c_void_p(base.data_ptr() + 4 * offset), rpb, rs, nb, bs), (p(acts), p(dout), p(ws), PA(*[t.data_ptr() for t in gw]), PA(*[t.data_ptr() for t in gb]))
            if want_dx:
                what, picked = "mlp32_backward_dx", (None if index is None else p(index), 0 if index is None else index.numel(), *(pad[0] if pad else (0, 0)))
                tail += (p(dx),)
            else:
                suffix, picked = self._picked(index, pad)
                what = "mlp32_backward" + suffix
            args = (*rows, *picked, *tail)
        env._on_stream(what, lambda: getattr(env.lib, what)(env.h, h, *args),
                       [base, acts, dout, ws] + ([dx] if want_dx else []) + (gw + gb if want_params else []) + ([] if index is None else [index]))
        return gw, gb, dx

    def input_grad(self, env: SigmaEnv, x: torch.Tensor | None = None, *, rows=None, index: torch.Tensor | None = None, check_index: bool = True, pad=None, dout: torch.Tensor):
        """``(y, dx)`` without autograd (a network made with ``input_grad=True``): the network's outputs on the rows -- ``x`` dense, or ``rows`` / ``index`` / ``pad``
        read where they lie, as ``apply`` takes them -- and the gradient of ``sum(y * dout)`` with respect to them, ``dx [n, in_dim]`` dense in the order of the
        rows (``pad``: the network's ``in_dim`` columns, padding included).  ``dout``: float32 CUDA, ``n * out_dim`` elements.  One saving forward and one launch
        (``sigmaenv_mlp32_input_grad``); the same bits for the same rows whatever their layout; the parameters are not looked at.  Streams: as ``apply``."""
        if not self._input_grad:
            raise RuntimeError("input_grad: the network was not made with input_grad=True")
        if isinstance(x, torch.Tensor):
            x = x.detach()
        spec, shape = self._rows_spec(x, rows, env, index, check_index, pad)
        n = int(np.prod(shape[:-1]))
        if not (isinstance(dout, torch.Tensor) and dout.is_cuda and dout.dtype == torch.float32 and dout.device == env.device and dout.numel() == n * self.out_dim):
            raise TypeError(f"input_grad: dout must be a float32 CUDA tensor of {n * self.out_dim} elements on {env.device}")
        y, acts = self._forward_save(env, spec)
        return y.view(shape), self._backward_dx(env, spec, acts, dout.detach(), want_params=False)[2]

    def apply(self, env: SigmaEnv, x: torch.Tensor | None = None, *, rows=None, index: torch.Tensor | None = None, check_index: bool = True, pad=None) -> torch.Tensor:
        """The network with a ``grad_fn``: ``y = apply(env, x)`` for dense ``x [..., in_dim]`` (``y [..., out_dim]``) or ``apply(env, rows=(base, offset,
        rows_per_block, row_stride, n_blocks, block_stride))`` for rows read where they lie, as ``forward_rows`` addresses them (``y [n_blocks, rows_per_block,
        out_dim]``) -- a minibatch of whole time slices of a rollout record.  With ``index`` (a contiguous int32 CUDA tensor ``[M]``, with ``rows``): a minibatch of
        BLOCKS, block ``m`` of the result being block ``index[m]`` of the record (``y [M, rows_per_block, out_dim]``; ``sigmaenv_mlp32_forward_save_indexed`` /
        ``sigmaenv_mlp32_backward_indexed``) -- shuffled frames, duplicates allowed --, bit for bit what the same rows gathered dense give.  An entry outside
        ``[0, n_blocks)`` raises ``ValueError`` before any launch (``index.min()`` / ``max()``: one host wait; ``check_index=False`` skips it, and the kernels then
        read such a block as zeros).  ``pad = (src, dst)`` (with ``index``; ``forward_rows``'s): the rows in memory are segments of ``src`` floats read as ``dst``
        columns, the rest zero -- values and gradients bit for bit those of the rows gathered and padded dense.  A ``torch.autograd.Function`` whose inputs are the parameters of the module the
        network was built or last ``load``ed from (float32 CUDA tensors on the env's device): ``loss.backward()`` fills their ``.grad``, so ``clip_grad_norm_`` and
        ``torch.optim.Adam`` work unchanged.  The forward is the EXACT fp32 chain whatever mode the network runs in (``sigmaenv_mlp32_forward_save``).  The gradient
        with respect to the input: a network made with ``input_grad=True`` takes a dense ``x`` with ``requires_grad`` and its ``backward`` fills ``x.grad``
        (``sigmaenv_mlp32_backward_dx``; once differentiable); without the flag ``x.requires_grad`` raises ``NotImplementedError``, and so does ``rows=(base, ...)``
        with ``base.requires_grad`` in both cases (a gradient scattered into a record is not built).

        Stale weights: the packed weights on the device are those of construction / the last ``load``.  If a parameter has been modified in place since (the
        optimiser stepped and ``load`` was not called) ``apply`` raises ``RuntimeError``: the forward would use the old numbers and credit the gradient to the new.

        Streams: the kernels run on the env's stream after everything torch's current stream holds, and torch's current stream then waits for them -- forwards
        and backwards alike (``SigmaEnv._on_stream``, the one statement of that order)."""
        through_x = self._input_grad and isinstance(x, torch.Tensor) and x.requires_grad
        spec, shape = self._rows_spec(x.detach() if through_x else x, rows, env, index, check_index, pad)
        for t in self._params:
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.device == env.device):
                raise TypeError(f"apply: the network's parameters must be float32 CUDA tensors on {env.device}: load(env, module) with the module on the device first")
        if any(t._version != v for t, v in zip(self._params, self._param_versions)):
            raise RuntimeError("apply: a parameter changed since the network was built or last loaded (an optimiser step?): call load(env, module) first -- the device "
                               "holds the old weights")
        if through_x:
            return _Mlp32InputFunction.apply(self, env, shape, x, *self._params)
        return _Mlp32Function.apply(self, env, spec, shape, *self._params)


def check_record(t, shape, what: str):
    """A rollout record the device loop writes: a contiguous float32 CUDA tensor of exactly ``shape``."""
    if not isinstance(t, torch.Tensor) or not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise TypeError(f"{what} must be a contiguous float32 CUDA tensor {list(shape)}")
    return t


def check_index(index, env, what: str):
    """A minibatch's frame or block indices: a contiguous int32 CUDA tensor ``[M]`` on the env's device."""
    if not (isinstance(index, torch.Tensor) and index.is_cuda and index.dtype == torch.int32 and index.dim() == 1 and index.is_contiguous() and index.device == env.device):
        raise TypeError(f"{what}: index must be a contiguous int32 CUDA tensor [M] on {env.device}")
    return index


def check_slab(slab, W: int, what: str = "slab", Bt: str = "Bt"):
    """The record rows of a rollout: a contiguous float32 CUDA tensor ``[T, Bt, W]`` (``Bt``: the name the message gives the buffer's env count)."""
    if not isinstance(slab, torch.Tensor) or not (slab.is_cuda and slab.dtype == torch.float32 and slab.is_contiguous() and slab.dim() == 3 and slab.shape[2] == W):
        raise TypeError(f"{what} must be a contiguous float32 CUDA tensor [T, {Bt}, {W}]")
    return slab


def check_rows(net, base, offset, rows_per_block, row_stride, n_blocks, block_stride, pad, what: str):
    """The row addressing of ``forward_rows`` / ``apply(rows=)`` inside ``base``, checked: row ``t * rows_per_block + b`` starts at float ``offset + t * block_stride +
    b * row_stride`` and is ``net._pad(pad)``'s width in memory.  Returns ``(offset, rows_per_block, row_stride, n_blocks, block_stride, src, dst)`` as ints."""
    offset, rpb, rs, nb, bs = int(offset), int(rows_per_block), int(row_stride), int(n_blocks), int(block_stride)
    src, dst, width = net._pad(pad, what)
    if rpb < 0 or nb < 0 or offset < 0 or rs < width or bs < 0:
        raise ValueError(f"{what}: counts and offsets must be >= 0 and row_stride >= the width of a row in memory, {width}")
    if rpb and nb and offset + (nb - 1) * bs + (rpb - 1) * rs + width > base.numel():
        raise ValueError(f"{what}: the last row ends beyond the tensor")
    return offset, rpb, rs, nb, bs, src, dst


class Critic(Mlp32):
    """The MAPPO critic (optimization_module.py:16-32): ``MultiAgentMLP(centralised=True, share_params=True, depth=3, num_cells=256, Tanh)`` --
    one shared MLP on the concatenated observations of all agents of an env; its output is the state value of every agent of that env."""

    def values(self, env: SigmaEnv, obs: torch.Tensor | None = None) -> torch.Tensor:
        """[B, N, 1] state values of ``env.obs`` (or ``obs [B, N, D]``)."""
        o = env.obs if obs is None else obs
        if self.in_dim != env.N * env.D:
            raise ValueError(f"critic input width {self.in_dim} != n_agents * obs_dim = {env.N * env.D}")
        v = self.forward(env, o.reshape(env.B, env.N * env.D))
        return v.reshape(env.B, 1, 1).expand(env.B, env.N, 1)

    def _padded(self, env, pad, what):
        """``pad = (D, Dc)`` of a critic on base observations (prioritized action propagation: ``N (D + 2 K)`` inputs) checked; returns ``Dc``, the agent's width"""
        if pad is None:
            return env.D
        src, dst, _ = self._pad(pad, what)
        if src != env.D or self.in_dim != env.N * dst:
            raise ValueError(f"{what}: pad = ({src}, {dst}) is not (obs_dim = {env.D}, the critic's input width / n_agents = {self.in_dim // env.N})")
        return dst

    def rollout_values(self, env: SigmaEnv, slab: torch.Tensor, obs_rec: torch.Tensor, T: int, env_first: int = 0, state_value: torch.Tensor | None = None,
                       next_state_value: torch.Tensor | None = None, pad=None):
        """The critic's two passes of GAE over the records of a ``T``-step rollout, read where they lie (``forward_rows``: no slice, no staging copy):
        ``state_value [T, B]`` from the root observations ``obs_rec [T, Bt, N, D]`` and ``next_state_value [T, B]`` from the observation part of the record rows
        ``slab [T, Bt, W]``.  ``Bt >= env.B``: the buffers of the whole batch, of which ``env`` owns the envs ``[env_first, env_first + env.B)`` (an env shard;
        ``Bt = env.B`` and 0 for a single handle).  Both sides are computed (as torchrl's GAE runs its value network on both); nothing is reused across steps.
        ``pad = (D, Dc)``: the base critic under prioritized action propagation, centralised on ``N Dc`` inputs -- ``obs_rec`` is then the base-observation record
        ``[T, Bt, N, Dc]`` (``Actor.rollout(base_obs=)``), and the next rows are the record's next observations with every agent's ``Dc - D`` placeholder columns
        zero (the reference's ``("next", base_observation)`` is the env's own output, not the policy-modified row), staged padded without a padded copy."""
        T, B, N, D = int(T), env.B, env.N, self._padded(env, pad, "rollout_values")
        W, e0 = N * (env.D + 1) + 1, int(env_first)
        if self.in_dim != N * D or self.out_dim != 1:
            raise ValueError(f"the critic maps n_agents * obs_dim = {N * D} inputs to 1 value, not {self.in_dim} to {self.out_dim}")
        if T < 1 or slab.dim() != 3 or slab.shape[0] < T or slab.shape[2] != W:
            raise TypeError(f"slab must be [>= {T}, Bt, {W}]")
        Bt = slab.shape[1]
        if not 0 <= e0 <= Bt - B:
            raise ValueError(f"envs [{e0}, {e0 + B}) are not inside the buffers' {Bt}")
        if obs_rec.dim() < 2 or obs_rec.shape[0] < T or obs_rec.shape[1] != Bt or obs_rec[0, 0].numel() != N * D:
            raise TypeError(f"obs_rec must be [>= {T}, {Bt}, {N}, {D}]")
        sv = self.forward_rows(env, obs_rec, e0 * N * D, B, N * D, T, Bt * N * D, out=state_value)
        nv = self.forward_rows(env, slab, e0 * W, B, W, T, Bt * W, out=next_state_value, pad=pad)
        return sv.view(T, B), nv.view(T, B)


    def apply(self, env: SigmaEnv, record: torch.Tensor, T: int | None = None, env_first: int = 0, t_first: int = 0, index: torch.Tensor | None = None,  # noqa: D102
              check_index: bool = True, pad=None) -> torch.Tensor:
        """``[T, B]`` state values with a ``grad_fn`` (``Mlp32.apply``) of the time slices ``[t_first, t_first + T)`` of a rollout record, read where they lie as
        ``rollout_values`` reads them: ``record`` is the root-observation record ``obs_rec [>= t_first + T, Bt, N, D]`` or the record rows ``slab [.., Bt, W]``
        (their observation part: the next observations); ``env`` owns the envs ``[env_first, env_first + env.B)`` of the buffer.  With ``index`` (int32 CUDA ``[M]``,
        ``Mlp32.apply``): the ``T * B`` frames ``f = t * B + b`` of those slices are blocks of one row each and the result is ``[M]``, the values of the frames
        ``index[m]`` (the record must be the env's own: ``Bt == env.B``).  ``pad = (D, Dc)`` (``rollout_values``'s): the critic on base observations -- ``record``
        is the base-observation record ``[.., Bt, N, Dc]``, read as it lies, or ``slab``, whose next observations are read padded (with ``index``)."""
        B, N, D = env.B, env.N, self._padded(env, pad, "apply")
        W = N * (env.D + 1) + 1
        if self.in_dim != N * D or self.out_dim != 1:
            raise ValueError(f"the critic maps n_agents * obs_dim = {N * D} inputs to 1 value, not {self.in_dim} to {self.out_dim}")
        if not isinstance(record, torch.Tensor) or record.dim() < 3:
            raise TypeError("record must be obs_rec [T, Bt, N, D] or slab [T, Bt, W]")
        Bt, width = record.shape[1], record[0, 0].numel()
        if width not in (N * D, W):
            raise TypeError(f"record rows of {width} floats: neither [N, {D}] observations nor record rows of {W}")
        if width != W or record.dim() != 3:
            pad = None  # (the base-observation record holds the padded rows themselves)
        T, e0, t0 = int(record.shape[0] - t_first if T is None else T), int(env_first), int(t_first)
        if T < 0 or t0 < 0 or t0 + T > record.shape[0] or not 0 <= e0 <= Bt - B:
            raise ValueError(f"time slices [{t0}, {t0 + T}) / envs [{e0}, {e0 + B}) are not inside the record {list(record.shape)}")
        if index is not None:
            if Bt != B:
                raise ValueError(f"apply: frames are indexed in the env's own record (Bt == B = {B}), not in a buffer of {Bt} envs")
            return super().apply(env, rows=(record, t0 * Bt * width, 1, width, T * B, width), index=index, check_index=check_index, pad=pad).view(-1)
        if pad is not None:
            raise TypeError("apply: the padded next rows of slab are built for frames picked by index")
        return super().apply(env, rows=(record, (t0 * Bt + e0) * width, B, width, T, Bt * width)).view(T, B)


def make_priority_mlp(obs_dim: int, hidden: int = 256) -> torch.nn.Sequential:
    """The priority actor's network in plain torch.nn (priority_module.py:34-51: ``MultiAgentMLP(depth=2, num_cells=256, Tanh)``, 2 outputs = loc, scale)."""
    return torch.nn.Sequential(torch.nn.Linear(obs_dim, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, 2))


class PriorityNet(Mlp32):
    """The priority module (sigmarl/modules/priority_module.py): an fp32 network obs_dim -> 256 -> 256 -> 2 on the priority observation (``SigmaEnv.obs``,
    without placeholder columns), a 1-D TanhNormal on [-1, 1] for the scores and ``rank_agents`` (agents by descending score; ties to the lower index).
    ``forward`` is the network alone (``Mlp32``); ``scores`` runs all three (``sigmaenv_priority_forward``)."""

    def __init__(self, mlp: torch.nn.Module, lib: capi.Library | None = None, mode: str = "split", input_grad: bool = False):
        super().__init__(mlp, lib, mode, input_grad)
        if self.out_dim != 2:
            raise ValueError("a priority network has 2 outputs (loc, scale)")

    def scores(self, env: SigmaEnv, obs: torch.Tensor | None = None, seed: int = 0, counter: int = 0, deterministic: bool = False):
        """(scores [B,N], log_prob [B,N], ranks [B,N] int32) of ``env.obs`` (or ``obs [B*N, obs_dim]``); enqueued on the env's stream."""
        if self.in_dim != (obs.shape[-1] if obs is not None else env.D):
            raise ValueError(f"priority network input width {self.in_dim} != observation width")
        kw = dict(dtype=torch.float32, device=env.device)
        scratch, sc, lp = torch.empty((env.B * env.N, 2), **kw), torch.empty((env.B, env.N), **kw), torch.empty((env.B, env.N), **kw)
        ranks = torch.empty((env.B, env.N), dtype=torch.int32, device=env.device)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        env._chk(env.lib.priority_forward(env.h, self.handle(env.lib, env), p(obs), p(scratch), p(sc), p(lp), p(ranks), int(seed), int(counter), int(bool(deterministic))),
                 "priority_forward")
        return sc, lp, ranks


def rank_scores(env: SigmaEnv, scores: torch.Tensor) -> torch.Tensor:
    """``sigmaenv_priority_rank``: ranks [B,N] int32 of ``scores [B,N]`` (descending; ties to the lower agent index)."""
    if not (scores.is_cuda and scores.dtype == torch.float32 and scores.is_contiguous() and tuple(scores.shape) == (env.B, env.N)):
        raise TypeError(f"scores must be a contiguous float32 CUDA tensor [{env.B}, {env.N}]")
    ranks = torch.empty((env.B, env.N), dtype=torch.int32, device=env.device)
    env._chk(env.lib.priority_rank(env.h, C.c_void_p(scores.data_ptr()), C.c_void_p(ranks.data_ptr())), "priority_rank")
    return ranks


def random_ranks(env: SigmaEnv, seed: int = 0, counter: int = 0) -> torch.Tensor:
    """``sigmaenv_priority_random``: one uniform permutation of the agents per env ([B,N] int32; prioritization_method "random")."""
    ranks = torch.empty((env.B, env.N), dtype=torch.int32, device=env.device)
    env._chk(env.lib.priority_random(env.h, int(seed), int(counter), C.c_void_p(ranks.data_ptr())), "priority_random")
    return ranks


class Actor:
    def __init__(self, mlp: torch.nn.Module, low, high, lib: capi.Library | None = None, precision: str = "fp32", mode: str = "split", input_grad: bool = False):
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision must be 'fp32' (the reference's arithmetic) or 'bf16' (fast inference variant)")
        self.precision = precision
        self.lib = lib or capi.load_library()
        self._mlp32 = Mlp32(mlp, self.lib, mode=mode, input_grad=input_grad)  # the exact network (also kept by the bf16 variant: a caller may ask for either per call)
        import weakref

        self._scratch_by_env = weakref.WeakKeyDictionary()  # SigmaEnv -> {kind: tensor}
        lin = [m for m in mlp.modules() if isinstance(m, torch.nn.Linear)]
        if len(lin) != 4 or lin[1].in_features != 256 or lin[2].out_features != 256 or lin[3].out_features != 4:
            raise ValueError("expected Linear(D,256), Linear(256,256), Linear(256,256), Linear(256,4)")
        self.obs_dim = lin[0].in_features
        arrs = []
        for m in lin:
            arrs.append(np.ascontiguousarray(m.weight.detach().cpu().numpy(), np.float32))
            arrs.append(np.ascontiguousarray(m.bias.detach().cpu().numpy(), np.float32))
        self._keep = arrs + [np.ascontiguousarray(low, np.float32), np.ascontiguousarray(high, np.float32)]
        # the bf16 kernel handle exists only for the widths its MFMA tiling takes (sigmaenv_actor_create: obs_dim in {8, 16, 24, 32}); other
        # observation switches (e.g. is_obs_steering: 35) run the fp32 network, which takes any width
        self._bf16 = {}  # library path -> (library, handle): see Mlp32
        self._bf16_version = {}  # library path -> the version of the weights the handle holds (Mlp32._version)
        if precision == "bf16":
            self._bf16_handle(self.lib)

    def _bf16_handle(self, lib: capi.Library, env: SigmaEnv | None = None):
        ent = self._bf16.get(lib.path)
        if ent is None:
            if self.obs_dim not in (8, 16, 24, 32):
                raise ValueError(f"the bf16 actor kernel takes obs_dim 8, 16, 24 or 32, not {self.obs_dim}: use precision='fp32' for this observation layout")
            h = C.c_void_p()
            rc = lib.actor_create(self.obs_dim, *[a.ctypes.data_as(C.c_void_p) for a in self._keep], C.byref(h))
            if rc != 0:
                raise RuntimeError(f"sigmaenv_actor_create failed with code {rc}")
            ent = self._bf16[lib.path] = (lib, h)
            self._bf16_version[lib.path] = 0
        if env is not None and self._bf16_version[lib.path] != self._mlp32._version:
            self._pack_bf16([env])
        return ent[1]

    def _pack_bf16(self, group):
        self._mlp32._ensure_snapshot(group[0])
        lib = group[0].lib
        h = self._bf16_handle(lib)
        wp, bp = self._mlp32._device_pointers()
        self._mlp32._ordered_pack(group, lambda env: env._chk(lib.actor_load_device(env.h, h, wp, bp), "actor_load_device"))
        self._bf16_version[lib.path] = self._mlp32._version

    def load(self, env, source) -> str:
        """New weights for the actor from the learner's tensors on the device (``Mlp32.load``: the same ``source``, refusals, stream order and host wait; ``env``
        is one env or the shards that share this actor).  Refreshes the fp32 network and the bf16 one wherever it exists (an actor of ``precision="bf16"`` gets
        it for every given env's library); ``low`` / ``high`` stay.  Returns the fp32 network's mode in force."""
        envs = _env_list(env)
        ws, bs = load_source([self.obs_dim, 256, 256, 256, 4], source, envs[0].device)
        mode = self._mlp32._load(envs, ws, bs)
        self._mlp32._remember(source_pairs(source))
        for group in _by_library(envs):
            if self.precision == "bf16" or group[0].lib.path in self._bf16:
                self._pack_bf16(group)
        return mode

    def apply(self, env: SigmaEnv, x: torch.Tensor | None = None, *, rows=None, index: torch.Tensor | None = None, check_index: bool = True) -> torch.Tensor:
        """The fp32 network's four outputs per row with a ``grad_fn`` (``Mlp32.apply``: same arguments, stale-weight guard and stream order; ``index``: a minibatch
        of frames, blocks of ``N`` rows).  The loss head on top of it -- log-probability of the recorded action, ratio, clip, entropy -- is ``learn.ppo_head``."""
        return self._mlp32.apply(env, x, rows=rows, index=index, check_index=check_index)

    def close(self):
        for lib, h in getattr(self, "_bf16", {}).values():
            lib.actor_destroy(h)
        self._bf16, self._bf16_version = {}, {}
        if getattr(self, "_mlp32", None) is not None:
            self._mlp32.close()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    # Scratch buffers are keyed PER ENV OBJECT: one Actor may drive several env shards on their own streams (bench.py --policy --streams 2), and a buffer shared by two
    # shards of equal size would be overwritten by the other shard's launches.  The key is the SigmaEnv itself, held weakly (the raw handle
    # address can be handed to a NEW env after close() -- same B, larger N: an undersized buffer, written past its end -- and the entries of closed envs never went
    # away); the FULL shape is compared as well.
    def _scratch(self, kind: str, env: SigmaEnv, shape, zero: bool) -> torch.Tensor:
        per_env = self._scratch_by_env.setdefault(env, {})
        t = per_env.get(kind)
        if t is None or tuple(t.shape) != tuple(shape) or t.device != env.device:
            t = (torch.zeros if zero else torch.empty)(tuple(shape), dtype=torch.float32, device=env.device)
            per_env[kind] = t
        return t

    def _scratch_actions(self, env: SigmaEnv) -> torch.Tensor:
        return self._scratch("a", env, (env.B, env.N, 2), True)

    def _scratch_out4(self, env: SigmaEnv) -> torch.Tensor:
        return self._scratch("o", env, (env.B * env.N, 4), False)

    def forward(self, env: SigmaEnv, actions: torch.Tensor, log_prob: torch.Tensor | None = None, loc_scale: torch.Tensor | None = None,
                obs: torch.Tensor | None = None, seed: int = 0, counter: int = 0, deterministic: bool = False, precision: str | None = None):
        """actions[B,N,2] := policy(env.obs or ``obs``); enqueued on the env's stream."""
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        if (precision or self.precision) == "fp32":
            lo, hi = self._keep[-2], self._keep[-1]
            env._chk(env.lib.actor_forward_f32(env.h, self._mlp32.handle(env.lib, env), p(obs), p(self._scratch_out4(env)), lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p),
                                               p(actions), p(log_prob), p(loc_scale), int(seed), int(counter), int(bool(deterministic))), "actor_forward_f32")
            return actions
        env._chk(env.lib.actor_forward(env.h, self._bf16_handle(env.lib, env), p(obs), p(actions), p(log_prob), p(loc_scale), int(seed), int(counter), int(bool(deterministic))),
                 "actor_forward")
        return actions

    def rollout(self, env: SigmaEnv, n_steps: int, slab: torch.Tensor | None = None, log_prob: torch.Tensor | None = None,
                actions: torch.Tensor | None = None, seed: int = 0, counter0: int = 0, path_first: int | None = None, path_count: int | None = None,
                deterministic: bool = False, precision: str | None = None, slab_ptr: int | None = None, wrapper: str | None = None,
                priority=None, tentative: torch.Tensor | None = None, ranks: torch.Tensor | None = None, scores: torch.Tensor | None = None,
                score_log_prob: torch.Tensor | None = None, obs_rec: torch.Tensor | None = None, base_obs: torch.Tensor | None = None,
                communication_noise=None):
        """``n_steps`` x (policy -> fused step + record + resets) enqueued back to back; optional records ``slab [T,B,W]``,
        ``log_prob [T,B,N]``, ``actions [T,B,N,2]`` (CUDA float32, contiguous).  ``slab_ptr``: the record target as a raw device address instead of ``slab`` (an env
        shard's first row inside a ``[T, B_total, W]`` buffer of the whole batch, with ``env.set_rollout_slab_stride(B_total * W)``).  ``precision`` (default: the actor's): "fp32" = the reference's
        arithmetic (``sigmaenv_rollout_f32``), "bf16" = the fast inference variant (``sigmaenv_rollout``).

        ``wrapper`` (fp32 only; ``params.rollout_wrapper`` gives the collector's choice for a ``Parameters``): ``None`` = the plain policy as above;
        ``"plain"`` = the same through ``sigmaenv_rollout_f32_ex``; ``"opponent"`` = opponent modelling (the env needs ``is_using_opponent_modeling``);
        ``"prioritized"`` = prioritized action propagation (the actor takes obs_dim + 2 n_nearing inputs) with ``priority`` = a ``PriorityNet``, ``"random"``
        or a rank tensor [B,N] int32 (CUDA).  Records: ``tentative [T,B,N,K,2]`` (the neighbour actions the policy saw), ``ranks [T,B,N]`` int32,
        ``scores`` / ``score_log_prob [T,B,N]`` (``PriorityNet`` only), ``base_obs [T,B,N,D + 2 K]`` (``"prioritized"`` only): the row every agent was evaluated on in
        its turn -- its ``env.obs`` row, then the 2 K neighbour-action columns it saw (the reference's ``base_observation``) --, written by the turn's gather, every
        row once per step.  Step semantics: include/sigmaenv.h, sigmaenv_rollout_f32_ex.

        ``communication_noise`` (``"prioritized"`` only, 2 observed neighbours; ``params.communication_noise`` gives it for a ``Parameters``): the reference's
        ``communication_noise_level`` -- a float, or a float32 CUDA tensor ``[B]`` of per-env levels (one rollout over a sweep of levels,
        ``evaluate.noise_sweep``; a float64 tensor is taken too: its envs compute what the float of the same value computes).  Every agent then
        sees the 2 K propagated-action columns of its turn plus a normal draw of std ``[s_v, s_v, s_d, s_d]``,
        ``s_v = max_speed * level``, ``s_d = max_steering * level`` (by the column's position, as the reference adds them: helper_training.py:1271-1287), drawn per
        (env, agent, step) from the rollout's key, also when ``deterministic``.  ``tentative`` and ``base_obs`` record the noisy values the actor was evaluated on;
        ``actions`` and the step stay clean.  Level 0.0 is the rollout without the argument.  The stds are formed on the host as the reference forms them (the
        double product, rounded to float32); the levels of a tensor are the caller's and are not checked (a NaN level gives NaN rows).

        ``obs_rec [T,B,N,D]`` (any precision, any wrapper): the root observations -- row t = ``env.obs`` as the final actor forward of step t read it, i.e. the
        ``observation`` of the collector's tensordict (the record row of step t - 1 holds it only where nothing was re-placed).  ``None``: the handle's setting is
        left as it is (off unless ``env.set_rollout_obs_record`` set it, as an env shard that records into the whole batch's buffer does).

        Inside ``initial_states.InitialStateBank(env).attached()`` every step runs as step -> record -> restart -> auto_reset -> settle (``sigmaenv_isb_attach``).
        An env whose parameters set ``is_challenging_initial_state_buffer`` is refused (``NotImplementedError``) without one."""
        check_rollout_wrapper(getattr(env, "parameters", None), wrapper, communication_noise)
        check_initial_state_bank(getattr(env, "parameters", None), getattr(env, "_initial_states", None) is not None)
        if obs_rec is not None:
            check_record(obs_rec, (int(n_steps), env.B, env.N, env.D), "obs_rec")
            env.set_rollout_obs_record(obs_rec)
            try:
                return self.rollout(env, n_steps, slab, log_prob, actions, seed, counter0, path_first, path_count, deterministic, precision, slab_ptr, wrapper, priority,
                                    tentative, ranks, scores, score_log_prob, base_obs=base_obs, communication_noise=communication_noise)
            finally:
                env.set_rollout_obs_record(None)  # (the copies are enqueued: the setting is only read while the loop enqueues)
        if path_first is None:
            path_first, path_count = env.default_paths()
        scratch = self._scratch_actions(env)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        p_slab = C.c_void_p(int(slab_ptr)) if slab_ptr else p(slab)
        if wrapper is not None:
            if (precision or self.precision) != "fp32":
                raise ValueError("the rollout wrappers run the fp32 actor (precision='fp32')")
            opts = self._wrapper_opts(env, int(n_steps), wrapper, priority, tentative, ranks, scores, score_log_prob, base_obs, communication_noise)
            lo, hi = self._keep[-2], self._keep[-1]
            env._chk(env.lib.rollout_f32_ex(env.h, self._mlp32.handle(env.lib, env), lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), p(self._scratch_out4(env)),
                                            int(n_steps), p(scratch), p_slab, p(log_prob), p(actions), int(seed), int(counter0), int(path_first), int(path_count),
                                            int(bool(deterministic)), C.byref(opts)), "rollout_f32_ex")
            return
        if base_obs is not None:
            raise ValueError("base_obs belongs to wrapper='prioritized'")
        if communication_noise is not None:
            raise ValueError("communication_noise belongs to wrapper='prioritized'")
        if (precision or self.precision) == "fp32":
            lo, hi = self._keep[-2], self._keep[-1]
            env._chk(env.lib.rollout_f32(env.h, self._mlp32.handle(env.lib, env), lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), p(self._scratch_out4(env)), int(n_steps),
                                         p(scratch), p_slab, p(log_prob), p(actions), int(seed), int(counter0), int(path_first), int(path_count),
                                         int(bool(deterministic))), "rollout_f32")
            return
        env._chk(env.lib.rollout(env.h, self._bf16_handle(env.lib, env), int(n_steps), p(scratch), p_slab, p(log_prob), p(actions), int(seed), int(counter0), int(path_first),
                                 int(path_count), int(bool(deterministic))), "rollout")

    def _noise_opts(self, env: SigmaEnv, opts: capi.RolloutOpts, noise) -> None:
        """``communication_noise`` into ``opts``: the pair ``(s_v, s_d)`` of a float level, or the ``[B, 2]`` pairs of a ``[B]`` tensor of levels."""
        if not hasattr(env.lib, "comm_noise_stds"):  # (a build from before the fields reads them as reserved words and would run without noise)
            raise RuntimeError("communication_noise: this build of the library does not add communication noise")
        if env.K != 2:
            raise NotImplementedError(f"communication_noise with {env.K} observed neighbours: the reference's 4 noise stds fit 2 K = 4 columns only "
                                      "(raises in the reference as well)")
        max_speed, max_steering = capi.AGENTS["max_speed"], capi.AGENTS["max_steering"]
        if isinstance(noise, torch.Tensor):
            if not (noise.is_cuda and noise.dtype in (torch.float32, torch.float64) and noise.device == env.device and tuple(noise.shape) == (env.B,)):
                raise TypeError(f"communication_noise must be a float or a float32 (or float64) CUDA tensor [{env.B}] on {env.device}")
            with torch.cuda.device(env.device):
                env.stream.wait_stream(torch.cuda.current_stream(env.device))
                with torch.cuda.stream(env.stream):
                    level = noise.to(torch.float64)
                    stds = torch.stack((level * max_speed, level * max_steering), dim=-1).to(torch.float32).contiguous()
            noise.record_stream(env.stream)
            opts.comm_noise_std_env = stds.data_ptr()
            self._noise_stds = stds  # (kept alive until the next call: the launches read it asynchronously)
            return
        if isinstance(noise, bool) or not isinstance(noise, (int, float, np.floating, np.integer)):
            raise TypeError(f"communication_noise must be a float or a float32 (or float64) CUDA tensor [{env.B}] on {env.device}")
        level = float(noise)
        if not (np.isfinite(level) and level >= 0.0):
            raise ValueError(f"communication_noise must be finite and >= 0, not {level}")
        opts.comm_noise_std[0], opts.comm_noise_std[1] = float(np.float32(max_speed * level)), float(np.float32(max_steering * level))

    def _wrapper_opts(self, env: SigmaEnv, T: int, wrapper: str, priority, tentative, ranks, scores, score_log_prob, base_obs=None, communication_noise=None) -> capi.RolloutOpts:
        opts = capi.RolloutOpts()
        opts.wrapper = {"plain": capi.WRAP_PLAIN, "opponent": capi.WRAP_OPPONENT, "prioritized": capi.WRAP_PRIORITIZED}[wrapper]

        def rec(t, shape, dtype, what):
            if t is None:
                return None
            if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
                raise TypeError(f"{what} must be a contiguous {dtype} CUDA tensor {list(shape)}")
            return t.data_ptr()

        opts.tentative_rec = rec(tentative, (T, env.B, env.N, env.K, 2), torch.float32, "tentative")
        if wrapper != "prioritized":
            if priority is not None or ranks is not None or scores is not None or score_log_prob is not None or base_obs is not None:
                raise ValueError("priority / ranks / scores / score_log_prob / base_obs belong to wrapper='prioritized'")
            if communication_noise is not None:
                raise ValueError("communication_noise belongs to wrapper='prioritized'")
            return opts
        if communication_noise is not None:
            self._noise_opts(env, opts, communication_noise)
        if base_obs is not None and not hasattr(env.lib, "ppo_head_1d"):  # (SIGMAENV_LIB_OLD_ABI: a build from before the record reads a shorter struct)
            raise RuntimeError("base_obs: this build of the library does not write the base-observation record")
        opts.base_obs_rec = rec(base_obs, (T, env.B, env.N, env.D + 2 * env.K), torch.float32, "base_obs")
        opts.rank_rec = rec(ranks, (T, env.B, env.N), torch.int32, "ranks")
        if isinstance(priority, PriorityNet):
            opts.priority_source = capi.PRIORITY_NET
            opts.priority_net = priority.handle(env.lib, env)
            opts.score_rec = rec(scores, (T, env.B, env.N), torch.float32, "scores")
            opts.score_logp_rec = rec(score_log_prob, (T, env.B, env.N), torch.float32, "score_log_prob")
        else:
            if scores is not None or score_log_prob is not None:
                raise ValueError("scores / score_log_prob are recorded with a PriorityNet only")
            if isinstance(priority, str) and priority == "random":
                opts.priority_source = capi.PRIORITY_RANDOM
            elif isinstance(priority, torch.Tensor):
                opts.priority_source = capi.PRIORITY_GIVEN
                opts.ranks_given = rec(priority, (env.B, env.N), torch.int32, "priority (ranks)")
                self._given_ranks = priority  # (kept alive until the next call: the launches read it asynchronously)
            else:
                raise TypeError("priority must be a PriorityNet, 'random' or an int32 rank tensor [B, N]")
        return opts
