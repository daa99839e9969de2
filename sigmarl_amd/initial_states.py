"""The challenging initial-state buffer on the device (``Parameters.is_challenging_initial_state_buffer``; ``sigmaenv_isb_*`` of include/sigmaenv.h, the
specification: sigmarl_amd/csrc/sigmaenv_isb.h): a per-env history of the last ``n_steps_stored`` states, a circular bank of the scenes ``n_steps_stored`` steps
before an agent-agent collision, and the restart of finished envs from random bank entries -- without a state, an index or a probability visiting the host.

    bank = InitialStateBank(env)                      # capacity 100, probability_record 1.0, probability_use_recording 0.2: the reference's defaults
    with bank.attached():
        actor.rollout(env, T, ...)                    # every step: step -> record -> restart -> auto_reset -> settle
    learn.train(env, actor, critic, initial_states=bank, ...)

The reference cannot run the feature past its first use of a recording (world_state_rt_sim.py:162 raises); the four departures from what its code states are listed in
sigmaenv_isb.h and DESIGN.md section 7."""
from __future__ import annotations

import contextlib
import ctypes as C

import torch

from . import capi
from .env import device_view


class InitialStateBank:
    """One bank of one env (``sigmaenv_isb_create``).  ``n_steps_stored`` defaults to the env's ``Parameters`` value (10 without parameters).  Only ``count`` (and
    ``ptr``) wait; everything else is enqueued on the env's stream."""

    def __init__(self, env, capacity: int = 100, n_steps_stored: int | None = None, probability_record: float = 1.0, probability_use_recording: float = 0.2):
        self.env, self.bank = env, None
        if n_steps_stored is None:
            n_steps_stored = int(getattr(getattr(env, "parameters", None), "n_steps_stored", 10))
        self.capacity, self.n_steps_stored = int(capacity), int(n_steps_stored)
        self.probability_record, self.probability_use_recording = float(probability_record), float(probability_use_recording)
        if not (1 <= self.capacity <= capi.ISB_MAX_CAPACITY and 1 <= self.n_steps_stored <= capi.ISB_MAX_STEPS_STORED):
            raise ValueError(f"InitialStateBank: capacity 1 .. {capi.ISB_MAX_CAPACITY}, n_steps_stored 1 .. {capi.ISB_MAX_STEPS_STORED}")
        if not (0.0 <= self.probability_record <= 1.0 and 0.0 <= self.probability_use_recording <= 1.0):
            raise ValueError("InitialStateBank: probabilities lie in [0, 1]")
        if not hasattr(env.lib, "isb_create"):
            raise RuntimeError("InitialStateBank: this build of the library has no initial-state bank")
        bank = C.c_void_p()
        with torch.cuda.device(env.device):
            env._chk(env.lib.isb_create(env.h, self.capacity, self.n_steps_stored, self.probability_record, self.probability_use_recording, C.byref(bank)), "isb_create")
        self.bank = bank
        self._views = {}
        B, N, S, cap = env.B, env.N, self.n_steps_stored, self.capacity
        layout = {capi.ISB_BANK_STATE: ("f32", (cap, N, 8)), capi.ISB_BANK_PATH: ("i32", (cap, N, 4)), capi.ISB_WORDS: ("i32", (2,)),
                  capi.ISB_RING_STATE: ("f32", (B, S, N, 8)), capi.ISB_RING_PATH: ("i32", (B, S, N, 4)), capi.ISB_HELD: ("i32", (B,)), capi.ISB_HEAD: ("i32", (B,)),
                  capi.ISB_PENDING: ("u8", (B,))}
        if hasattr(env.lib, "state_save"):  # (an older build under SIGMAENV_LIB_OLD_ABI=1 has neither the snapshot entry points nor this id)
            layout[capi.ISB_EPISODES] = ("i32", (B,))
        for what, (kind, shape) in layout.items():
            p, nb = C.c_void_p(), C.c_size_t()
            env._chk(env.lib.isb_get(env.h, self.bank, what, C.byref(p), C.byref(nb)), "isb_get")
            self._views[what] = device_view(p.value, shape, kind, env.device.index, self)

    def close(self):
        if getattr(self, "bank", None) and getattr(self.env, "h", None):
            if getattr(self.env, "_initial_states", None) is self:
                self.env._initial_states = None
            self.env.lib.isb_destroy(self.bank)
        self.bank = None
        self._views = {}

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ---- the calls --------------------------------------------------------------------------------------------------
    def reset(self):
        """Empties the bank and every ring, then pushes every env's current rows (``sigmaenv_isb_reset``)."""
        self.env._chk(self.env.lib.isb_reset(self.env.h, self.bank), "isb_reset")

    def record(self, seed: int = 0, counter: int = 0):
        """On the frame a step left, before any reset: push, the record decisions, the ordered bank writes, ``pending`` (``sigmaenv_isb_record``)."""
        self.env._chk(self.env.lib.isb_record(self.env.h, self.bank, int(seed), int(counter)), "isb_record")

    def restart(self, seed: int = 0, counter: int = 0):
        """Before ``env.auto_reset``: finished envs restart from a random bank entry with ``probability_use_recording`` (``sigmaenv_isb_restart``)."""
        self.env._chk(self.env.lib.isb_restart(self.env.h, self.bank, int(seed), int(counter)), "isb_restart")

    def settle(self):
        """After ``env.auto_reset``: every env that was reset, wholly or in one agent, starts its history anew (``sigmaenv_isb_settle``)."""
        self.env._chk(self.env.lib.isb_settle(self.env.h, self.bank), "isb_settle")

    @contextlib.contextmanager
    def attached(self):
        """While inside, every step of ``Actor.rollout`` on this env runs as step -> record -> restart -> auto_reset -> settle (``sigmaenv_isb_attach``); always
        detaches."""
        self.env._chk(self.env.lib.isb_attach(self.env.h, self.bank), "isb_attach")
        self.env._initial_states = self
        try:
            yield self
        finally:
            self.env._initial_states = None
            self.env._chk(self.env.lib.isb_attach(self.env.h, None), "isb_attach")

    # ---- contents ---------------------------------------------------------------------------------------------------
    def view(self, what: int) -> torch.Tensor:
        """Zero-copy view of one of the bank's device arrays (``capi.ISB_*``): for tests and checkpoints."""
        return self._views[what]

    _STATE_KEYS = {"bank_state": capi.ISB_BANK_STATE, "bank_path": capi.ISB_BANK_PATH, "words": capi.ISB_WORDS, "ring_state": capi.ISB_RING_STATE,
                   "ring_path": capi.ISB_RING_PATH, "held": capi.ISB_HELD, "head": capi.ISB_HEAD, "pending": capi.ISB_PENDING, "episodes": capi.ISB_EPISODES}

    def state_dict(self) -> dict:
        """Every word of the bank and of the rings (copies on the device, enqueued behind the env's stream; ``.cpu()`` them for a file) with the four settings."""
        if capi.ISB_EPISODES not in self._views:
            raise RuntimeError("InitialStateBank.state_dict: this build of the library does not expose the bank's episodes copy")
        e = self.env
        with torch.cuda.device(e.device):
            torch.cuda.current_stream(e.device).wait_stream(e.stream)
        d = {k: self._views[w].clone() for k, w in self._STATE_KEYS.items()}
        d.update(capacity=self.capacity, n_steps_stored=self.n_steps_stored, probability_record=self.probability_record,
                 probability_use_recording=self.probability_use_recording)
        return d

    def load_state_dict(self, d: dict) -> None:
        """The inverse: refuses (before any copy) a dict of another ``capacity`` / ``n_steps_stored`` or with a tensor of another shape or dtype; the message names
        it.  The probabilities are settings of this object and stay."""
        if capi.ISB_EPISODES not in self._views:
            raise RuntimeError("InitialStateBank.load_state_dict: this build of the library does not expose the bank's episodes copy")
        for k in ("capacity", "n_steps_stored"):
            if int(d[k]) != getattr(self, k):
                raise ValueError(f"InitialStateBank.load_state_dict: {k} is {d[k]} in the dict, {getattr(self, k)} here")
        for k, w in self._STATE_KEYS.items():
            t, v = d[k], self._views[w]
            if not isinstance(t, torch.Tensor) or t.shape != v.shape or t.dtype != v.dtype:
                raise ValueError(f"InitialStateBank.load_state_dict: {k} must be a {v.dtype} tensor {list(v.shape)}")
        e = self.env
        with torch.cuda.device(e.device):
            cur = torch.cuda.current_stream(e.device)
            cur.wait_stream(e.stream)
            for k, w in self._STATE_KEYS.items():
                self._views[w].copy_(d[k].to(e.device))
            e.stream.wait_stream(cur)

    @property
    def count(self) -> int:
        """Entries held (waits for the env's stream)."""
        self.env.sync()
        return int(self._views[capi.ISB_WORDS][1].item())

    @property
    def ptr(self) -> int:
        """The slot the next recording goes to (waits)."""
        self.env.sync()
        return int(self._views[capi.ISB_WORDS][0].item())

    def entries(self):
        """``(state [count, N, 8] float32, path [count, N, 4] int32)``: copies of the entries held, in slot order (waits for ``count``)."""
        n = self.count
        return self._views[capi.ISB_BANK_STATE][:n].clone(), self._views[capi.ISB_BANK_PATH][:n].clone()

    def load(self, state: torch.Tensor, path: torch.Tensor):
        """Loads ``state [n, N, 8]`` float32 / ``path [n, N, 4]`` int32 (CUDA, contiguous; ``n <= capacity``) as the bank's first ``n`` entries and sets
        ``count = n``: a saved bank (``entries()``), or a hand-made scenario set.  The rows are ``BUF_STATE`` / ``BUF_PATH`` rows."""
        e = self.env
        n = int(state.shape[0]) if isinstance(state, torch.Tensor) and state.dim() == 3 else -1
        ok = (isinstance(state, torch.Tensor) and isinstance(path, torch.Tensor) and state.is_cuda and path.is_cuda and state.dtype == torch.float32 and path.dtype == torch.int32
              and state.is_contiguous() and path.is_contiguous() and tuple(state.shape) == (n, e.N, 8) and tuple(path.shape) == (n, e.N, 4) and 0 <= n <= self.capacity)
        if not ok:
            raise TypeError(f"InitialStateBank.load: contiguous CUDA tensors state [n, {e.N}, 8] float32 and path [n, {e.N}, 4] int32 with n <= {self.capacity}")
        with torch.cuda.device(e.device):
            e.stream.wait_stream(torch.cuda.current_stream(e.device))
        e._chk(e.lib.isb_set(e.h, self.bank, C.c_void_p(state.data_ptr()) if n else None, C.c_void_p(path.data_ptr()) if n else None, n), "isb_set")
        state.record_stream(e.stream)
        path.record_stream(e.stream)
