"""Frames of selected envs, drawn on the device: a top-down view of map, short-term reference paths and vehicles.

The reference looks at a rollout through ``env.render`` / ``extra_render`` (``sigmarl/scenarios/road_traffic.py:1637-1800``) and ``save_video``: a pyglet scene graph
behind ``is_save_simulation_video``, ``is_real_time_rendering``, ``is_visualize_short_term_path`` and ``is_visualize_lane_boundary``.  Here ``Renderer`` is a device
object beside the env (``sigmaenv_render_*``, include/sigmaenv.h; the pixels are specified in csrc/sigmaenv_render.h): one launch per frame on the env's stream, no
host wait, ``uint8`` RGB frames ``[n_sel, H, W, 3]`` of the envs a selection names.  ``frame()`` draws the buffers as they stand (or tensors given in their place: a
recorded trajectory), ``attached()`` lets ``Actor.rollout`` / ``evaluate.evaluate(render=)`` draw every ``every``-th step into a ring of frames -- the step's outcome
BEFORE the resets clear its collisions --, ``video()`` is the ring in time order and ``save()`` writes it.

Not drawn (out of scope): text (``render_title``, the clock), the CBF and nominal action arrows, the group outlines, a camera that follows an env.

The default palette, ``default_palette(N)``: background ``(255, 255, 255)``, lane boundaries ``(96, 96, 96)``, collision ``(255, 0, 0)``, then agent ``i`` of ``N`` at
hue ``h = (0.58 + i / N) mod 1`` -- equally spaced, starting at blue so that no agent is close to the collision red for small ``N`` --, saturation ``0.65`` and value
``0.85``, converted with the usual HSV sextant formula (``colorsys.hsv_to_rgb``) and rounded to ``uint8`` by ``int(255 v + 0.5)``.  The heading mark is black.
"""
from __future__ import annotations

import colorsys
import contextlib
import ctypes as C

import numpy as np
import torch

from . import capi

H_BOUNDARY_M, H_PATH_M = 0.01, 0.01  # default half-widths in metres (scaled by the view; at least half a pixel)


def default_palette(n_agents: int) -> np.ndarray:
    """``u8 [3 + N, 3]``: background, boundary, collision, the agents (the formula: module docstring)."""
    rows = [(255, 255, 255), (96, 96, 96), (255, 0, 0)]
    for i in range(int(n_agents)):
        rgb = colorsys.hsv_to_rgb((0.58 + i / int(n_agents)) % 1.0, 0.65, 0.85)
        rows.append(tuple(int(255 * v + 0.5) for v in rgb))
    return np.asarray(rows, np.uint8)


def fit_view(world_x_dim: float, world_y_dim: float, width: int, height: int | None = None):
    """``(scale, x0, y1, height)`` of the view that fits ``[0, world_x_dim] x [0, world_y_dim]`` into ``width`` (x ``height``) pixels, centred.  ``height=None``: from
    the aspect ratio, rounded up to a multiple of 4."""
    width = int(width)
    if height is None:
        height = int(np.ceil(width * float(world_y_dim) / float(world_x_dim)))
        height = (height + 3) // 4 * 4
    height = int(height)
    scale = min(width / float(world_x_dim), height / float(world_y_dim))
    x0 = float(world_x_dim) / 2 - width / (2 * scale)
    y1 = float(world_y_dim) / 2 + height / (2 * scale)
    return float(np.float32(scale)), float(np.float32(x0)), float(np.float32(y1)), height


def check_image(width: int, height: int, samples: int, selection, n_envs: int) -> np.ndarray:
    """The library's refusals at create, made on the host before the call; returns the selection as ``int32 [n_sel]``."""
    if int(width) < 4 or int(width) % 4 or int(width) > capi.RND_MAX_DIM:
        raise ValueError(f"render: width = {width} must be a multiple of 4 within [4, {capi.RND_MAX_DIM}] (a lane writes four pixels as three dwords)")
    if not 1 <= int(height) <= capi.RND_MAX_DIM:
        raise ValueError(f"render: height = {height} must lie within [1, {capi.RND_MAX_DIM}]")
    if int(samples) not in (1, 2, 4):
        raise ValueError(f"render: samples = {samples} per axis must be 1, 2 or 4")
    sel = np.ascontiguousarray(np.asarray(selection, np.int64).reshape(-1))
    if sel.size < 1 or sel.size > 65535:
        raise ValueError("render: the selection must name 1 .. 65535 envs")
    bad = np.nonzero((sel < 0) | (sel >= int(n_envs)))[0]
    if len(bad):
        raise ValueError(f"render: envs[{int(bad[0])}] = {int(sel[bad[0]])} is outside [0, {int(n_envs)})")
    return sel.astype(np.int32)


def render_src(vertices_ptr=None, short_term_ptr=None, state_ptr=None, col_agents_ptr=None, col_flags_ptr=None):
    """The ``sigmaenv_render_src_t`` of a frame's overrides (``None`` without any): raw device addresses, each 4-byte aligned -- the library's refusal, made on the
    host before the call."""
    ptrs = dict(vertices=vertices_ptr, short_term=short_term_ptr, state=state_ptr, col_agents=col_agents_ptr, col_flags=col_flags_ptr)
    if all(p is None for p in ptrs.values()):
        return None
    src = capi.RenderSrc()
    for name, p in ptrs.items():
        if p is None:
            continue
        if int(p) == 0 or int(p) & 3:
            raise ValueError(f"render: the {name} override is null or not 4-byte aligned")
        setattr(src, name, int(p))
    return src


class Renderer:
    """The rasteriser of one env (``sigmaenv_render_create``).

    ``envs``: the selection, any order, duplicates allowed.  ``view=None`` fits the map's ``[0, world_x_dim] x [0, world_y_dim]``, centred; otherwise
    ``(scale px/m, x0, y1)`` with ``(x0, y1)`` the world point of the top-left corner (``height`` is then required).  ``samples``: 1, 2 or 4 per axis.
    ``ring_frames``: the capacity of the ring ``attached()`` and ``frame()`` without ``out`` draw into.  ``palette``: ``u8 [3 + N, 3]`` (``default_palette``).
    ``short_term_path=None`` takes ``Parameters.is_visualize_short_term_path`` when the env carries parameters.  ``h_boundary`` / ``h_path``: half-widths in PIXELS
    (default: 0.01 m at the view's scale, at least half a pixel)."""

    def __init__(self, env, envs=(0,), width: int = 512, height: int | None = None, view=None, samples: int = 2, ring_frames: int = 0, palette=None,
                 short_term_path: bool | None = None, h_boundary: float | None = None, h_path: float | None = None):
        self.env, self.r = env, None
        if view is None:
            scale, x0, y1, height = fit_view(env.map.world_x_dim, env.map.world_y_dim, width, height)
        else:
            if height is None:
                raise ValueError("render: a view of the caller's needs a height")
            scale, x0, y1 = (float(v) for v in view)
        self.width, self.height, self.samples, self.ring_frames = int(width), int(height), int(samples), int(ring_frames)
        self.selection = check_image(self.width, self.height, self.samples, envs, env.B)
        self.view = (scale, x0, y1)
        if short_term_path is None:
            short_term_path = bool(getattr(env.parameters, "is_visualize_short_term_path", False)) if getattr(env, "parameters", None) is not None else False
        self.short_term_path = bool(short_term_path)
        self.palette = np.ascontiguousarray(default_palette(env.N) if palette is None else np.asarray(palette, np.uint8))
        if self.palette.shape != (3 + env.N, 3):
            raise ValueError(f"render: the palette must be uint8 [{3 + env.N}, 3]: background, boundary, collision, the agents")
        if self.ring_frames < 0:
            raise ValueError("render: ring_frames >= 0")
        self.h_boundary = float(h_boundary) if h_boundary is not None else max(0.5, H_BOUNDARY_M * scale)
        self.h_path = float(h_path) if h_path is not None else max(0.5, H_PATH_M * scale)
        args = capi.RenderArgs()
        args.scale, args.x0, args.y1, args.h_boundary, args.h_path = scale, x0, y1, self.h_boundary, self.h_path
        args.height, args.width, args.samples = self.height, self.width, self.samples
        args.flags = capi.RENDER_SHORT_TERM if self.short_term_path else 0
        args.n_sel, args.ring_frames = len(self.selection), self.ring_frames
        args.palette = self.palette.ctypes.data
        args.selection = self.selection.ctypes.data
        r = C.c_void_p()
        with torch.cuda.device(env.device):
            env._chk(env.lib.render_create(env.h, C.byref(args), C.byref(r)), "render_create")
        self.r = r
        self._ring = None

    # ---- plumbing ---------------------------------------------------------------------------------------------
    @property
    def shape(self):
        return (len(self.selection), self.height, self.width, 3)

    def _check(self, t, dtype, shape, what):
        if t is None:
            return None
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
            raise TypeError(f"render: {what} must be a contiguous {dtype} CUDA tensor {list(shape)}")
        return t.data_ptr()

    def _get(self):
        ring, frames, drawn, newest = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_int32()
        self.env._chk(self.env.lib.render_get(self.env.h, self.r, C.byref(ring), C.byref(frames), C.byref(drawn), C.byref(newest)), "render_get")
        return ring.value, int(frames.value), int(newest.value), int(drawn.value)

    @property
    def frames(self) -> int:
        """frames drawn so far, as the host counts them (no wait)"""
        return self._get()[1]

    @property
    def newest_slot(self) -> int:
        """the ring slot of the newest ring frame, -1 before the first"""
        return self._get()[2]

    def ring(self) -> torch.Tensor:
        """the ring ``[ring_frames, n_sel, H, W, 3]`` as a zero-copy view, in slot order"""
        if self.ring_frames < 1:
            raise RuntimeError("render: the renderer was created without a ring (ring_frames=0)")
        if self._ring is None:
            from .env import device_view

            self._ring = device_view(self._get()[0], (self.ring_frames,) + self.shape, "u8", self.env.device.index, self)
        return self._ring

    def close(self):
        if getattr(self, "r", None):  # (also after the env was closed: an orphaned renderer can only be destroyed, and its images and ring are freed here)
            self.env.lib.render_destroy(self.r)
        self.r, self._ring = None, None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ---- the calls ----------------------------------------------------------------------------------------------
    def frame(self, out: torch.Tensor | None = None, *, to_ring: bool = False, vertices=None, short_term=None, state=None, col_agents=None, col_flags=None) -> torch.Tensor:
        """One frame of every selected env, one launch: ``uint8 [n_sel, H, W, 3]`` on the device, into ``out`` (or a new tensor; ``to_ring=True``: the next ring slot,
        and the returned tensor is a view of it).  The env's buffers as they stand, or -- per argument -- a tensor of the same layout in their place
        (``vertices [B,N,5,2]``, ``short_term [B,N,NS,2]``, ``state [B,N,8]`` f32; ``col_agents [B,N,N]``, ``col_flags [B,N,4]`` u8), each starting on a 4-byte
        boundary."""
        e = self.env
        src = render_src(self._check(vertices, torch.float32, (e.B, e.N, 5, 2), "vertices"), self._check(short_term, torch.float32, (e.B, e.N, e.n_short_term, 2), "short_term"),
                         self._check(state, torch.float32, (e.B, e.N, 8), "state"), self._check(col_agents, torch.uint8, (e.B, e.N, e.N), "col_agents"),
                         self._check(col_flags, torch.uint8, (e.B, e.N, 4), "col_flags"))
        if to_ring:
            if out is not None:
                raise TypeError("render: out or to_ring, not both")
            ring = self.ring()
            e._chk(e.lib.render_frame(e.h, self.r, C.byref(src) if src is not None else None, None), "render_frame")
            return ring[self.newest_slot]
        if out is None:
            out = torch.empty(self.shape, dtype=torch.uint8, device=e.device)
        if self._check(out, torch.uint8, self.shape, "out") & 15:
            raise ValueError("render: out must be 16-byte aligned")
        e._chk(e.lib.render_frame(e.h, self.r, C.byref(src) if src is not None else None, C.c_void_p(out.data_ptr())), "render_frame")
        return out

    @contextlib.contextmanager
    def attached(self, every: int = 1):
        """While inside, every ``every``-th step of ``Actor.rollout`` on this env (counted from here) goes to the ring, drawn after the step and before its resets
        (``sigmaenv_render_attach``); always detaches."""
        self.env._chk(self.env.lib.render_attach(self.env.h, self.r, int(every)), "render_attach")
        try:
            yield self
        finally:
            self.env._chk(self.env.lib.render_attach(self.env.h, None, 0), "render_attach")

    def video(self) -> torch.Tensor:
        """The ring's frames in time order ``[n, n_sel, H, W, 3]``, ``n = min(ring frames drawn, ring_frames)``: a view of the ring where it has not wrapped (or
        wrapped onto slot 0), a copy otherwise."""
        ring = self.ring()
        _, _, newest, drawn = self._get()
        if newest < 0:
            return ring[:0]
        if drawn <= self.ring_frames or newest == self.ring_frames - 1:
            return ring[: min(drawn, self.ring_frames)]
        return torch.cat([ring[newest + 1:], ring[: newest + 1]])

    def save(self, path: str, frames: torch.Tensor | None = None, duration_ms: int = 100):
        """Writes ``frames`` (default: ``video()``) to ``path``: ``.npy`` always (``[n, n_sel, H, W, 3]`` uint8); ``.gif`` (the selected envs side by side, one image
        per frame) and ``.png`` (the newest frame) through PIL only if PIL imports.  Waits for the device."""
        v = (self.video() if frames is None else frames).cpu().numpy()
        if path.endswith(".npy"):
            np.save(path, v)
            return path
        if not (path.endswith(".gif") or path.endswith(".png")):
            raise ValueError("render: save() writes .npy, .gif or .png")
        try:
            from PIL import Image
        except ImportError as err:
            raise RuntimeError("render: writing .gif / .png needs PIL (Pillow), which does not import here; save(.npy) needs nothing") from err
        if len(v) == 0:
            raise ValueError("render: no frame to save")
        images = [Image.fromarray(np.concatenate(list(f), axis=1)) for f in v]
        if path.endswith(".png"):
            images[-1].save(path)
        else:
            images[0].save(path, save_all=True, append_images=images[1:], duration=int(duration_ms), loop=0)
        return path
