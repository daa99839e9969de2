"""Frames drawn on the device (sigmaenv_render_*, ``sigmarl_amd.render``) held to tests/render_check.py.

1. planted frames through ``frame(overrides)`` equal the twin AS BYTES, every pixel, on the smallest shapes that can go wrong (``render_check.cases``): N = 1, one
   env, 64 x 64, S = 1; N = 4, B = 5 with the selection [4, 0, 2, 0]; 72 x 100 (W a multiple of 4 only, partial tiles on both edges); a vehicle across a tile corner,
   one across the image's edge, one wholly outside; a zero-area quad, a NaN vertex, an infinite path point, coordinates that overflow (nothing drawn, nothing
   faults: the box arithmetic never converts them, tests/test_render_check.py runs the same header under the host sanitizers); 64 vehicles in one tile, past the
   list's capacity; S = 2 and 4; a collision byte; the short-term flag off; and a frame in which nothing is drawn equals the background in every tile.
2. ``Actor.rollout`` with a renderer attached (4 agents x 6 envs, 12 steps, every = 3, ring of 3) leaves what the detached rollout leaves, bit for bit; the ring holds
   steps 3, 6, 9 and wraps at 12; each ring frame equals ``frame()`` in a step-by-step replay at that step BEFORE its resets -- alone, and with an evaluator and an
   initial-state bank attached beside it, whose results do not change.
3. ``evaluate(render=)`` gives the same metrics; ``save`` round-trips through ``.npy`` (and writes a GIF where PIL imports).
4. the refusals on the device path."""
import ctypes as C

import numpy as np
import pytest

import render_check as rc

pytestmark = pytest.mark.gpu

LOW, HIGH = [-1.0, -0.6], [1.0, 0.6]
KW = dict(scenario_type="intersection_1", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False)


def _env(N, B, **kw):
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters

    p = dict(KW, n_agents=N)
    p.update(kw)
    return SigmaEnv(Parameters(**p), n_envs=B, device="cuda:0")


def _bits(t):
    import torch

    return t.contiguous().view(torch.uint8)


# ---- 1. planted frames ---------------------------------------------------------------------------------------------------------------------------
SHAPES = {name: (c["N"], c["B"]) for name, c in rc.cases().items()}


@pytest.mark.parametrize("name", list(SHAPES))
def test_planted_frames_equal_the_twin_as_bytes(name):
    import torch
    from sigmarl_amd.render import Renderer

    N, B = SHAPES[name]
    env = _env(N, B, **(dict(scenario_type="cpm_entire") if N > 16 else {}))  # lends its handle and its map: its own buffers are never read
    c = rc.cases(dict(left=env.map.left, right=env.map.right, n_left=env.map.n_left, n_right=env.map.n_right))[name]
    tw = rc.twin(c)
    r = Renderer(env, envs=c["sel"], width=c["W"], height=c["H"], view=c["view"], samples=c["S"], ring_frames=2, palette=c["palette"], short_term_path=bool(c["flags"] & 1),
                 h_boundary=float(c["h_b"]), h_path=float(c["h_p"]))
    keys = ("vertices", "short_term", "state", "col_agents", "col_flags")
    dev = {k: torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in keys}
    got = r.frame(**dev)
    assert got.shape == (len(c["sel"]), c["H"], c["W"], 3) and got.dtype == torch.uint8
    diff = int((got.cpu().numpy() != tw["frames"]).sum())
    print(name, "bytes that differ:", diff, "tile lists:", sorted(set(rc.tile_lists(c, int(c["sel"][0])).values()))[-3:])
    assert rc.same_bytes(got.cpu().numpy(), tw["frames"]), diff
    # the float64 bracket on the DEVICE's own pixels, directly: the colours of layers 2 and 3 lie above the map, so their counts hold over the env's map too
    direct = rc.check(got.cpu().numpy(), c)
    if c.get("bracket"):
        print(name, "device bracket (count, lo, hi):", rc.bracket(got.cpu().numpy(), c))
    assert all(direct.values()) and (bool(direct) == (name in ("one_agent", "bracket"))), direct
    # again into the ring, and into a caller's tensor filled with something else first: the same bytes
    again = r.frame(to_ring=True, **dev)
    out = torch.full_like(got, 7)
    assert r.frame(out, **dev) is out
    assert torch.equal(again, got) and torch.equal(out, got) and r.frames == 3 and r.newest_slot == 0
    # nothing drawn: every tile's list is empty and the frame is the background, byte for byte
    nothing = {k: torch.from_numpy(v).cuda() for k, v in rc.empty_inputs(N, B).items()}
    bg = r.frame(**nothing).cpu().numpy()
    assert all(rc.same_bytes(bg[k], tw["bg_rgb"]) for k in range(len(c["sel"])))
    for x in (r, env):
        x.close()


# ---- 2. attached -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beside", [False, True], ids=["alone", "beside_evaluator_and_bank"])
def test_attached_rollout_equals_the_detached_one_and_its_ring_the_replay(beside):
    import torch
    from sigmarl_amd.actor import Actor, make_mlp
    from sigmarl_amd.env import _buf_layout
    from sigmarl_amd.evaluate import Evaluator
    from sigmarl_amd.initial_states import InitialStateBank
    from sigmarl_amd.render import Renderer

    N, B, T, every, seed, counter0 = 4, 6, 12, 3, 5, 40
    envs = [_env(N, B, is_testing_mode=True) for _ in range(3)]  # detached, attached, replayed step by step
    for e in envs:
        e.reset_random(seed=3)
    torch.manual_seed(1)
    mlp = make_mlp(envs[0].D)
    with torch.no_grad():
        for m in mlp:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(1.7)
                m.bias.uniform_(-0.3, 0.3)
    actor = Actor(mlp, low=LOW, high=HIGH)
    W, D = N * (envs[0].D + 1) + 1, envs[0].D
    rec = [dict(slab=torch.zeros(T, B, W, device="cuda"), log_prob=torch.zeros(T, B, N, device="cuda"), actions=torch.zeros(T, B, N, 2, device="cuda"),
                obs_rec=torch.zeros(T, B, N, D, device="cuda")) for _ in range(2)]
    evs = [Evaluator(e) for e in envs] if beside else [None] * 3
    banks = [InitialStateBank(e, capacity=3, n_steps_stored=3, probability_use_recording=0.5) for e in envs] if beside else [None] * 3
    for bk in banks:
        if bk is not None:
            bk.load(bk.env.state[:2].clone(), bk.env.buffer(3)[:2].clone())  # (3: capi.BUF_PATH) two scenes to restart from
    rs = [Renderer(e, envs=(5, 0, 3), width=64, samples=2, ring_frames=3, short_term_path=True) for e in envs[1:]]

    def rollouts(env, records, ev, bank, renderer):
        """9 steps, then 3 more, inside ONE attachment; returns the ring as it stood after the first part"""
        import contextlib

        with contextlib.ExitStack() as st:
            for x in (ev, bank):
                if x is not None:
                    st.enter_context(x.attached())
            if renderer is not None:
                st.enter_context(renderer.attached(every))
            first = {k: v[:9] for k, v in records.items()}
            actor.rollout(env, 9, seed=seed, counter0=counter0, **first)
            mid = None
            if renderer is not None:
                assert renderer.frames == 3 and renderer.newest_slot == 2
                v = renderer.video()
                assert v.data_ptr() == renderer.ring().data_ptr() and v.shape[0] == 3  # not wrapped: a view
                mid = v.clone()
            actor.rollout(env, 3, seed=seed, counter0=counter0 + 9, **{k: v[9:] for k, v in records.items()})
        return mid

    rollouts(envs[0], rec[0], evs[0], banks[0], None)
    mid = rollouts(envs[1], rec[1], evs[1], banks[1], rs[0])
    envs[0].sync()
    envs[1].sync()
    for k in rec[0]:
        assert torch.equal(_bits(rec[0][k]), _bits(rec[1][k])), k
    for which in _buf_layout(B, N, envs[0].K, D):
        assert torch.equal(_bits(envs[0].buffer(which)), _bits(envs[1].buffer(which))), which
    assert rs[0].frames == 4 and rs[0].newest_slot == 0  # step 12 wrapped onto slot 0
    video = rs[0].video()
    assert video.shape == (3, 3, rs[0].height, 64, 3) and torch.equal(video[2], rs[0].ring()[0]) and torch.equal(video[0], rs[0].ring()[1])
    actor.rollout(envs[1], 1, seed=seed, counter0=counter0 + T)  # detached again: the next rollout draws nothing
    assert rs[0].frames == 4
    # the replay: the same actions step by step, a frame after every third step and BEFORE its resets
    hand = []
    for t in range(T):
        envs[2].step(rec[1]["actions"][t].contiguous())
        if beside:
            evs[2].accumulate()
        if (t + 1) % every == 0:
            hand.append(rs[1].frame())
        if beside:
            banks[2].record(seed, counter0 + t)
            banks[2].restart(seed, counter0 + t)
        envs[2].auto_reset(seed=seed, counter=counter0 + t)
        if beside:
            banks[2].settle()
    assert len(hand) == 4
    for k in range(3):
        assert torch.equal(mid[k], hand[k]), ("steps 3, 6, 9", k)
        assert torch.equal(video[k], hand[k + 1]), ("steps 6, 9, 12", k)
    assert not torch.equal(hand[0], hand[1]) and not torch.equal(hand[1], hand[2])  # the vehicles move: the frames differ
    assert (hand[0] != torch.tensor(rs[1].palette[0], device="cuda")).any()  # something is drawn
    if beside:
        a, d = evs[1].accumulators(), evs[0].accumulators()
        assert all(rc.same_bytes(a[k], d[k]) for k in a) and evs[1].frames == T
        assert torch.equal(_bits(evs[1].finish()["metrics"]), _bits(evs[0].finish()["metrics"]))
        assert torch.equal(_bits(evs[1].finish()["metrics"]), _bits(evs[2].finish()["metrics"]))
    for x in (*rs, *[x for x in (*evs, *banks) if x is not None], actor, *envs):
        x.close()


# ---- 3. evaluate(render=) and save -----------------------------------------------------------------------------------------------------------------------
def _evaluated(tmp_path):
    import torch
    from sigmarl_amd.actor import Actor, make_mlp
    from sigmarl_amd.evaluate import evaluate
    from sigmarl_amd.render import Renderer

    env = _env(4, 3, is_testing_mode=True, max_steps=9)
    torch.manual_seed(2)
    actor = Actor(make_mlp(env.D), low=LOW, high=HIGH)
    plain = evaluate(env, actor, seed=7)
    r = Renderer(env, envs=(2, 0), width=64, samples=1, ring_frames=4)
    drawn = evaluate(env, actor, seed=7, render=r, render_every=2)
    return env, actor, r, plain, drawn


def test_evaluate_with_a_renderer_gives_the_same_metrics_and_save_round_trips(tmp_path):
    import torch

    env, actor, r, plain, drawn = _evaluated(tmp_path)
    assert plain["frames"] == drawn["frames"] == 8
    for k in ("metrics", "counts"):
        assert torch.equal(_bits(plain[k]), _bits(drawn[k])), k
    assert r.frames == 3  # 7 steps, every second one
    video = r.video()
    assert video.shape == (3, 2, r.height, 64, 3)
    path = r.save(str(tmp_path / "rollout.npy"))
    assert rc.same_bytes(np.load(path), video.cpu().numpy())
    with pytest.raises(ValueError, match="npy"):
        r.save(str(tmp_path / "rollout.mp4"))
    for x in (r, actor, env):
        x.close()


def test_save_writes_a_gif_where_pil_imports(tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image

    env, actor, r, _, _ = _evaluated(tmp_path)
    path = r.save(str(tmp_path / "rollout.gif"))
    with Image.open(path) as im:
        assert im.size == (2 * 64, r.height) and getattr(im, "n_frames", 1) == 3
    for x in (r, actor, env):
        x.close()


# ---- 4. refusals on the device path ---------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device_path():
    import torch
    from sigmarl_amd import capi
    from sigmarl_amd.render import Renderer, default_palette

    env, other = _env(4, 3), _env(4, 3)
    lib = env.lib
    pal, sel = default_palette(4), np.asarray([2, 0], np.int32)

    def args(**kw):
        a = capi.RenderArgs()
        a.scale, a.x0, a.y1, a.h_boundary, a.h_path = 16.0, 0.0, 4.0, 1.0, 1.0
        a.height, a.width, a.samples, a.flags, a.n_sel, a.ring_frames = 64, 64, 2, 1, 2, 0
        a.palette, a.selection = pal.ctypes.data, sel.ctypes.data
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    out = C.c_void_p()
    bad_sel = np.asarray([0, 3], np.int32)
    for kw, msg in ((dict(width=66), b"multiple of 4"), (dict(samples=3), b"1, 2 or 4"), (dict(selection=bad_sel.ctypes.data), b"outside [0, n_envs)"),
                    (dict(scale=float("nan")), b"finite"), (dict(flags=2), b"flags"), (dict(palette=None), b"required")):
        assert lib.render_create(env.h, C.byref(args(**kw)), C.byref(out)) == -22 and msg in lib.last_error(env.h) and not out.value, kw
    for kw in (dict(width=66), dict(samples=8), dict(envs=(3,))):
        with pytest.raises(ValueError):
            Renderer(env, **dict(dict(width=64), **kw))
    r = Renderer(env, envs=(2, 0), width=64)
    frame = torch.empty(r.shape, dtype=torch.uint8, device="cuda")
    for call in (lambda: lib.render_frame(other.h, r.r, None, C.c_void_p(frame.data_ptr())), lambda: lib.render_attach(other.h, r.r, 1),
                 lambda: lib.render_get(other.h, r.r, None, None, None, None)):
        assert call() == -22 and b"another handle" in lib.last_error(other.h)
    assert lib.render_frame(None, r.r, None, None) == -22 and lib.render_frame(env.h, None, None, None) == -22 and b"null renderer" in lib.last_error(env.h)
    src = capi.RenderSrc()
    src.state = env.state.data_ptr() + 2
    assert lib.render_frame(env.h, r.r, C.byref(src), C.c_void_p(frame.data_ptr())) == -22 and b"4-byte aligned" in lib.last_error(env.h)
    assert lib.render_frame(env.h, r.r, None, C.c_void_p(frame.data_ptr() + 4)) == -22 and b"16-byte aligned" in lib.last_error(env.h)
    assert lib.render_frame(env.h, r.r, None, None) == -22 and b"without a ring" in lib.last_error(env.h)
    assert lib.render_attach(env.h, r.r, 1) == -22 and b"without a ring" in lib.last_error(env.h)
    with pytest.raises(ValueError, match="4-byte aligned"):
        r.frame(col_flags=torch.zeros(3 * 4 * 4 + 1, dtype=torch.uint8, device="cuda")[1:].view(3, 4, 4))
    with pytest.raises(TypeError, match="vertices"):
        r.frame(vertices=torch.zeros(3, 4, 4, 2, device="cuda"))
    assert r.frames == 0
    ring = Renderer(env, envs=(1,), width=64, ring_frames=2)
    assert lib.render_attach(env.h, ring.r, 0) == -22 and b"every" in lib.last_error(env.h)
    env.sync()
    for x in (ring, r, env, other):
        x.close()
