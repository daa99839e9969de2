"""Synthetic map tables and query states for the lane-boundary scan beyond what the shipped maps reach (host only, numpy only).

`table(name)` returns a dict with the keys of `sigmarl_amd.mapc.compile_scenario` (pass it as `MapTable(name, table=...)`); `states(name)` returns the query
states placed on it by a fixed rule, and `teleported(name)` the states the far-teleport reset moves the same agents to.  Everything is deterministic: analytic
curves, index rules and one `default_rng(SEED)` for the jitter.

  long257  S-curve paths at 0.05 m spacing: path 0 with 257 centre points (64 chunks of SIGMAENV_CHUNK = 4 segments: the last one the pruned scan's 64-bit masks
           hold) and 255 / 250 boundary points, path 1 with 5 / 5 / 6 points (1 .. 2 chunks: fewer than the CBF kernel's first set of four), path 2 with 130.
  long258  the same with 258 centre points on path 0: 65 chunks, the full scan.
  dense    nearly straight polylines at 0.012 .. 0.015 m spacing (200 / 257 / 230 points): up to 20 boundary segments within the rectangle's circumradius (NEAR_CAP = 8).
  hairpin  257 points out, round a U-turn of radius 0.15 m and back 0.3 m beside itself (chunk c and chunk 63 - c are spatial neighbours), plus one closed path
           (is_loop = 1, first point == last point).
  origin   a straight path through (0, 0) with one 5e-10 m segment on the centre line and on the left boundary: squared length 2.5e-19 < 2^-60.
"""
import numpy as np

f32 = np.float32
SEED = 20240611
LANE_HALF = 0.1                                   # lane width 0.2: the default vehicle (0.22 x 0.107) fits with 0.0465 m to spare on either side
LENGTH, WIDTH = 0.22, 0.107                       # capi.AGENTS (the default vehicle)
_lh, _wh = f32(LENGTH / 2), f32(WIDTH / 2)
RECT_RADIUS = float(np.sqrt(f32(f32(_lh * _lh) + f32(_wh * _wh))) * f32(1.00001) + f32(1e-5))  # the library's float32 circumradius (sigmaenv_create: rect_radius)
NEAR_RADIUS = float(f32(RECT_RADIUS) + f32(1e-4))  # a boundary segment within it goes on the near list (scan_tile_balanced: near_thr)
NAMES = ("long257", "long258", "dense", "hairpin", "origin")
N_STATES = 96                                     # per map: 6 envs of 16 agents, 24 of 4; the first 72 / 24 fill 24 envs of 3 / 1


# ---- curves: arc length -> (point, unit tangent), float64 -------------------------------------------------------------------------------------------
def _s_curve(length, y0, amp=0.5):
    def c(s):
        x = s
        y = y0 + amp * np.sin(2 * np.pi * s / length)
        dy = amp * 2 * np.pi / length * np.cos(2 * np.pi * s / length)
        t = np.stack([np.ones_like(s), dy], -1)
        return np.stack([x, y], -1), t / np.linalg.norm(t, axis=-1, keepdims=True)
    return c


def _hairpin(leg, radius, x0=0.5, y0=0.5):
    arc = np.pi * radius

    def c(s):
        s = np.asarray(s, np.float64)
        out, back = s < leg, s >= leg + arc
        a = np.clip((s - leg) / radius, 0.0, np.pi)
        p = np.where(out[..., None], np.stack([x0 + s, np.full_like(s, y0)], -1),
                     np.where(back[..., None], np.stack([x0 + leg - (s - leg - arc), np.full_like(s, y0 + 2 * radius)], -1),
                              np.stack([x0 + leg + radius * np.sin(a), y0 + radius - radius * np.cos(a)], -1)))
        t = np.where(out[..., None], np.stack([np.ones_like(s), np.zeros_like(s)], -1),
                     np.where(back[..., None], np.stack([-np.ones_like(s), np.zeros_like(s)], -1), np.stack([np.cos(a), np.sin(a)], -1)))
        return p, t
    return c


def _circle(radius, cx, cy):
    def c(s):
        a = np.asarray(s, np.float64) / radius
        return np.stack([cx + radius * np.cos(a), cy + radius * np.sin(a)], -1), np.stack([-np.sin(a), np.cos(a)], -1)
    return c


def _sample(curve, length, n, offset):
    """n points at equal arc-length steps of the curve displaced by `offset` along its left normal."""
    p, t = curve(np.linspace(0.0, length, n))
    return (p + offset * np.stack([-t[:, 1], t[:, 0]], -1)).astype(f32)


def _path(curve, length, n_center, n_left, n_right, is_loop=False):
    center = _sample(curve, length, n_center, 0.0)
    left, right = _sample(curve, length, n_left, LANE_HALF), _sample(curve, length, n_right, -LANE_HALF)
    if is_loop:  # closed: the last point IS the first one, bit for bit
        center[-1], left[-1], right[-1] = center[0], left[0], right[0]
    return {"center": center, "left": left, "right": right, "is_loop": is_loop, "curve": curve, "length": length}


def _yaw(center):
    v = np.diff(center, axis=0).astype(f32)
    return np.arctan2(v[:, 1].astype(np.float64), v[:, 0].astype(np.float64)).astype(f32)


def _pack(paths):
    n = len(paths)
    mc, ml, mr = (max(len(p[k]) for p in paths) for k in ("center", "left", "right"))
    out = {"center": np.zeros((n, mc, 2), f32), "yaw": np.zeros((n, mc), f32), "left": np.zeros((n, ml, 2), f32), "right": np.zeros((n, mr, 2), f32),
           "n_center": np.zeros(n, np.int32), "n_yaw": np.zeros(n, np.int32), "n_left": np.zeros(n, np.int32), "n_right": np.zeros(n, np.int32),
           "is_loop": np.zeros(n, np.uint8), "lanelet_ids": np.arange(n, dtype=np.int32)[:, None].copy(), "n_lanelet_ids": np.ones(n, np.int32),
           "list_id": np.zeros(n, np.int32), "local_id": np.arange(n, dtype=np.int32)}
    for i, p in enumerate(paths):
        c, l, r, y = p["center"], p["left"], p["right"], _yaw(p["center"])
        out["n_center"][i], out["n_left"][i], out["n_right"][i], out["n_yaw"][i] = len(c), len(l), len(r), len(y)
        out["center"][i, :len(c)], out["left"][i, :len(l)], out["right"][i, :len(r)], out["yaw"][i, :len(y)] = c, l, r, y
        out["is_loop"][i] = p["is_loop"]
    allp = np.concatenate([p[k] for p in paths for k in ("center", "left", "right")]).astype(np.float64)
    out["world_x_dim"] = np.float64(allp[:, 0].max() + allp[:, 0].min())
    out["world_y_dim"] = np.float64(allp[:, 1].max() + allp[:, 1].min())
    out["parser_lane_width"] = np.float64(2 * LANE_HALF)
    out["lane_width"] = np.float64(2 * LANE_HALF)
    return out


def _long(n_longest):
    length = 0.05 * (n_longest - 1)
    return [_path(_s_curve(length, 1.0), length, n_longest, 255, 250),
            _path(_s_curve(0.2, 3.0, amp=0.01), 0.2, 5, 5, 6),
            _path(_s_curve(6.45, 5.0), 6.45, 130, 128, 131)]


def _origin():
    p = _path(lambda s: (np.stack([s - 3.0, np.zeros_like(s)], -1), np.stack([np.ones_like(s), np.zeros_like(s)], -1)), 6.0, 121, 121, 97)
    for key, y in (("center", 0.0), ("left", LANE_HALF)):  # one 5e-10 m segment right after x = 0 (point 60 of 121 lies on x = 0 exactly)
        a = p[key]
        assert a[60, 0] == 0.0
        p[key] = np.concatenate([a[:61], np.array([[5e-10, y]], f32), a[61:]]).astype(f32)
    return [p]


_paths_cache = {}


def paths(name):
    if name not in _paths_cache:
        if name in ("long257", "long258"):
            ps = _long(int(name[4:]))
        elif name == "dense":
            ps = [_path(_s_curve(0.015 * 199, 1.0, amp=0.02), 0.015 * 199, 200, 257, 230)]
        elif name == "hairpin":
            ps = [_path(_hairpin((12.8 - np.pi * 0.15) / 2, 0.15), 12.8, 257, 257, 251),
                  _path(_circle(0.6, 3.0, 3.0), 2 * np.pi * 0.6, 100, 98, 101, is_loop=True)]
        elif name == "origin":
            ps = _origin()
        else:
            raise KeyError(name)
        _paths_cache[name] = ps
    return _paths_cache[name]


def table(name):
    return _pack(paths(name))


def duplicate_point_table():
    """`origin` with the 5e-10 m segment collapsed to an exact duplicate of its first point: the reference divides 0 by 0 there and stops at its own assertion
    (helper_scenario.py:862-881), so the package refuses such a table (tests/test_scan_synthetic_host.py)."""
    t = table("origin")
    t["center"][0, 61] = t["center"][0, 60]
    return t


# ---- query states ---------------------------------------------------------------------------------------------------------------------------------
def _pose(curve, s, lateral, dyaw=0.0):
    p, t = curve(np.asarray([s], np.float64))
    p, t = p[0], t[0]
    q = p + lateral * np.array([-t[1], t[0]])
    return float(q[0]), float(q[1]), float(np.arctan2(t[1], t[0]) + dyaw)


def _count_within(poly, x, y, radius):
    """Segments of the float32 polyline within `radius` of (x, y), float64."""
    a, b = poly[:-1].astype(np.float64), poly[1:].astype(np.float64)
    ab = b - a
    t = np.clip(((np.array([x, y]) - a) * ab).sum(-1) / np.maximum((ab * ab).sum(-1), 1e-300), 0.0, 1.0)
    return int((np.linalg.norm(a + ab * t[:, None] - np.array([x, y]), axis=-1) <= radius).sum())


def _lateral_with_count(p, side, s, want, at_least=False):
    """The smallest lateral offset towards boundary `side` (a 0.1 mm grid) at which exactly (at least) `want` of its segments lie within the circumradius."""
    poly, sign = (p["left"], 1.0) if side == 0 else (p["right"], -1.0)
    for d in np.arange(0.0, LANE_HALF + RECT_RADIUS, 1e-4):
        x, y, _ = _pose(p["curve"], s, sign * d)
        x, y = float(f32(x)), float(f32(y))  # (the position the environments get is float32)
        n = _count_within(poly, x, y, NEAR_RADIUS)
        clear = n == _count_within(poly, x, y, NEAR_RADIUS - 2e-6) == _count_within(poly, x, y, NEAR_RADIUS + 2e-6)  # no segment within float32 rounding of the radius
        if clear and ((n >= want) if at_least else (n == want)):
            return sign * d
    raise AssertionError((side, s, want))


def _build_states(name):
    """[N_STATES] rows (path, point id, x, y, yaw, speed) and the rows the same agents are teleported to.  Categories by i % 8:
    0 on the lane (spread over the whole path; every other one within the last 0.2 m of path 0: its last chunks), 1 / 2 astride the left / right boundary, 3 at a polyline vertex or
    on the bisector of two segments (ties), 4 far off the map (2 m and 50 m), 5 on the lane with a yaw and lateral jitter, 6 map-specific (dense: exactly 8, exactly 9
    and >= 12 near segments; others: the end of the path), 7 on the other paths of the map."""
    ps = paths(name)
    rng = np.random.default_rng(SEED + NAMES.index(name))
    rows, tele = [], []
    p0 = ps[0]
    L0 = p0["length"]

    def add(pi, s, lateral, dyaw=0.0, xy=None, s_tele=None):
        p = ps[pi]
        x, y, yaw = _pose(p["curve"], s, lateral, dyaw)
        if xy is not None:
            x, y = xy
        n = len(p["center"])
        pt = int(np.clip(round(s / p["length"] * (n - 1)), 1, n - 2))
        rows.append((pi, pt, x, y, yaw, float(rng.uniform(0.1, 0.8))))
        # the far teleport: to the mirrored arc length of the same path (hairpin: the other leg, 0.3 m beside; elsewhere: the other end), on the lane
        st = p["length"] - s if s_tele is None else s_tele
        st = float(np.clip(st, 0.02 * p["length"], 0.98 * p["length"]))
        xt, yt, yawt = _pose(p["curve"], st, float(rng.uniform(-0.02, 0.02)))
        tele.append((pi, pt, xt, yt, yawt, 0.0))  # (the point id stays: what the agent knew before)

    for i in range(N_STATES):
        cat, k = i % 8, i // 8  # k = 0 .. 11
        if cat == 0:
            s = L0 - 0.02 - 0.035 * (k // 2) if k % 2 else L0 * (0.02 + 0.96 * k / 11)
            add(0, s, float(rng.uniform(-0.03, 0.03)))
        elif cat in (1, 2):
            side = 1.0 if cat == 1 else -1.0
            s = L0 - 0.02 - 0.035 * (k // 2) if k % 2 else L0 * (0.03 + 0.9 * k / 11)
            add(0, s, side * (LANE_HALF + float(rng.uniform(-0.04, 0.04))), dyaw=float(rng.uniform(-0.6, 0.6)))
        elif cat == 3:
            key = ("center", "left", "right")[k % 3]
            poly = p0[key]
            j = [1, len(poly) // 3, len(poly) - 2, len(poly) // 2][k % 4]
            lat = {"center": 0.0, "left": LANE_HALF, "right": -LANE_HALF}[key]
            v = poly[j].astype(np.float64)
            if k < 4:       # exactly at the vertex: both adjoining segments at distance 0
                xy = (float(v[0]), float(v[1]))
            elif k < 8:     # within a micrometre of it
                xy = (float(v[0]) + float(rng.uniform(-1e-6, 1e-6)), float(v[1]) + float(rng.uniform(-1e-6, 1e-6)))
            else:           # on the bisector of the two segments that meet there, 3 cm to the outside of the bend (or either side of a straight line)
                u0 = (poly[j] - poly[j - 1]).astype(np.float64)
                u1 = (poly[j + 1] - poly[j]).astype(np.float64)
                u0, u1 = u0 / np.linalg.norm(u0), u1 / np.linalg.norm(u1)
                b = u0 - u1
                b = b / np.linalg.norm(b) if np.linalg.norm(b) > 1e-9 else np.array([-u0[1], u0[0]])
                xy = (float(v[0] + 0.03 * b[0]), float(v[1] + 0.03 * b[1]))
            add(0, L0 * j / (len(poly) - 1), lat, xy=xy)
        elif cat == 4:
            off = (2.0, 50.0)[k % 2] * (1.0 if k % 4 < 2 else -1.0)
            add(0, L0 * (0.05 + 0.9 * k / 11), off, dyaw=float(rng.uniform(-3.0, 3.0)))
        elif cat == 5:
            add(0, L0 * float(rng.uniform(0.01, 0.99)), float(rng.uniform(-0.045, 0.045)), dyaw=float(rng.uniform(-0.3, 0.3)))
        elif cat == 6:
            if name == "dense":
                s = L0 * (0.2 + 0.05 * k) + 0.0037  # (off the vertices: at a vertex the count grows two at a time)
                want, at_least = ((8, False), (9, False), (12, True))[k % 3]
                add(0, s, _lateral_with_count(p0, (k // 3) % 2, s, want, at_least))
            else:
                add(0, L0 * (0.9 + 0.1 * k / 11), float(rng.uniform(-0.16, 0.16)), dyaw=float(rng.uniform(-0.2, 0.2)))
        else:
            pi = 1 + k % (len(ps) - 1) if len(ps) > 1 else 0
            p = ps[pi]
            lat = (0.0, LANE_HALF + 0.01, -LANE_HALF - 0.01, 0.02)[k % 4]
            add(pi, p["length"] * (0.04 + 0.92 * ((k * 5) % 12) / 11), lat, dyaw=float(rng.uniform(-0.4, 0.4)))
    return np.asarray(rows, np.float64), np.asarray(tele, np.float64)


_states_cache = {}


def _cached(name):
    if name not in _states_cache:
        _states_cache[name] = _build_states(name)
    return _states_cache[name]


def states(name):
    """float64 [N_STATES, 6]: path, centre-line point id, x, y, yaw, speed."""
    return _cached(name)[0].copy()


def teleported(name):
    return _cached(name)[1].copy()


def state8(rows):
    """The eight-float agent state of `SigmaEnv.reset` (x, y, yaw, speed, steering, vx, vy, sideslip) of state rows."""
    x, y, yaw, sp = (rows[:, c].astype(f32) for c in (2, 3, 4, 5))
    z = np.zeros_like(x)
    return np.stack([x, y, yaw, sp, z, sp * np.cos(yaw).astype(f32), sp * np.sin(yaw).astype(f32), z], -1).astype(f32)


def vertices(rows):
    """The rectangle's corners, closed (5 points: front-right, front-left, rear-left, rear-right, front-right as the reference orders them), float32: the
    query points of the golden.  (The environments compute their own; these are data for the polyline functions.)"""
    x, y, yaw = rows[:, 2].astype(f32).astype(np.float64), rows[:, 3].astype(f32).astype(np.float64), rows[:, 4].astype(f32).astype(np.float64)
    c, s = np.cos(yaw), np.sin(yaw)
    out = np.zeros((len(rows), 5, 2), f32)
    for q, (lx, ly) in enumerate(((LENGTH / 2, WIDTH / 2), (LENGTH / 2, -WIDTH / 2), (-LENGTH / 2, -WIDTH / 2), (-LENGTH / 2, WIDTH / 2), (LENGTH / 2, WIDTH / 2))):
        out[:, q, 0] = (x + c * lx - s * ly).astype(f32)
        out[:, q, 1] = (y + s * lx + c * ly).astype(f32)
    return out
