"""Phase E of the step kernel on its tile-wide list of near boundary segments (run with -m gpu on an MI355X).

The scan appends every boundary segment within the rectangle's circumradius to ONE list per tile (capacity: slots of a full tile x NEAR_CAP = 8 entries) and phase E
tests one (entry, rectangle edge) per lane; a tile whose total exceeds the capacity walks every segment of the boundaries that counted one.  Here the total of a tile
is put below, exactly at, one above the capacity -- and, for the single-agent tile (capacity 8), far above it from one side of the one agent -- at 16 x 1, 4 x 4,
3 x 5 (generic) and 1 x 1 (generic) on the `dense` map of tests/synthetic_maps.py, and the CPM map runs at the same shapes with states beside its boundaries.

Every state stands still (speed 0) and the first step commands speed 0: the scan of that step sees the placed positions.  The count of a state is taken in float64
from the map's polylines and the position the ORACLE holds after the reset -- never from the device -- and asserted before the step, together with a clearance: no
segment lies within 1e-3 m of the threshold, so no count hinges on a rounding.  The crossings are predicted on the host per rectangle edge as well (and held against
the oracle's flag after the step): on the dense map every tile has a crossing that only edges other than edge 0 of an agent other than slot 0 find (rotated agents;
the single-agent tile: edges other than edge 0), and slot 0 has entries but no crossing -- an entry decoded to the wrong slot or edge changes a flag.

After the step: an eight-step step_autoreset_n launch with re-placements from the start table (max_steps = 5), against eight single launches of a second handle
byte for byte and against the oracle as tests/test_gpu_scan_synthetic.py compares (masks, col_flags, done, timers bit for bit; distances, short-term path and
rewards bit for bit).  At 16 x 1 a third handle runs the full scan (SIGMAENV_PRUNE=0) and must give the same bytes."""
import functools

import numpy as np
import pytest

import oracle_binding as ob
import synthetic_maps as sm
import test_gpu_parity as tp
import test_gpu_scan_synthetic as tgs
from sigmarl_amd import capi
from sigmarl_amd.maps import load_map
from sigmarl_amd.params import Parameters, make_config

pytestmark = pytest.mark.gpu

NEAR_CAP = 8        # sigmaenv.hip: entries of the tile's list per agent slot of a full tile
CLEAR = 1e-3        # no counted (or uncounted) segment within this of the threshold
MAX_STEPS = 5       # one single step, then the launch of eight: every env runs out of steps inside it
# N -> (envs per wavefront, the step kernel's instantiation <FASTDIV, PAR, SN, SG, VAR, MTVS>)
SHAPES = {16: (1, (True, True, 16, 1, False, False)), 4: (4, (True, True, 4, 4, False, False)), 3: (5, (True, True, 0, 0, False, False)),
          1: (1, (True, True, 0, 0, False, False))}
f32 = np.float32


# ---- host geometry, float64 on the float32 inputs ------------------------------------------------------------------------------------------------------
def _seg_dist(poly, x, y):
    a, b = poly[:-1].astype(np.float64), poly[1:].astype(np.float64)
    ab = b - a
    q = np.array([x, y], np.float64)
    t = np.clip(((q - a) * ab).sum(-1) / np.maximum((ab * ab).sum(-1), 1e-300), 0.0, 1.0)
    return np.linalg.norm(a + ab * t[:, None] - q, axis=-1)


def _count(poly, x, y):
    """(segments within the near threshold, whether none lies within CLEAR of it)."""
    d = _seg_dist(poly, x, y)
    return int((d <= sm.NEAR_RADIUS).sum()), bool((np.abs(d - sm.NEAR_RADIUS) > CLEAR).all())


def _edges_crossing(poly, x, y, yaw):
    """Which of the rectangle's four edges properly cross a segment of the polyline (vertex order of the reference: front-right, front-left, rear-left, rear-right)."""
    v = sm.vertices(np.array([[0, 0, x, y, yaw, 0.0]], np.float64))[0].astype(np.float64)
    a, b = poly[:-1].astype(np.float64), poly[1:].astype(np.float64)

    def side(p, q, r):
        return (q[..., 0] - p[..., 0]) * (r[..., 1] - p[..., 1]) - (q[..., 1] - p[..., 1]) * (r[..., 0] - p[..., 0])
    out = []
    for e in range(4):
        p, q = v[e], v[e + 1]
        out.append(bool(((side(a, b, p) * side(a, b, q) < 0) & (side(p, q, a) * side(p, q, b) < 0)).any()))
    return out


# ---- the dense map: states with a chosen count ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense_state(side, s0, want, at_least, rotated):
    """A pose beyond boundary `side` of the dense map (outside the lane: the other boundary is more than the threshold away) with exactly (at least) `want` of its
    segments within the threshold, CLEAR of any doubt; rotated: turned so that edges 1 .. 3 cross the boundary and edge 0 does not, else no edge crosses."""
    p = sm.paths("dense")[0]
    poly, other, sign = (p["left"], p["right"], 1.0) if side == 0 else (p["right"], p["left"], -1.0)
    for s in s0 + 0.0011 * np.arange(12):
        for d in np.arange(sm.LANE_HALF + 0.03, sm.LANE_HALF + sm.RECT_RADIUS, 1e-4):
            for dyaw in ((1.2, 1.5708, 1.9, -1.2, -1.5708, -1.9) if rotated else (0.0,)):
                x, y, yaw = sm._pose(p["curve"], s, sign * d, dyaw)
                x, y, yaw = float(f32(x)), float(f32(y)), float(f32(yaw))
                n, clear = _count(poly, x, y)
                n_other, clear_other = _count(other, x, y)
                if not (clear and clear_other and n_other == 0 and ((n >= want) if at_least else (n == want))):
                    break  # (the count does not depend on the yaw)
                hits = _edges_crossing(poly, x, y, yaw)
                if (rotated and not hits[0] and any(hits[1:])) or (not rotated and not any(hits)):
                    return x, y, yaw
    raise AssertionError((side, s0, want, rotated))


def _dense_plans(N):
    """Per tile (= case) the (side, count, at_least, rotated) of every slot, None = far off the map (no entry)."""
    G = SHAPES[N][0]
    S = G * N
    cap = S * NEAR_CAP
    if N == 1:  # capacity 8: the map's 8 / 9 / up-to-20 lists, each on one side of the one agent
        return cap, {"below": [(0, 5, False, True)], "at": [(1, 8, False, True)], "above": [(0, 9, False, True)], "oneside": [(1, 12, True, True)]}
    n_full = (cap - NEAR_CAP) // 15  # slots with 15 entries each, then one slot that decides the case
    plans = {}
    for case, last in (("below", cap - 15 * n_full - 1), ("at", cap - 15 * n_full), ("above", cap - 15 * n_full + 1)):
        slots = [None] * S
        for k in range(n_full):
            slots[k] = (k % 2, 15, False, k in (1, 4))   # slot 0 stands straight: entries, no crossing; slots 1 and 4 are turned into the boundary
        slots[S - 1] = (1, last, False, False)            # (the last slot of the tile: in the last env of a multi-env tile)
        plans[case] = slots
    return cap, plans


def _dense_rows(N):
    """(rows [tiles * S] of (path, point, x, y, yaw, speed), per tile: expected total, per-slot crossing prediction)."""
    p = sm.paths("dense")[0]
    cap, plans = _dense_plans(N)
    rows, want_total, want_hit = [], [], []
    n_pts = len(p["center"])
    for case, slots in plans.items():
        tot, hit = 0, []
        for k, spec in enumerate(slots):
            s = p["length"] * (0.12 + 0.76 * k / max(len(slots) - 1, 1))
            if spec is None:
                x, y, yaw = sm._pose(p["curve"], s, 2.0 + 0.4 * k)
                hit.append(False)
            else:
                side, want, at_least, rotated = spec
                x, y, yaw = _dense_state(side, s, want, at_least, rotated)
                tot += want if not at_least else _count(p["left" if side == 0 else "right"], x, y)[0]
                hit.append(rotated)
            rows.append((0, int(np.clip(round(s / p["length"] * (n_pts - 1)), 1, n_pts - 2)), x, y, yaw, 0.0))
        want_total.append(tot)
        want_hit.append(hit)
    return cap, list(plans), np.asarray(rows, np.float64), want_total, want_hit


# ---- the CPM map: states beside its boundaries -----------------------------------------------------------------------------------------------------------
def _cpm_rows(N, mp, tiles=2):
    G = SHAPES[N][0]
    S = G * N
    pf, pc = mp.list_first[0], mp.list_count[0]
    rows = []
    for tile in range(tiles):
        for k in range(S):
            path = (7 * tile + 3 * k) % pc
            gp = pf + path
            n = int(mp.n_center[gp])
            found = None
            for pt in range(8 + 2 * k, n - 3):      # the first point from here on whose pose is CLEAR on both boundaries
                c = mp.center[gp, pt].astype(np.float64)
                yaw0 = float(mp.yaw[gp, min(pt, int(mp.n_yaw[gp]) - 1)])
                lat = 0.0 if k == 0 else (0.035, -0.035, 0.05)[k % 3]
                dyaw = 0.0 if k == 0 else (0.0, 0.9, -0.9, 1.5708)[k % 4]
                x = float(f32(c[0] - lat * np.sin(yaw0)))
                y = float(f32(c[1] + lat * np.cos(yaw0)))
                if _count(mp.left[gp, :mp.n_left[gp]], x, y)[1] and _count(mp.right[gp, :mp.n_right[gp]], x, y)[1]:
                    found = (path, pt, x, y, float(f32(yaw0 + dyaw)), 0.0)
                    break
            assert found is not None, (tile, k)
            rows.append(found)
    return np.asarray(rows, np.float64)


# ---- driver ---------------------------------------------------------------------------------------------------------------------------------------------------
def _placement(mp, N, rows):
    B = len(rows) // N
    ids = np.zeros((len(rows), 4), np.int32)
    ids[:, 0] = mp.list_first[0] + rows[:, 0].astype(np.int32)
    ids[:, 2] = rows[:, 0].astype(np.int32)
    ids[:, 3] = rows[:, 1].astype(np.int32)
    return np.repeat(np.arange(B), N).astype(np.int32), np.tile(np.arange(N), B).astype(np.int32), ids, sm.state8(rows)


def _tile_counts(mp, ora, N, S):
    """Entries per tile and per (slot, side) from the positions and paths the oracle holds; asserts the clearance of every one."""
    st, path = ora.get(capi.BUF_STATE).reshape(-1, 8), ora.get(capi.BUF_PATH).reshape(-1, 4)
    per = np.zeros((len(st), 2), int)
    for i in range(len(st)):
        gp = int(path[i, 0])
        for side, (poly, n) in enumerate(((mp.left, mp.n_left), (mp.right, mp.n_right))):
            per[i, side], clear = _count(poly[gp, :n[gp]], float(st[i, 0]), float(st[i, 1]))
            assert clear, f"slot {i} side {side}: a segment within {CLEAR} m of the threshold"
    return per.reshape(-1, S, 2)


def _run(monkeypatch, name, mp, N, rows, expect):
    """reset with `rows` -> `expect(per-tile counts, oracle)` -> one standing step -> eight-step launch; HIP handles against each other and against the oracle."""
    import torch

    G, inst = SHAPES[N]
    B = len(rows) // N
    p = Parameters(n_agents=N, scenario_type=name, is_use_mtv_distance=False, rew_method="distance", dt=0.05, is_apply_mask=False, is_obs_noise=False,
                   max_steps=MAX_STEPS)
    cfg = make_config(p, mp, B)
    cfg.envs_per_group = G
    many, one, ora = tgs._handle(monkeypatch, cfg, mp), tgs._handle(monkeypatch, cfg, mp), ob.OracleEnv(cfg, mp)
    devs = [many, one] + ([tgs._handle(monkeypatch, cfg, mp, {"SIGMAENV_PRUNE": 0})] if N == 16 else [])
    try:
        ls = many.env.launch_shape()
        assert (ls["wave_G"], ls["wave_wpb"], ls["pruned_scan"]) == (G, 1, 1) and ls["instantiation"] == inst, ls
        if N == 16:
            assert devs[2].env.launch_shape()["pruned_scan"] == 0
        place = _placement(mp, N, rows)
        for e in devs + [ora]:
            e.reset(*place, 1)
            e.observe()
        per = _tile_counts(mp, ora, N, G * N)
        hits = expect(per)
        stand = np.zeros((B, N, 2), np.float32)
        for e in devs + [ora]:
            e.step(stand)
        assert np.array_equal(ora.get(capi.BUF_STATE).reshape(-1, 8)[:, :3], sm.state8(rows)[:, :3]), "the standing step moved an agent"
        flags = ora.get(capi.BUF_COL_FLAGS).reshape(-1, 4)[:, 0].astype(bool)
        if hits is not None:
            assert np.array_equal(flags, np.asarray(hits, bool).reshape(-1)), "the oracle's boundary flags are not the predicted crossings"
        tgs._check(devs + [ora], f"{name} N={N}: standing step")
        pf, pc = mp.list_first[0], mp.list_count[0]
        rng = np.random.default_rng(100 + N)
        acts = np.stack([rng.uniform(-0.2, 1.0, (8, B, N)), rng.uniform(-0.5, 0.5, (8, B, N))], axis=-1).astype(np.float32)
        dacts = torch.as_tensor(acts).cuda().contiguous()
        for k in range(8):
            one.env.step_autoreset(dacts[k], 5, 1 + k, pf, pc)
        for d in [many] + devs[2:]:
            d.env.step_autoreset_n(dacts, None, seed=5, counter0=1, path_first=pf, path_count=pc)
            d.env.sync()
        replaced = 0
        for k in range(8):
            ora.step(acts[k])
            replaced += int(ora.get(capi.BUF_DONE).astype(bool).sum())
            ora.auto_reset(5, 1 + k, pf, pc)
        assert replaced >= B, "no env was re-placed inside the launch"
        tgs._check(devs + [ora], f"{name} N={N}: step_autoreset_n of 8 steps")
        for d in devs[1:]:
            for which in tp.INT_BUFS + tp.FLT_BUFS:
                assert many.get(which).tobytes() == d.get(which).tobytes(), f"{name} N={N}: buffer {which} differs between the eight-step launch and " + \
                    ("eight single launches" if d is one else "the full scan")
        return flags
    finally:
        for e in devs + [ora]:
            e.close()


@pytest.mark.parametrize("N", sorted(SHAPES))
def test_tile_total_around_the_capacity_on_the_dense_map(N, monkeypatch):
    mp = tgs._map("dense")
    cap, cases, rows, want_total, want_hit = _dense_rows(N)
    S = SHAPES[N][0] * N
    assert cap == S * NEAR_CAP and len(rows) == len(cases) * S

    def expect(per):
        total = per.sum(axis=(1, 2))
        print(f"dense N={N}: capacity {cap}, tile totals {dict(zip(cases, total.tolist()))}")
        assert total.tolist() == want_total
        assert total[cases.index("below")] == cap - 1 if N > 1 else total[0] < cap
        assert total[cases.index("at")] == cap and total[cases.index("above")] == cap + 1
        if N == 1:
            assert total[cases.index("oneside")] >= 12 and (per[cases.index("oneside"), 0] > 0).sum() == 1  # all on one side of the one agent
        else:
            for t in range(len(cases)):
                assert per[t, 0].sum() > 0 and not want_hit[t][0] and any(want_hit[t][1:])  # slot 0: entries, no crossing; a later slot crosses (edges 1 .. 3 only)
        return want_hit
    _run(monkeypatch, "dense", mp, N, rows, expect)


@pytest.mark.parametrize("N", sorted(SHAPES))
def test_listed_segments_on_the_cpm_map(N, monkeypatch):
    mp = load_map("cpm_entire")
    S = SHAPES[N][0] * N
    rows = _cpm_rows(N, mp)

    def expect(per):
        total = per.sum(axis=(1, 2))
        print(f"cpm_entire N={N}: capacity {S * NEAR_CAP}, tile totals {total.tolist()}")
        assert (total <= S * NEAR_CAP).all() and (total > 0).all()  # the list holds them: the list walk runs, and has entries to walk
        return None
    flags = _run(monkeypatch, "cpm_entire", mp, N, rows, expect).reshape(-1, S)
    if N > 1:
        assert not flags[:, 0].any() and flags[:, 1:].any()  # crossings, none of them slot 0's
