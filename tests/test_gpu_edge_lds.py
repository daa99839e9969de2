"""Phase E of the step kernel on list entries that carry their segment's end points in LDS (run with -m gpu on an MI355X).

Phase E tests one listed segment per lane: the first pass takes entries 0 .. 63, a second one the rest; the first XY_CAP entries of the list have their end points
in LDS (in the bytes of the distance matrix: (S (N + 1) - 3) / 4 entries, at most the list's capacity), an entry beyond takes its segment from the map by its code.
On the `dense` map of tests/synthetic_maps.py a tile's total is put one below, at and one above 64 and XY_CAP (16 x 1: 67, 4 x 4: 19, 3 x 5: 14; the single-agent
tile has no room for coordinates and keeps the cases of tests/test_gpu_edge_list.py), and for every total the crossing agent is moved through every slot with
entries but slot 0, which always has entries and no crossing.  The list is filled left boundaries first, then right ones, each in slot order with rising segment
index, so the LAST slot's right-hand entries end the list: where the total lies above a boundary, that slot's crossing pose is searched such that every crossing
segment is among the entries beyond the boundary -- the crossing is then found by the second pass (or from the map) or not at all.  Counts and crossings are
predicted in float64 from the positions the oracle holds and asserted before the step, with the clearance of tests/test_gpu_edge_list.py.

After the standing step: an eight-step step_autoreset_n launch (max_steps = 5: every env is re-placed inside it; every step has its own random actions) against
eight single launches of a second handle, byte for byte in every buffer and in every record row, and against the oracle.

The entry / exit segments of phase C (the segment between the first, and between the last, points of a path's two boundaries, reached through the boundaries'
point counts): on every shipped map with a non-loop path and on all three paths of `long257` (255 / 250, 5 / 6 and 128 / 131 boundary points) agents stand astride
them; col_flags, done and timers after one step equal the oracle's bit for bit.  (A per-path row of these end points was measured and left out,
profiles/edge_lds_ab.txt; the cases hold whatever form reaches them.)"""
import functools
import os

import numpy as np
import pytest

import oracle_binding as ob
import synthetic_maps as sm
import test_gpu_edge_list as tel
import test_gpu_parity as tp
import test_gpu_scan_synthetic as tgs
from sigmarl_amd import capi
from sigmarl_amd.maps import ASSET_DIR, load_map
from sigmarl_amd.params import Parameters, make_config

pytestmark = pytest.mark.gpu

PASS = 64           # lanes of a pass of phase E: entries 64 and up are the second pass's
f32 = np.float32


def xy_cap(N):
    """Entries of the tile's list whose end points are kept in LDS (Smem::near_xy_cap)."""
    S = tel.SHAPES[N][0] * N
    return max(0, min(S * tel.NEAR_CAP, (S * (N + 1) - 3) // 4))


def _totals(N):
    bounds = [PASS] + ([xy_cap(N)] if xy_cap(N) not in (PASS, tel.SHAPES[N][0] * N * tel.NEAR_CAP) else [])
    return sorted({b + k for b in bounds for k in (-1, 0, 1)}), bounds


def _plan(S, T):
    """Slots with entries and their counts (6 .. 15 each): slots 0, 1, ... and the tile's last slot."""
    m = max(2, -(-T // 13))
    base, rem = divmod(T, m)
    return list(range(m - 1)) + [S - 1], [base + (k < rem) for k in range(m)]


def _crossings(poly, lo, hi, x, y, yaws):
    """[len(yaws), 4 edges, hi - lo] proper crossings of the rectangle's edges with segments lo .. hi - 1 of the polyline (float64 on the float32 inputs)."""
    rows = np.zeros((len(yaws), 6))
    rows[:, 2], rows[:, 3], rows[:, 4] = x, y, yaws
    v = sm.vertices(rows).astype(np.float64)
    a, b = poly[lo:hi].astype(np.float64)[None], poly[lo + 1:hi + 1].astype(np.float64)[None]

    def side(p, q, r):
        return (q[..., 0] - p[..., 0]) * (r[..., 1] - p[..., 1]) - (q[..., 1] - p[..., 1]) * (r[..., 0] - p[..., 0])
    out = []
    for e in range(4):
        p, q = v[:, e, None, :], v[:, e + 1, None, :]
        out.append((side(a, b, p) * side(a, b, q) < 0) & (side(p, q, a) * side(p, q, b) < 0))
    return np.stack(out, axis=1)


@functools.lru_cache(maxsize=None)
def _tail_state(side, s0, want, tail):
    """A pose beyond boundary `side` of the dense map with exactly `want` near segments of which only the `tail` with the highest indices are crossed, by edges
    other than edge 0 (and with the same crossings 0.004 rad to either side of the yaw: no prediction hinges on a rounding)."""
    p = sm.paths("dense")[0]
    poly, other, sign = (p["left"], p["right"], 1.0) if side == 0 else (p["right"], p["left"], -1.0)
    dy = np.arange(-3.1, 3.1, 0.002)
    for s in s0 + 0.0011 * np.arange(12):
        for d in np.arange(sm.LANE_HALF + 0.03, sm.LANE_HALF + sm.RECT_RADIUS, 1e-4):
            x, y, yaw0 = sm._pose(p["curve"], s, sign * d)
            x, y = float(f32(x)), float(f32(y))
            n, clear = tel._count(poly, x, y)
            if n != want or not clear:
                continue
            n_other, clear_other = tel._count(other, x, y)
            if n_other or not clear_other:
                continue
            near = np.where(tel._seg_dist(poly, x, y) <= sm.NEAR_RADIUS)[0]
            lo, hi = max(int(near[0]) - 2, 0), min(int(near[-1]) + 3, len(poly) - 1)
            yaws = (yaw0 + dy).astype(f32).astype(np.float64)
            c = _crossings(poly, lo, hi, x, y, yaws)
            in_tail = np.zeros(hi - lo, bool)
            in_tail[near[-tail:] - lo] = True
            ok = ~c[:, 0].any(-1) & c[:, 1:][:, :, in_tail].any((1, 2)) & ~c[:, :, ~in_tail].any((1, 2))
            ok = ok & np.roll(ok, 2) & np.roll(ok, -2) & np.roll(ok, 1) & np.roll(ok, -1)
            ok[:2] = ok[-2:] = False
            if ok.any():
                return x, y, float(yaws[int(np.argmax(ok))])
    raise AssertionError((side, s0, want, tail))


@functools.lru_cache(maxsize=None)
def _dense_cases(N):
    """(rows, per tile: (total, crossing slot, entries the crossing must come from: first index or None), per tile per slot: crossing expected)."""
    G = tel.SHAPES[N][0]
    S = G * N
    p = sm.paths("dense")[0]
    n_pts = len(p["center"])
    totals, bounds = _totals(N)
    rows, tiles, hits = [], [], []
    for T in totals:
        slots, counts = _plan(S, T)
        below = [b for b in bounds if b < T]
        for j in slots[1:]:
            hit = []
            for k in range(S):
                s = p["length"] * (0.12 + 0.76 * k / (S - 1))
                if k not in slots:
                    x, y, yaw = sm._pose(p["curve"], s, 2.0 + 0.4 * k)
                else:
                    want = counts[slots.index(k)]
                    side = 1 if k == S - 1 else k % 2
                    if k == j and k == S - 1 and below:
                        x, y, yaw = _tail_state(side, s, want, T - max(below))
                    else:
                        x, y, yaw = tel._dense_state(side, s, want, False, k == j)
                hit.append(k == j)
                rows.append((0, int(np.clip(round(s / p["length"] * (n_pts - 1)), 1, n_pts - 2)), x, y, yaw, 0.0))
            tiles.append((T, j, max(below) if (j == S - 1 and below) else None))
            hits.append(hit)
    return np.asarray(rows, np.float64), tiles, hits


def _bits(t):
    import torch

    return t.contiguous().view(torch.int32)


def _run(monkeypatch, name, mp, N, rows, expect):
    """tests/test_gpu_edge_list.py::_run with the record rows of both forms of the eight steps compared as well."""
    import torch

    G, inst = tel.SHAPES[N]
    B = len(rows) // N
    p = Parameters(n_agents=N, scenario_type=name, is_use_mtv_distance=False, rew_method="distance", dt=0.05, is_apply_mask=False, is_obs_noise=False,
                   max_steps=tel.MAX_STEPS)
    cfg = make_config(p, mp, B)
    cfg.envs_per_group = G
    many, one, ora = tgs._handle(monkeypatch, cfg, mp), tgs._handle(monkeypatch, cfg, mp), ob.OracleEnv(cfg, mp)
    devs = [many, one] + ([tgs._handle(monkeypatch, cfg, mp, {"SIGMAENV_PRUNE": 0})] if N == 16 else [])
    try:
        ls = many.env.launch_shape()
        assert (ls["wave_G"], ls["wave_wpb"], ls["pruned_scan"]) == (G, 1, 1) and ls["instantiation"] == inst, ls
        place = tel._placement(mp, N, rows)
        for e in devs + [ora]:
            e.reset(*place, 1)
            e.observe()
        hits = expect(tel._tile_counts(mp, ora, N, G * N), ora)
        stand = np.zeros((B, N, 2), np.float32)
        for e in devs + [ora]:
            e.step(stand)
        assert np.array_equal(ora.get(capi.BUF_STATE).reshape(-1, 8)[:, :3], sm.state8(rows)[:, :3]), "the standing step moved an agent"
        flags = ora.get(capi.BUF_COL_FLAGS).reshape(-1, 4)[:, 0].astype(bool)
        assert np.array_equal(flags, np.asarray(hits, bool).reshape(-1)), "the oracle's boundary flags are not the predicted crossings"
        tgs._check(devs + [ora], f"{name} N={N}: standing step")
        for d in devs:
            for which in (capi.BUF_COL_FLAGS, capi.BUF_DONE, capi.BUF_TIMER):
                assert d.get(which).tobytes() == ora.get(which).tobytes(), f"{name} N={N}: buffer {which} differs from the oracle after the standing step"
        pf, pc = mp.list_first[0], mp.list_count[0]
        rng = np.random.default_rng(200 + N)
        acts = np.stack([rng.uniform(-0.2, 1.0, (8, B, N)), rng.uniform(-0.5, 0.5, (8, B, N))], axis=-1).astype(np.float32)
        dacts = torch.as_tensor(acts).cuda().contiguous()
        W = N * (many.env.D + 1) + 1
        rec_many, rec_one = torch.zeros((8, B, W), device="cuda"), torch.zeros((8, B, W), device="cuda")
        for k in range(8):
            one.env.set_slab(rec_one[k])
            one.env.step_autoreset(dacts[k], 5, 1 + k, pf, pc)
        one.env.sync()
        one.env.set_slab(None)
        many.env.step_autoreset_n(dacts, rec_many, seed=5, counter0=1, path_first=pf, path_count=pc)
        many.env.sync()
        for d in devs[2:]:
            d.env.step_autoreset_n(dacts, None, seed=5, counter0=1, path_first=pf, path_count=pc)
            d.env.sync()
        replaced = 0
        for k in range(8):
            ora.step(acts[k])
            replaced += int(ora.get(capi.BUF_DONE).astype(bool).sum())
            ora.auto_reset(5, 1 + k, pf, pc)
        assert replaced >= B, "no env was re-placed inside the launch"
        for k in range(8):
            assert torch.equal(_bits(rec_many[k]), _bits(rec_one[k])), f"{name} N={N}: record row of step {k} differs between the eight-step launch and eight single launches"
        tgs._check(devs + [ora], f"{name} N={N}: step_autoreset_n of 8 steps")
        for d in devs[1:]:
            for which in tp.INT_BUFS + tp.FLT_BUFS:
                assert many.get(which).tobytes() == d.get(which).tobytes(), f"{name} N={N}: buffer {which} differs between the eight-step launch and " + \
                    ("eight single launches" if d is one else "the full scan")
    finally:
        for e in devs + [ora]:
            e.close()


@pytest.mark.parametrize("N", [16, 4, 3])
def test_totals_around_the_pass_and_the_coordinate_capacity(N, monkeypatch):
    mp = tgs._map("dense")
    G = tel.SHAPES[N][0]
    S = G * N
    rows, tiles, want_hit = _dense_cases(N)
    totals, bounds = _totals(N)
    assert {16: [64, 67], 4: [64, 19], 3: [64, 14]}[N] == bounds and len(rows) == len(tiles) * S

    def expect(per, ora):
        total = per.sum(axis=(1, 2))
        print(f"dense N={N}: pass {PASS}, coordinate capacity {xy_cap(N)}, list capacity {S * tel.NEAR_CAP}; tile totals {sorted(set(total.tolist()))}, {len(tiles)} tiles")
        assert total.tolist() == [t[0] for t in tiles] and sorted(set(total.tolist())) == totals and total.max() <= S * tel.NEAR_CAP
        st = ora.get(capi.BUF_STATE).reshape(-1, S, 8)
        poly = sm.paths("dense")[0]
        seen_beyond = set()
        for t, (T, j, first) in enumerate(tiles):
            assert per[t, 0].sum() > 0 and not want_hit[t][0] and want_hit[t][j] and sum(want_hit[t]) == 1  # slot 0: entries, no crossing; one later slot crosses
            x, y, yaw = (float(v) for v in st[t, j, :3])
            side = 1 if j == S - 1 else j % 2
            pl = poly["left" if side == 0 else "right"]
            c = _crossings(pl, 0, len(pl) - 1, x, y, np.array([yaw]))[0]
            assert not c[0].any() and c[1:].any(), "the crossing agent: edges other than edge 0 only"
            if first is not None:
                # the list: left boundaries, then right ones, each in slot order with rising segment index -- the last slot's right-hand entries end it
                assert per[t, S - 1, 0] == 0 and per[t, S - 1, 1] > 0
                near = np.where(tel._seg_dist(pl, x, y) <= sm.NEAR_RADIUS)[0]
                pos = T - len(near) + np.arange(len(near))  # list positions of the slot's entries
                crossed = np.where(c.any(0))[0]
                assert set(crossed) <= set(near[pos >= first]), "a crossing segment is listed before the boundary"
                seen_beyond.add(first)
        assert seen_beyond == {b for b in bounds if b < max(totals)}, "no crossing that only entries beyond each boundary find"
        return want_hit
    _run(monkeypatch, "dense", mp, N, rows, expect)


def test_single_agent_tile_takes_every_segment_from_the_map(monkeypatch):
    """1 x 1: capacity 8, no room for coordinates (XY_CAP = 0) -- the cases of tests/test_gpu_edge_list.py on the by-code path."""
    assert xy_cap(1) == 0
    mp = tgs._map("dense")
    cap, cases, rows, want_total, want_hit = tel._dense_rows(1)

    def expect(per, ora):
        assert per.sum(axis=(1, 2)).tolist() == want_total
        return want_hit
    _run(monkeypatch, "dense", mp, 1, rows, expect)


# ---- the entry / exit segments of phase C --------------------------------------------------------------------------------------------------------------------
def _shipped_maps():
    return sorted(f[:-4] for f in os.listdir(ASSET_DIR) if f.endswith(".npz"))


def _entry_exit_rows(mp, N, max_paths=6):
    """One env per tested non-loop path: slot 0 on the lane in the middle of the path, slot 1 astride the entry segment, the last slot astride the exit segment,
    the others far off the map.  Paths: the first `max_paths` non-loop ones and every non-loop one whose boundaries differ in their point counts (at most 3)."""
    nonloop = [gp for gp in range(len(mp.is_loop)) if not mp.is_loop[gp]]
    paths = nonloop[:max_paths] + [gp for gp in nonloop[max_paths:] if mp.n_left[gp] != mp.n_right[gp]][:3]
    rows, ids = [], []
    for gp in paths:
        lst = next((k for k in sorted(mp.list_first) if mp.list_first[k] <= gp < mp.list_first[k] + mp.list_count[k]), 0)
        n, nl, nr = int(mp.n_center[gp]), int(mp.n_left[gp]), int(mp.n_right[gp])
        ny = int(mp.n_yaw[gp])
        for k in range(N):
            if k == 1 or (k == N - 1 and N > 2):
                a, b = (mp.left[gp, 0], mp.right[gp, 0]) if k == 1 else (mp.left[gp, nl - 1], mp.right[gp, nr - 1])
                c = (a.astype(np.float64) + b.astype(np.float64)) / 2
                pt = 1 if k == 1 else n - 2
                rows.append((gp, pt, float(f32(c[0])), float(f32(c[1])), float(mp.yaw[gp, min(pt, ny - 1)]), 0.0))
            elif k == 0:
                c = mp.center[gp, n // 2].astype(np.float64)
                rows.append((gp, n // 2, float(c[0]), float(c[1]), float(mp.yaw[gp, min(n // 2, ny - 1)]), 0.0))
            else:
                c = mp.center[gp, n // 2].astype(np.float64)
                rows.append((gp, n // 2, float(f32(c[0] + 3.0 + 0.5 * k)), float(f32(c[1] - 3.0 - 0.5 * k)), 0.3 * k, 0.0))
            ids.append((gp, 0, gp - mp.list_first[lst], rows[-1][1]))
    return paths, np.asarray(rows, np.float64), np.asarray(ids, np.int32)


def _entry_exit_once(monkeypatch, name, mp, N):
    G = tel.SHAPES[N][0]
    paths, rows, ids = _entry_exit_rows(mp, N)
    B = len(paths)
    p = Parameters(n_agents=N, scenario_type=name, is_use_mtv_distance=False, rew_method="distance", dt=0.05, is_apply_mask=False, is_obs_noise=False)
    cfg = make_config(p, mp, B)
    cfg.envs_per_group = G
    dev, ora = tgs._handle(monkeypatch, cfg, mp), ob.OracleEnv(cfg, mp)
    try:
        assert dev.env.launch_shape()["wave_G"] == G
        place = (np.repeat(np.arange(B), N).astype(np.int32), np.tile(np.arange(N), B).astype(np.int32), ids, sm.state8(rows))
        for e in (dev, ora):
            e.reset(*place, 1)
            e.observe()
        st = ora.get(capi.BUF_STATE).reshape(-1, 8)
        want = np.zeros((B * N, 2), bool)
        for i, gp in enumerate(np.repeat(paths, N)):
            x, y, yaw = (float(v) for v in st[i, :3])
            nl, nr = int(mp.n_left[gp]), int(mp.n_right[gp])
            want[i, 0] = any(tel._edges_crossing(np.stack([mp.left[gp, 0], mp.right[gp, 0]]), x, y, yaw))
            want[i, 1] = any(tel._edges_crossing(np.stack([mp.left[gp, nl - 1], mp.right[gp, nr - 1]]), x, y, yaw))
        want = want.reshape(B, N, 2)
        assert want[:, 1, 0].all() and (N == 1 or want[:, N - 1, 1].all()), "the placed agents do not stand astride the entry / exit segments"
        stand = np.zeros((B, N, 2), np.float32)
        for e in (dev, ora):
            e.step(stand)
        cf = ora.get(capi.BUF_COL_FLAGS).reshape(B, N, 4)
        assert np.array_equal(cf[..., 1:3].astype(bool), want), f"{name} N={N}: the oracle's entry / exit bytes are not the predicted crossings"
        if cfg.has_entry_exit:
            assert cf[..., 3].any(), f"{name} N={N}: no reset request"
        for which in (capi.BUF_COL_FLAGS, capi.BUF_DONE, capi.BUF_TIMER):
            assert dev.get(which).tobytes() == ora.get(which).tobytes(), f"{name} N={N}: buffer {which} differs from the oracle"
        return [(int(mp.n_left[gp]), int(mp.n_right[gp])) for gp in paths]
    finally:
        for e in (dev, ora):
            e.close()


@pytest.mark.parametrize("N", [16, 4, 3])
def test_entry_and_exit_segments_of_every_map(N, monkeypatch):
    counts = _entry_exit_once(monkeypatch, "long257", tgs._map("long257"), N)
    assert any(nl > nr for nl, nr in counts) and any(nl < nr for nl, nr in counts)  # boundaries with different point counts, either way round
    tested = 0
    for name in _shipped_maps():
        mp = load_map(name)
        if not (np.asarray(mp.is_loop) == 0).any():
            continue
        _entry_exit_once(monkeypatch, name, mp, N)
        tested += 1
    assert tested >= 1
