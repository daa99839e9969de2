"""The polyline scan on synthetic maps beyond the shipped ones, on the host: the C oracle against the reference (tests/golden/scan_synthetic.npz, written by
tests/golden/gen/gen_scan_synthetic.py from the reference's get_perpendicular_distances and interX), and the conditions that keep the GPU tests of
tests/test_gpu_scan_synthetic.py from showing nothing -- each computed from the golden and numpy float64 alone, never from the code under test.

Bar of the oracle comparison: what tests/test_oracle_golden.py applies to the same functions on functions.npz -- distances, indices and flags bit for bit (same
float32 inputs, same arithmetic)."""
import os

import numpy as np
import pytest

import oracle_binding as ob
import synthetic_maps as sm
import traj_replay as tr
from sigmarl_amd.maps import MapTable

KEYS = ("center", "left", "right")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(tr.GOLDEN_DIR, "scan_synthetic.npz"))


def _poly(gold, name, key, path):
    return np.ascontiguousarray(gold[f"{name}_{key}"][path, :int(gold[f"{name}_n_{key}"][path])], np.float32)


def _segment_distances(poly, x, y):
    """float64 distance of (x, y) to every segment of the float32 polyline."""
    a, b = poly[:-1].astype(np.float64), poly[1:].astype(np.float64)
    ab, q = b - a, np.array([x, y], np.float64)
    t = np.clip(((q - a) * ab).sum(-1) / (ab * ab).sum(-1), 0.0, 1.0)
    return np.linalg.norm(a + ab * t[:, None] - q, axis=-1)


@pytest.mark.parametrize("name", sm.NAMES)
def test_golden_holds_the_tables_and_states_of_the_helper(gold, name):
    tab = sm.table(name)
    for k in KEYS + ("yaw", "n_center", "n_left", "n_right", "n_yaw", "is_loop"):
        assert np.array_equal(gold[f"{name}_{k}"], tab[k]), k
    assert np.array_equal(gold[f"{name}_states"], sm.states(name)) and np.array_equal(gold[f"{name}_tele_states"], sm.teleported(name))
    assert np.array_equal(gold[f"{name}_vertices"], sm.vertices(sm.states(name)))
    assert len(sm.states(name)) == sm.N_STATES <= 24 * 4


@pytest.mark.parametrize("name", sm.NAMES)
def test_oracle_polyline_functions_equal_the_reference(gold, name):
    lib = ob.load_oracle()
    for tag in ("", "tele_"):
        rows, verts = gold[f"{name}_{tag}states"], gold[f"{name}_{tag}vertices"]
        pts = np.concatenate([rows[:, None, 2:4].astype(np.float32), verts[:, :4]], axis=1)
        for pi in np.unique(rows[:, 0].astype(int)):
            sel = np.nonzero(rows[:, 0].astype(int) == pi)[0]
            for q, key in enumerate(KEYS):
                poly = _poly(gold, name, key, pi)
                for c in range(5 if q else 1):
                    p = np.ascontiguousarray(pts[sel, c])
                    d, idx = np.zeros(len(sel), np.float32), np.zeros(len(sel), np.int32)
                    lib.fn_point_polyline(len(sel), ob.ptr(p), ob.ptr(poly), len(poly), ob.ptr(d), ob.ptr(idx))
                    assert np.array_equal(d, gold[f"{name}_{tag}dist"][sel, q, c]), (name, tag, pi, key, c)
                    if c == 0:
                        assert np.array_equal(idx, gold[f"{name}_{tag}closest"][sel, q]), (name, tag, pi, key)
                if q:
                    v = np.ascontiguousarray(verts[sel])
                    hit = np.zeros(len(sel), np.uint8)
                    lib.fn_interx(len(sel), ob.ptr(v), 5, 10, ob.ptr(poly), len(poly), 0, ob.ptr(hit))
                    assert np.array_equal(hit, gold[f"{name}_{tag}hit"][sel, q - 1]), (name, tag, pi, key)


def test_point_counts_are_what_the_maps_promise(gold):
    for name, n in (("long257", 257), ("long258", 258)):
        assert [int(gold[f"{name}_n_{k}"][0]) for k in KEYS] == [n, 255, 250]
        assert [int(gold[f"{name}_n_{k}"][1]) for k in KEYS] == [5, 5, 6] and int(gold[f"{name}_n_center"][2]) == 130
    assert all(200 <= int(gold[f"dense_n_{k}"][0]) <= 257 for k in KEYS) and int(gold["dense_n_left"][0]) == 257
    for k in KEYS:
        d = np.linalg.norm(np.diff(_poly(gold, "dense", k, 0).astype(np.float64), axis=0), axis=1)
        assert 0.011 < d.min() and d.max() < 0.016
    assert int(gold["hairpin_n_center"][0]) == 257 and int(gold["hairpin_is_loop"][1]) == 1
    for k in KEYS:
        loop = _poly(gold, "hairpin", k, 1)
        assert np.array_equal(loop[0], loop[-1])
    # the hairpin comes back within 0.1 .. 0.3 m of itself: chunk 3 and chunk 60 of its centre line and of its left boundary are spatial neighbours
    for k, lo, hi in (("center", 0.29, 0.31), ("left", 0.09, 0.11)):
        p = _poly(gold, "hairpin", k, 0).astype(np.float64)
        gap = np.linalg.norm(p[12:17, None] - p[None, 240:245], axis=-1).min()
        assert lo < gap < hi, (k, gap)
    # origin: a point at (0, 0) and a segment whose float32 squared length is below 2^-60 (and not zero)
    for k in ("center", "left"):
        p = _poly(gold, "origin", k, 0)
        l = np.diff(p, axis=0)
        len2 = (l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1]).astype(np.float32)
        assert 0 < len2.min() < 2.0 ** -60
    assert (_poly(gold, "origin", "center", 0) == 0).all(axis=1).any()


def test_states_reach_the_last_chunks_of_every_polyline_of_long257(gold):
    """Closest index >= 252 (segment 251 .. 255: chunks 62 and 63, the last bits of the 64-bit masks, and the largest values of the uint8 near list) for at least 8
    agents on the centre line (257 points) and on the left boundary (255 points).  The right boundary has 250 points: its largest possible index is 249, so there
    the bar is its own last two chunks (index >= 246: segments 245 .. 248, chunks 61 and 62)."""
    on0 = gold["long257_states"][:, 0] == 0
    cl = gold["long257_closest"][on0]
    assert (cl[:, 0] >= 252).sum() >= 8 and (cl[:, 1] >= 252).sum() >= 8 and (cl[:, 2] >= 246).sum() >= 8, [(cl[:, q] >= 252).sum() for q in range(3)]
    assert cl[:, 0].max() == 256 and cl[:, 1].max() == 254 and cl[:, 2].max() == 249  # the very last segment of each


def test_near_list_counts_bracket_its_capacity(gold):
    """(agent, side) pairs with exactly 8 (NEAR_CAP: the list is full, not overflowed), exactly 9 (overflowed by one) and 12 or more boundary segments within
    rect_radius + 1e-4 of the centre: at least four each, on `dense`."""
    counts = []
    for row in gold["dense_states"]:
        for key in ("left", "right"):
            counts.append(int((_segment_distances(_poly(gold, "dense", key, int(row[0])), np.float32(row[2]), np.float32(row[3])) <= sm.NEAR_RADIUS).sum()))
    counts = np.asarray(counts)
    assert (counts == 8).sum() >= 4 and (counts == 9).sum() >= 4 and (counts >= 12).sum() >= 4, np.bincount(counts)
    # and on the long maps a straddling vehicle stays below the capacity (0.05 m spacing): the overflow is the dense map's business
    assert counts.max() >= 16


@pytest.mark.parametrize("name", sm.NAMES)
def test_far_states_and_collision_shares(gold, name):
    # neigh_radius_far as sigmaenv_create forms it: 9 x the float32 circumradius -- beyond it the two-level search over all boxes runs
    far = 9.0 * sm.RECT_RADIUS
    assert (gold[f"{name}_dist"][:, 0, 0] > far).sum() >= 4
    assert (gold[f"{name}_dist"][:, 0, 0] > 40.0).sum() >= 2  # the 50 m ones: every chunk is a candidate
    hit = gold[f"{name}_hit"].any(axis=1)
    assert hit.mean() >= 0.2 and (~hit).mean() >= 0.2, hit.mean()
    # ... in every prefix the agent counts of the GPU tests use (96 = 6 x 16 = 24 x 4, 72 = 24 x 3, 24 = 24 x 1)
    for m in (72, 24):
        assert hit[:m].mean() >= 0.2 and (~hit[:m]).mean() >= 0.2, (m, hit[:m].mean())


def test_hairpin_teleports_leave_a_stale_index(gold):
    """The far-teleport reset moves an agent to the other leg: its nearest boundary segment is more than 100 indices from the one before."""
    on0 = gold["hairpin_states"][:, 0] == 0
    jump = np.abs(gold["hairpin_tele_closest"][on0, 1:].astype(int) - gold["hairpin_closest"][on0, 1:].astype(int)).max(axis=1)
    assert (jump > 100).sum() >= 4
    near = np.linalg.norm(gold["hairpin_tele_states"][on0, 2:4] - gold["hairpin_states"][on0, 2:4], axis=1)
    assert ((jump > 100) & (near < 0.5)).sum() >= 4  # ... although the agent moved less than half a metre (the other leg lies 0.3 m beside)


def test_exact_ties_take_the_first_index(gold):
    n_ties = 0
    for name in sm.NAMES:
        rows = gold[f"{name}_states"]
        for i, row in enumerate(rows):
            for q, key in enumerate(KEYS):
                d = _segment_distances(_poly(gold, name, key, int(row[0])), np.float32(row[2]), np.float32(row[3]))
                first = int(np.argmin(d))
                if (d == d[first]).sum() >= 2:  # two segments at exactly the same distance
                    n_ties += 1
                    assert int(gold[f"{name}_closest"][i, q]) == first + 1, (name, i, key)
    assert n_ties >= 5


def test_maptable_accepts_the_maps_and_refuses_duplicate_points():
    for name in sm.NAMES:
        mp = MapTable(name, table=sm.table(name))
        assert mp.n_paths == len(sm.paths(name)) and mp.list_count[0] == mp.n_paths
    with pytest.raises(ValueError, match="points 60 and 61 coincide"):
        MapTable("duplicate", table=sm.duplicate_point_table())
