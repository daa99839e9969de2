"""The pruned scan's create-time neighbour table (NeighRow, neigh_rows_build in sigmarl_amd/csrc/sigmaenv_device.h), read back through sigmaenv_neigh_rows -- the
very function sigmaenv_create fills the device table with; no GPU, no handle.

Per chunk of a polyline and per radius (tight / near / far) the library keeps the neighbour chunks twice: as a bit set (own chunk included), which is what the
list is cut from, and as what the step kernel walks: ONE list of index bytes without the own chunk -- the tight ring, then what the near radius adds, then what the
far radius adds, each ring ascending -- and per level the length of its prefix, or the overflow mark when the level has more neighbours than the list holds (the
kernel then takes the search over the group boxes).  Held here, for every polyline of at most 64 chunks of every shipped map and of every map of
tests/synthetic_maps.py:

  * the bit sets equal the rule restated in numpy (float64 box distance of the float32 boxes, `<= radius + 1e-5`, the three float32 radii),
  * a level's prefix + own chunk == the bits of the level's set, every ring ascending, the bytes past the list's end repeating its last entry; a marked level is one
    whose neighbour count exceeds the capacity, every wider level is marked with it, and the list stops with the widest level that fits,
  * the levels nest (tight within near within far), which is what makes a position past a prefix harmless: it is a chunk of a wider ring, or one tested twice,

and, from the maps alone, that the set of maps reaches a row with two runs of neighbours, a level at exactly its capacity and a level one above it."""
import glob
import os

import numpy as np
import pytest

import synthetic_maps as sm
import test_scan_bound_host as th
from sigmarl_amd import capi
from sigmarl_amd.maps import ASSET_DIR, load_map

f32 = np.float32
CAP = 28               # NEIGH_CAP: list bytes of the 32-byte row; the three counts follow at 28, 29, 30, a pad byte at 31
OVERFLOW = 255         # NEIGH_OVERFLOW
LEVELS = ("tight", "near", "far")
SHIPPED = tuple(sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(ASSET_DIR, "*.npz")) if "pseudo_distance" not in p))
MAPS = sm.NAMES + SHIPPED
RADII = tuple(f32(k) * f32(sm.RECT_RADIUS) for k in (3.6, 6.0, 9.0))  # sigmaenv_create: multiples of the rectangle's float32 circumradius

_rows = {}


def map_table(name):
    return th.map_table(name) if name in sm.NAMES else load_map(name)


def restated_masks(boxes):
    """[nch, 3] bit sets by the rule of neigh_rows_build, in numpy."""
    b = boxes.astype(np.float64)
    dx = np.maximum(np.maximum(b[:, None, 0] - b[None, :, 2], b[None, :, 0] - b[:, None, 2]), 0.0)
    dy = np.maximum(np.maximum(b[:, None, 1] - b[None, :, 3], b[None, :, 1] - b[:, None, 3]), 0.0)
    dd = np.sqrt(dx * dx + dy * dy)
    return [[sum(1 << int(c) for c in np.nonzero(dd[a] <= float(r) + 1e-5)[0]) for r in RADII] for a in range(len(b))]


def table_rows(name):
    """[(path, polyline, boxes, rows uint8 [nch, 32], masks [nch][3] as Python ints)] of the map's polylines of at most 64 chunks."""
    if name not in _rows:
        lib = capi.load_library()
        mp = map_table(name)
        out = []
        for path in range(mp.n_paths):
            for pl in range(3):
                boxes = np.ascontiguousarray(th.chunk_boxes(th.polyline(mp, path, pl)), f32)
                nch = len(boxes)
                if nch < 1 or nch > 64:
                    continue
                rows, masks = np.full((nch, 32), 0xAA, np.uint8), np.zeros((nch, 3), np.uint64)
                rc = lib.neigh_rows(boxes.ctypes.data, nch, sm.LENGTH, sm.WIDTH, rows.ctypes.data, masks.ctypes.data)
                assert rc == 0, (name, path, pl, rc)
                out.append((path, pl, boxes, rows, [[int(x) for x in m] for m in masks]))
        _rows[name] = out
    return _rows[name]


def bits(mask):
    return [c for c in range(64) if (mask >> c) & 1]


def runs(idx):
    return sum(1 for j, c in enumerate(idx) if j == 0 or c != idx[j - 1] + 1)


@pytest.mark.parametrize("name", MAPS)
def test_masks_equal_the_restated_rule(name):
    got = table_rows(name)
    assert got or name == "long258", name
    for path, pl, boxes, _, masks in got:
        assert masks == restated_masks(boxes), (name, path, pl)
        for a, m in enumerate(masks):
            assert (m[0] >> a) & 1 and m[0] & ~m[1] == 0 and m[1] & ~m[2] == 0, (name, path, pl, a)  # the own chunk; the levels nest


@pytest.mark.parametrize("name", MAPS)
def test_lists_hold_the_bits_of_their_masks(name):
    for path, pl, _, rows, masks in table_rows(name):
        for a, row in enumerate(rows):
            lst, cnts = [int(x) for x in row[:CAP]], [int(x) for x in row[CAP:CAP + 3]]
            assert row[31] == 0, (name, path, pl, a)
            stored, marked = 0, False
            for lvl in range(3):
                want = [c for c in bits(masks[a][lvl]) if c != a]
                tag = (name, path, pl, a, LEVELS[lvl])
                if cnts[lvl] == OVERFLOW:  # a marked level: more neighbours than the list holds; every wider level is marked with it
                    assert len(want) > CAP, tag
                    marked = True
                else:
                    assert not marked and len(want) <= CAP and cnts[lvl] == len(want), tag
                    ring = lst[stored:cnts[lvl]]
                    assert ring == sorted(ring) and sorted(lst[:cnts[lvl]]) == want, tag  # the level's prefix is the level's set; what the level adds is ascending
                    assert sum(1 << c for c in lst[:cnts[lvl]]) | (1 << a) == masks[a][lvl], tag
                    stored = cnts[lvl]
            assert lst[stored:] == [lst[stored - 1] if stored else 0] * (CAP - stored), (name, path, pl, a)  # past the end: the last entry again (tested twice, the same bit)


def test_polylines_beyond_the_masks_are_refused():
    lib = capi.load_library()
    boxes, rows = np.zeros((65, 4), f32), np.zeros((65, 32), np.uint8)
    assert lib.neigh_rows(boxes.ctypes.data, 65, sm.LENGTH, sm.WIDTH, rows.ctypes.data, None) != 0
    assert lib.neigh_rows(boxes.ctypes.data, 0, sm.LENGTH, sm.WIDTH, rows.ctypes.data, None) != 0


def test_maps_reach_two_runs_the_capacity_and_one_above():
    """From the maps alone (the restated rule, no library): some level's neighbours + own chunk form two runs of indices, some level has exactly as many neighbours
    as its list holds, and some level has one more.  On the map of the headline too: two runs."""
    seen = {"two_runs": set(), "at_capacity": set(), "one_above": set()}
    for name in MAPS:
        mp = map_table(name)
        for path in range(mp.n_paths):
            for pl in range(3):
                boxes = th.chunk_boxes(th.polyline(mp, path, pl))
                if not 1 <= len(boxes) <= 64:
                    continue
                for a, m in enumerate(restated_masks(boxes)):
                    for lvl in range(3):
                        n = len(bits(m[lvl])) - 1
                        if runs(bits(m[lvl])) == 2:
                            seen["two_runs"].add(name)
                        if n == CAP:
                            seen["at_capacity"].add((name, LEVELS[lvl]))
                        if n == CAP + 1:
                            seen["one_above"].add((name, LEVELS[lvl]))
    assert "cpm_entire" in seen["two_runs"] and "hairpin" in seen["two_runs"], seen["two_runs"]
    assert seen["at_capacity"] and seen["one_above"], seen
