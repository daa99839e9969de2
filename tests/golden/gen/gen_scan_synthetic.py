"""Ground truth of the polyline scan on the synthetic maps of tests/synthetic_maps.py, from the reference's own functions.

Runs `get_perpendicular_distances` and `interX` (sigmarl/helper_scenario.py:829, :1148) on every map and query state (the placed states and the states the far
teleport moves the agents to) and writes tests/golden/scan_synthetic.npz plus its line of tests/golden/MANIFEST.json.  Data only: tables, states, the
rectangles' corner points (float32, tests/synthetic_maps.vertices), distances (centre point and the four corners to the left and right boundary, centre point to
the centre line), closest indices (the reference's argmin + 1) and the rectangle-versus-boundary flags.

    python tests/golden/gen/gen_scan_synthetic.py

The exact duplicate point (synthetic_maps.duplicate_point_table) is tried first: the reference must stop at its own NaN assertion there -- that is why the fixture
holds no such map and the package refuses one.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(TESTS, "golden")
TABLE_KEYS = ("center", "left", "right", "yaw", "n_center", "n_left", "n_right", "n_yaw", "is_loop")


def content_hash(path):
    z = np.load(path)
    h = hashlib.sha256()
    for k in sorted(z.files):
        a = np.ascontiguousarray(z[k])
        h.update(k.encode()); h.update(str(a.dtype).encode()); h.update(str(a.shape).encode()); h.update(a.tobytes())
    return h.hexdigest()


def main():
    sys.path.insert(0, HERE)
    sys.path.insert(0, TESTS)
    import refshim

    refshim.install()
    import torch
    from sigmarl.helper_scenario import get_perpendicular_distances, interX

    import synthetic_maps as sm

    # the duplicate point: 0 / 0 in the projection, and the reference's own assertion
    dup = sm.duplicate_point_table()
    try:
        get_perpendicular_distances(torch.tensor([[0.01, 0.02]], dtype=torch.float32), torch.from_numpy(dup["center"][0, :int(dup["n_center"][0])]))
        raise SystemExit("the reference accepted a duplicate point: decide its semantics before refusing it")
    except AssertionError:
        print("duplicate consecutive point: the reference stops at `assert not distances.isnan().any()`")

    out = {}
    for name in sm.NAMES:
        tab = sm.table(name)
        for k in TABLE_KEYS:
            out[f"{name}_{k}"] = tab[k]
        for tag, rows in (("", sm.states(name)), ("tele_", sm.teleported(name))):
            verts = sm.vertices(rows)
            pts = np.concatenate([np.stack([rows[:, 2], rows[:, 3]], -1).astype(np.float32)[:, None], verts[:, :4]], axis=1)  # centre, four corners
            M = len(rows)
            dist = np.zeros((M, 3, 5), np.float32)      # [state, centre line / left / right, centre point + 4 corners] (centre line: the centre point only)
            idx = np.zeros((M, 3), np.int32)
            hit = np.zeros((M, 2), np.uint8)
            for pi in np.unique(rows[:, 0].astype(int)):
                sel = np.nonzero(rows[:, 0].astype(int) == pi)[0]
                for q, key in enumerate(("center", "left", "right")):
                    poly = torch.from_numpy(np.ascontiguousarray(tab[key][pi, :int(tab["n_" + key][pi])]))
                    for c in range(5 if q else 1):
                        d, i = get_perpendicular_distances(torch.from_numpy(np.ascontiguousarray(pts[sel, c])), poly)
                        dist[sel, q, c] = d.numpy()
                        if c == 0:
                            idx[sel, q] = i.numpy()
                    if q:
                        L1 = torch.from_numpy(np.ascontiguousarray(verts[sel]))
                        hit[sel, q - 1] = interX(L1, poly.unsqueeze(0).expand(len(sel), -1, -1)).numpy()
            out[f"{name}_{tag}states"] = rows
            out[f"{name}_{tag}vertices"] = verts
            out[f"{name}_{tag}dist"] = dist
            out[f"{name}_{tag}closest"] = idx
            out[f"{name}_{tag}hit"] = hit
        print(name, "colliding", int(out[f"{name}_hit"].any(-1).sum()), "of", len(out[f"{name}_hit"]))
    path = os.path.join(OUT, "scan_synthetic.npz")
    np.savez_compressed(path, **out)
    man_path = os.path.join(OUT, "MANIFEST.json")
    man = json.load(open(man_path))
    man["scan_synthetic.npz"] = content_hash(path)
    with open(man_path, "w") as f:
        json.dump(dict(sorted(man.items())), f, indent=1)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
