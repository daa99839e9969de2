"""The renderer's picture and host parts (no GPU): sigmarl_amd/csrc/sigmaenv_render.h compiled ALONE into a stand-alone program (tests/host_program.py: with
AddressSanitizer + UBSan where the compiler has them; a program with its own main, nothing is loaded into Python under a sanitizer) and held to the float32 twin of
tests/render_check.py as bytes over the planted frames -- among them a zero-area quad, a NaN vertex, an infinite path point and coordinates whose pixel values
overflow, which draw nothing and index nothing, and 64 vehicles in one tile, whose list passes its capacity --; the twin against its three float64 checks; every
planted defect of the twin fails the check named beside it; the header, the ctypes mirrors and the build id's source list against include/sigmaenv.h; the refusals
made before any device call; the view fit and the palette formula of sigmarl_amd/render.py."""
import colorsys
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import host_program
import render_check as rc
from sigmarl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#define SIGMA_HD static inline
#include "sigmaenv_render.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static void rd(FILE* f, void* p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }

int main() {
  FILE* in = fopen("%(inp)s", "rb");
  FILE* out = fopen("%(out)s", "wb");
  if (!in || !out) return 3;
  int32_t n_cases = 0;
  rd(in, &n_cases, 4);
  for (int c = 0; c < n_cases; ++c) {
    int32_t d[10];  // N, B, W, H, S, flags, n_sel, n_paths, stride, n_st
    float f[5];     // scale, x0, y1, h_b, h_p
    rd(in, d, sizeof d);
    rd(in, f, sizeof f);
    const size_t N = d[0], B = d[1], W = d[2], H = d[3], n_sel = d[6], n_paths = d[7], stride = d[8], n_st = d[9];
    const int S = d[4], flags = d[5];
    std::vector<uint8_t> palette((3 + N) * 3), pal((4 + N) * 3), ca(B * N * N), cf(B * N * 4), bg(H * W * 3), frame(H * W * 3);
    std::vector<int32_t> sel(n_sel), n_left(n_paths), n_right(n_paths);
    std::vector<float> left(n_paths * stride * 2), right(n_paths * stride * 2), vertices(B * N * 10), st(B * N * n_st * 2), state(B * N * 8);
    std::vector<uint16_t> mask(H * W);
    rd(in, palette.data(), palette.size());
    rd(in, sel.data(), 4 * n_sel);
    rd(in, left.data(), 4 * left.size());
    rd(in, right.data(), 4 * right.size());
    rd(in, n_left.data(), 4 * n_paths);
    rd(in, n_right.data(), 4 * n_paths);
    rd(in, vertices.data(), 4 * vertices.size());
    rd(in, st.data(), 4 * st.size());
    rd(in, state.data(), 4 * state.size());
    rd(in, ca.data(), ca.size());
    rd(in, cf.data(), cf.size());
    rnd_view_t v = {f[0], f[1], f[2]};
    rnd_palette_fill(palette.data(), (int)N, pal.data());
    rnd_background(v, (int)W, (int)H, S, f[3], left.data(), right.data(), n_left.data(), n_right.data(), (int)n_paths, (int)stride, pal.data(), mask.data(), bg.data());
    fwrite(mask.data(), 2, mask.size(), out);
    fwrite(bg.data(), 1, bg.size(), out);
    std::vector<rnd_prim_t> prims(rnd_prim_count((int)N, (int)n_st, flags));
    for (size_t k = 0; k < n_sel; ++k) {
      const size_t b = sel[k];
      rnd_frame_env(v, (int)W, (int)H, S, (int)N, (int)n_st, flags, f[4], mask.data(), bg.data(), pal.data(), vertices.data() + b * N * 10, st.data() + b * N * n_st * 2,
                    state.data() + b * N * 8, ca.data() + b * N * N, cf.data() + b * N * 4, prims.data(), frame.data());
      fwrite(frame.data(), 1, frame.size(), out);
    }
  }
  fclose(in); fclose(out);
  printf("ok %%d cases, tile %%d x %%d, lane %%d, block %%d, cap %%d, max %%d, prim %%d bytes, counts %%d %%d, samples %%d%%d%%d%%d\n", (int)n_cases, RND_TILE_W, RND_TILE_H, RND_LANE_PX,
         RND_BLOCK, RND_LIST_CAP, RND_MAX_DIM, (int)sizeof(rnd_prim_t), rnd_prim_count(16, 3, 1), rnd_prim_count(16, 3, 0), rnd_samples_ok(1), rnd_samples_ok(2), rnd_samples_ok(3),
         rnd_samples_ok(4));
  return 0;
}
"""


def write_case(f, c):
    m = c["map"]
    f.write(struct.pack("<10i", c["N"], c["B"], c["W"], c["H"], c["S"], c["flags"], len(c["sel"]), m["left"].shape[0], m["left"].shape[1], c["short_term"].shape[2]))
    f.write(struct.pack("<5f", *c["view"], c["h_b"], c["h_p"]))
    for a, dt in ((c["palette"], np.uint8), (c["sel"], np.int32), (m["left"], np.float32), (m["right"], np.float32), (m["n_left"], np.int32), (m["n_right"], np.int32),
                  (c["vertices"], np.float32), (c["short_term"], np.float32), (c["state"], np.float32), (c["col_agents"], np.uint8), (c["col_flags"], np.uint8)):
        f.write(np.ascontiguousarray(a, dt).tobytes())


@pytest.fixture(scope="module")
def planted():
    assert (capi.RND_TILE_W, capi.RND_TILE_H, capi.RND_LIST_CAP) == (rc.TILE_W, rc.TILE_H, rc.LIST_CAP)  # the twin restates the library's tile walk: no library, no yardstick
    cs = rc.cases()
    return cs, {name: rc.twin(c) for name, c in cs.items()}


@pytest.fixture(scope="module")
def header_results(tmp_path_factory, planted):
    if host_program.compiler() is None:
        pytest.fail("no host C++ compiler: the header cannot be compiled alone")
    tmp = tmp_path_factory.mktemp("render_header")
    cs, _ = planted
    with open(tmp / "in.bin", "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for c in cs.values():
            write_case(f, c)
    stdout = host_program.build_and_run(tmp, "render_header", PROGRAM % dict(inp=str(tmp / "in.bin"), out=str(tmp / "out.bin")))
    assert (f"ok {len(cs)} cases, tile {rc.TILE_W} x {rc.TILE_H}, lane 4, block 256, cap {rc.LIST_CAP}, max {capi.RND_MAX_DIM}, prim 44 bytes, counts 112 32, samples 1101"
            in stdout)
    raw, at, res = open(tmp / "out.bin", "rb").read(), 0, {}
    for name, c in cs.items():
        px = c["H"] * c["W"]
        mask = np.frombuffer(raw, np.uint16, px, at).reshape(c["H"], c["W"])
        at += 2 * px
        bg = np.frombuffer(raw, np.uint8, 3 * px, at).reshape(c["H"], c["W"], 3)
        at += 3 * px
        frames = np.frombuffer(raw, np.uint8, len(c["sel"]) * 3 * px, at).reshape(len(c["sel"]), c["H"], c["W"], 3)
        at += len(c["sel"]) * 3 * px
        res[name] = dict(mask=mask, bg_rgb=bg, frames=frames)
    assert at == len(raw)
    return res


NAMES = list(rc.cases())


def test_the_cases_cover_what_they_claim(planted):
    cs, tw = planted
    assert (capi.RND_TILE_W, capi.RND_TILE_H, capi.RND_LIST_CAP) == (rc.TILE_W, rc.TILE_H, rc.LIST_CAP)
    assert (cs["one_agent"]["N"], cs["one_agent"]["B"], cs["one_agent"]["W"], cs["one_agent"]["H"], cs["one_agent"]["S"]) == (1, 1, 64, 64, 1)
    lat = cs["lattice"]
    assert (lat["N"], lat["B"], lat["sel"].tolist()) == (4, 5, [4, 0, 2, 0])
    assert (cs["edge"]["H"], cs["edge"]["W"]) == (72, 100) and cs["edge"]["W"] % 16 and cs["edge"]["H"] % rc.TILE_H  # W a multiple of 4 only; partial tiles on both edges
    assert {cs[n]["S"] for n in cs} == {1, 2, 4}
    # the capacity case: a tile's list beyond the capacity, another just below it, an empty one
    lists = rc.tile_lists(cs["capacity"], 0)
    assert max(lists.values()) > 4 * rc.LIST_CAP and any(0 < v <= rc.LIST_CAP for v in lists.values()) and min(lists.values()) == 0
    # the edge case: a vehicle listed in all four tiles around the corner (row 16, column 64), one cut by the image's edge, and what draws nothing has no box
    e = cs["edge"]
    prims = rc.env_prims(e, 0)
    P = len(prims)
    quad = {i: prims[P - 2 * e["N"] + 2 * i] for i in range(e["N"])}
    assert quad[0]["box"][0] < 64 <= quad[0]["box"][1] and quad[0]["box"][2] < 16 <= quad[0]["box"][3]
    assert quad[1]["box"][1] == e["W"] - 1 and all(quad[i] is None for i in (2, 3, 4, 6))
    assert sum(q is None for q in prims[: P - 2 * e["N"]]) >= 2 + 5  # the infinite point's two segments and disc, the overflowing path
    assert prims[P - 2 * e["N"] + 2 * 3 + 1] is not None  # the zero-area quad's mark is a dot
    # a tile with an empty list is the background, byte for byte
    for name in ("one_agent", "mean", "edge"):
        c = cs[name]
        empty = [t for t, v in rc.tile_lists(c, int(c["sel"][0])).items() if v == 0]
        assert empty
        for ty, tx in empty:
            sl = (slice(ty * rc.TILE_H, (ty + 1) * rc.TILE_H), slice(tx * rc.TILE_W, (tx + 1) * rc.TILE_W))
            assert rc.same_bytes(tw[name]["frames"][0][sl], tw[name]["bg_rgb"][sl])
    assert not rc.same_bytes(tw["lattice"]["frames"][0], tw["lattice"]["frames"][1]) and rc.same_bytes(tw["lattice"]["frames"][1], tw["lattice"]["frames"][3])
    assert not rc.same_bytes(tw["capacity"]["frames"][0], tw["capacity"]["frames"][1])  # the same vehicles in another agent order: another picture
    assert not rc.same_bytes(tw["lattice"]["frames"], tw["lattice_no_paths"]["frames"])


@pytest.mark.parametrize("name", NAMES)
def test_the_twin_holds_its_float64_checks(planted, name):
    cs, tw = planted
    c = cs[name]
    got = rc.check(tw[name]["frames"], c)
    if c.get("bracket"):
        print(name, rc.bracket(tw[name]["frames"], c))
    assert all(got.values()), got
    if name in ("one_agent", "lattice", "mean", "bracket", "lattice_no_paths"):
        assert got  # these carry a check


@pytest.mark.parametrize("name", NAMES)
def test_header_equals_the_twin_as_bytes(planted, header_results, name):
    _, tw = planted
    got = header_results[name]
    for k in ("mask", "bg_rgb", "frames"):
        assert rc.same_bytes(got[k], tw[name][k]), (name, k, int((np.asarray(got[k]) != tw[name][k]).sum()))


@pytest.mark.parametrize("defect", list(rc.DEFECTS))
def test_every_planted_defect_fails_its_named_check(planted, defect):
    cs, _ = planted
    named, failed = rc.DEFECTS[defect], set()
    for name, c in cs.items():
        got = rc.check(rc.twin(c, defect=defect)["frames"], c)
        failed |= {k for k, v in got.items() if not v}
    print(defect, named, failed)
    assert named in failed, (defect, named, failed)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_struct_layouts_and_constants_match_the_header(tmp_path):
    if shutil.which("cc") is None:
        pytest.fail("no host C compiler: the header's layout cannot be checked")
    structs = {"sigmaenv_render_args_t": capi.RenderArgs, "sigmaenv_render_src_t": capi.RenderSrc}
    body = ""
    for cname, mirror in structs.items():
        body += f'  printf("{cname} %zu\\n", sizeof({cname}));\n'
        body += "".join(f'  printf("{cname}.{f[0]} %zu\\n", offsetof({cname}, {f[0]}));\n' for f in mirror._fields_)
    body += '  printf("SHORT_TERM %d\\n", SIGMAENV_RENDER_SHORT_TERM);\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sigmaenv.h"\nint main(void) {\n' + body + '  printf("abi %d\\n", SIGMAENV_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, mirror in structs.items():
        assert int(got[cname]) == ctypes.sizeof(mirror)
        for f in mirror._fields_:
            assert int(got[f"{cname}.{f[0]}"]) == getattr(mirror, f[0]).offset, (cname, f[0])
    assert int(got["SHORT_TERM"]) == capi.RENDER_SHORT_TERM == 1
    assert int(got["abi"]) == capi.ABI_VERSION == 5  # new entry points only: no existing structure changed
    hdr = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "sigmaenv_render.h")).read()
    for name, v in (("RND_TILE_W", capi.RND_TILE_W), ("RND_TILE_H", capi.RND_TILE_H), ("RND_LIST_CAP", capi.RND_LIST_CAP), ("RND_MAX_DIM", capi.RND_MAX_DIM)):
        assert f"#define {name} {v} " in hdr or f"#define {name} {v}\n" in hdr, name
    assert "hip" not in hdr.split("#ifndef SIGMAENV_RENDER_H")[1].lower().replace("__host__ __device__", "")  # plain C++: no HIP in the code
    assert "-ffp-contract=off" in hdr and "sigma_trig_f32.h" in hdr


ENTRY_POINTS = ("render_create", "render_destroy", "render_frame", "render_attach", "render_get")


def test_the_entry_points_are_bound_and_hashed_into_the_build_id():
    header = open(os.path.join(ROOT, "include", "sigmaenv.h")).read()
    for name in ENTRY_POINTS:
        assert "sigmaenv_" + name in capi.exported_symbols() and name in capi._PRODUCT_ONLY and f" sigmaenv_{name}(" in header, name
    assert "road_traffic.py:1637-1800" in header and "road_traffic.py:1660-1800" in header  # the drawing list each entry point takes over
    mk = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "Makefile")).read()
    src = [ln for ln in mk.splitlines() if ln.startswith("SRC = ")][0].split()
    assert "sigmaenv_render.h" in src and "sigmaenv_render.inc" in src
    hip = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "sigmaenv.hip")).read()
    assert '#include "sigmaenv_render.h"' in hip and '#include "sigmaenv_render.inc"' in hip
    snap = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "sigmaenv_snapshot.h")).read()
    assert "render" not in snap.lower()  # the renderer holds no env state: nothing of it in the state layout
    if os.path.exists(capi.DEFAULT_LIB):
        lib = ctypes.CDLL(capi.DEFAULT_LIB)
        assert all(hasattr(lib, "sigmaenv_" + name) for name in ENTRY_POINTS)


# ---- the host side of sigmarl_amd/render.py -------------------------------------------------------------------------------------------------
def test_refusals_before_any_device_call():
    from sigmarl_amd import render as R

    assert R.check_image(64, 64, 1, [4, 0, 2, 0], 5).tolist() == [4, 0, 2, 0] and R.check_image(64, 64, 1, [4, 0, 2, 0], 5).dtype == np.int32
    with pytest.raises(ValueError, match="multiple of 4"):
        R.check_image(66, 64, 1, [0], 1)
    for s in (0, 3, 8):
        with pytest.raises(ValueError, match="1, 2 or 4"):
            R.check_image(64, 64, s, [0], 1)
    for sel in ([5], [-1], [0, 1, 7]):
        with pytest.raises(ValueError, match="outside"):
            R.check_image(64, 64, 1, sel, 5)
    with pytest.raises(ValueError, match="selection"):
        R.check_image(64, 64, 1, [], 5)
    assert R.render_src() is None
    s = R.render_src(vertices_ptr=4096, col_flags_ptr=8192)
    assert (s.vertices, s.short_term, s.state, s.col_agents, s.col_flags) == (4096, None, None, None, 8192) and not any(s.reserved)
    for bad in (dict(vertices_ptr=4098), dict(short_term_ptr=4097), dict(state_ptr=2), dict(col_agents_ptr=4099), dict(col_flags_ptr=0)):
        with pytest.raises(ValueError, match="null or not 4-byte aligned"):
            R.render_src(**bad)


def test_view_fit_and_default_palette():
    from sigmarl_amd import render as R

    s, x0, y1, h = R.fit_view(4.5, 4.0, 512)
    assert h == 456 and h % 4 == 0 and h >= 512 * 4.0 / 4.5  # rounded up to a multiple of 4
    assert abs((4.5 / 2 - x0) * s - 256) < 1e-3 and abs((y1 - 4.0 / 2) * s - h / 2) < 1e-3  # the map's centre is the image's centre
    assert (0 - x0) * s >= -1e-3 and (4.5 - x0) * s <= 512 + 1e-3 and (y1 - 4.0) * s >= -1e-3 and (y1 - 0) * s <= h + 1e-3  # the whole map is inside
    s2, _, _, h2 = R.fit_view(2.0, 4.0, 64, 64)
    assert h2 == 64 and abs(s2 - 16.0) < 1e-6  # the tighter axis decides
    for n in (1, 4, 16, 64):
        pal = R.default_palette(n)
        assert pal.shape == (3 + n, 3) and pal.dtype == np.uint8 and len({tuple(r) for r in pal}) == 3 + n and (0, 0, 0) not in {tuple(r) for r in pal}
        for i in (0, n - 1):
            want = [int(255 * v + 0.5) for v in colorsys.hsv_to_rgb((0.58 + i / n) % 1.0, 0.65, 0.85)]
            assert pal[3 + i].tolist() == want
