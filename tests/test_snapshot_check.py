"""The env snapshot's layout and piece arithmetic on the host (no GPU): sigmarl_amd/csrc/sigmaenv_snapshot.h compiled ALONE into a stand-alone program
(tests/host_program.py: with AddressSanitizer + UBSan where the compiler has them) against the numpy twin tests/snapshot_check.py -- the segment table, the totals, the
kernel's constants and, for every lane of the flat grid, its (segment, piece, block, env, live offset, blob offset) agree number for number over six configurations;
offsets are multiples of 16, segments do not overlap, every SIGMAENV_BUF_* id is present, the grid touches every byte of every segment exactly once; a configuration
past the multiplier division's range divides plainly and still agrees; save / restore / masked restore over plain arrays; every defect planted in the twin fails a
named check; the header, the ctypes mirror and the entry points against include/sigmaenv.h and the build id's source list."""
import ctypes
import os
import struct

import numpy as np
import pytest

import host_program
import snapshot_check as sc
from sigmarl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = capi.N_SHORT_TERM


def shape(B, N, K, flags, cbf, ns=NS):
    return (B, N, K, capi.obs_dim(K, flags, ns, N), ns, flags, cbf)


# (B, N, K, D, NS, obs_flags, cbf): default, OBS_FULL | BIRD_VIEW, BOUNDARY_POINTS, opponent pad, CBF attached (with groups; and without: no segment more), N = 64
CONFIGS = {
    "default": shape(130, 4, 2, 0, sc.CBF_NONE),
    "full_bird_view": shape(6, 4, 2, capi.OBS_FULL | capi.OBS_BIRD_VIEW, sc.CBF_NONE),
    "boundary_points": shape(5, 3, 2, capi.OBS_BOUNDARY_POINTS, sc.CBF_NONE),
    "opponent_pad": shape(7, 16, 2, capi.OBS_OPPONENT_PAD, sc.CBF_NONE, 5),
    "cbf_attached": shape(6, 4, 2, 0, sc.CBF_GROUPED),
    "n64": shape(2, 64, 2, 0, sc.CBF_ATTACHED),
}
# past x * d < 2^32: SIGMAENV_BUF_OBS has N * D / 4 pieces per env (D > 5000 in the full view of 64 agents), times 4096 envs -- sampled, not enumerated
BIG = shape(4096, 64, 4, capi.OBS_FULL | capi.OBS_BIRD_VIEW | capi.OBS_REF_OTHERS, sc.CBF_NONE)
BIG_SAMPLES = 997

PROGRAM = r"""
#define SIGMA_HD static inline
#include "sigmaenv_snapshot.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static void w64(FILE* f, uint64_t v) { fwrite(&v, 8, 1, f); }

int main() {
  FILE* in = fopen("%(inp)s", "rb");
  FILE* out = fopen("%(out)s", "wb");
  if (!in || !out) return 3;
  int32_t n_cases = 0;
  if (fread(&n_cases, 4, 1, in) != 1) return 2;
  for (int c = 0; c < n_cases; ++c) {
    int32_t d[8];  // B, N, K, D, NS, obs_flags, cbf, samples (0: every lane of the grid)
    if (fread(d, 4, 8, in) != 8) return 2;
    SnapLayout L;
    SnapTable T;
    snap_layout(d[0], d[1], d[2], d[3], d[4], d[5], d[6], &L);
    if (snap_table(L, d[0], &T) != 0) return 4;
    w64(out, (uint64_t)L.n); w64(out, L.total); w64(out, T.wg_first[T.n]);
    for (int s = 0; s < L.n; ++s) {
      const SnapSegment& g = L.seg[s];
      const uint64_t row[14] = {(uint64_t)g.id, (uint64_t)g.elem, g.w, (uint64_t)g.blocks, g.block_stride, g.offset, T.piece[s], T.ppe[s], T.ppb[s], T.pieces[s], T.m_ppe[s],
                                T.m_ppb[s], T.wg_first[s], snap_padding(T, s)};
      fwrite(row, 8, 14, out);
    }
    if (d[7] == 0) {  // the kernel's walk: every workgroup, every lane
      for (uint32_t wg = 0; wg < T.wg_first[T.n]; ++wg) {
        const int s = snap_segment_of(T, wg);
        for (uint32_t lane = 0; lane < SNAP_BLOCK; ++lane) {
          const uint32_t q = (wg - T.wg_first[s]) * SNAP_BLOCK + lane;
          if (q >= T.pieces[s]) continue;
          const SnapPiece p = snap_locate(T, s, q);
          const uint64_t row[6] = {(uint64_t)s, q, p.block, p.env, p.live_off, p.blob_off};
          fwrite(row, 8, 6, out);
        }
      }
    } else {
      for (int s = 0; s < L.n; ++s) {
        const uint32_t step = T.pieces[s] / (uint32_t)d[7] + 1u;
        for (uint64_t q = 0; q < T.pieces[s]; q += step) {
          const SnapPiece p = snap_locate(T, s, (uint32_t)q);
          const uint64_t row[6] = {(uint64_t)s, q, p.block, p.env, p.live_off, p.blob_off};
          fwrite(row, 8, 6, out);
        }
        const SnapPiece p = snap_locate(T, s, T.pieces[s] - 1u);
        const uint64_t row[6] = {(uint64_t)s, T.pieces[s] - 1u, p.block, p.env, p.live_off, p.blob_off};
        fwrite(row, 8, 6, out);
      }
    }
    w64(out, 0xFFFFFFFFFFFFFFFFull);  // end of the case
  }
  fclose(in); fclose(out);
  printf("ok %%d cases, magic %%x, version %%u, block %%d, max segments %%d, table %%d bytes\n", (int)n_cases, (unsigned)SNAP_MAGIC, (unsigned)SNAP_VERSION, (int)SNAP_BLOCK,
         (int)SNAP_MAX_SEGMENTS, (int)sizeof(SnapTable));
  return 0;
}
"""

SEG_KEYS = ("id", "elem", "w", "blocks", "block_stride", "offset", "piece", "ppe", "ppb", "pieces", "m_ppe", "m_ppb", "wg_first", "padding")


@pytest.fixture(scope="module")
def header_results(tmp_path_factory):
    if host_program.compiler() is None:
        pytest.fail("no host C++ compiler: the header cannot be compiled alone")
    tmp = tmp_path_factory.mktemp("snapshot_header")
    cases = [(k, v, 0) for k, v in CONFIGS.items()] + [("big", BIG, BIG_SAMPLES)]
    with open(tmp / "in.bin", "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for _, shp, samples in cases:
            f.write(struct.pack("<8i", *shp, samples))
    stdout = host_program.build_and_run(tmp, "snapshot_header", PROGRAM % dict(inp=str(tmp / "in.bin"), out=str(tmp / "out.bin")))
    assert f"ok {len(cases)} cases, magic {sc.MAGIC:x}, version {sc.VERSION}, block {sc.BLOCK}, max segments 32," in stdout
    assert int(stdout.split("table ")[1].split()[0]) <= 2048  # the kernel argument
    raw = np.fromfile(tmp / "out.bin", np.uint64)
    res, at = {}, 0
    for name, _, _ in cases:
        n, total, grid = (int(x) for x in raw[at: at + 3])
        at += 3
        segs = raw[at: at + 14 * n].reshape(n, 14).astype(np.int64)
        at += 14 * n
        end = at + int(np.argmax(raw[at:] == np.uint64(0xFFFFFFFFFFFFFFFF)))
        rows = raw[at: end].reshape(-1, 6).astype(np.int64)
        at = end + 1
        res[name] = dict(total=total, grid=grid, segs=segs, rows=rows)
    assert at == raw.size
    return res


def twin_rows(shp):
    segs, total = sc.layout(*shp)
    rows, grid = sc.table(segs, shp[0])
    return segs, total, rows, grid


@pytest.mark.parametrize("name", list(CONFIGS))
def test_the_header_agrees_with_the_twin(header_results, name):
    got = header_results[name]
    segs, total, rows, grid = twin_rows(CONFIGS[name])
    assert got["total"] == total and got["grid"] == grid and len(got["segs"]) == len(segs)
    for s, (g, r) in enumerate(zip(segs, rows)):
        want = [{**g, **r, "padding": sc.padding(g, r)}[k] for k in SEG_KEYS]
        assert list(got["segs"][s]) == want, (name, s, dict(zip(SEG_KEYS, got["segs"][s])))
        end = g["offset"] + g["blocks"] * CONFIGS[name][0] * g["w"]
        assert end + sc.padding(g, r) == (segs[s + 1]["offset"] if s + 1 < len(segs) else total)  # the padding reaches exactly the next segment (or the total)
    want = np.concatenate([np.stack([np.full_like(q, s), q, b, e, lo, bo], 1) for s, (q, b, e, lo, bo) in enumerate(sc.enumerate_pieces(segs, rows, grid))])
    assert np.array_equal(got["rows"], want), name  # every lane of the grid, in grid order: segment, piece, block, env, both offsets


def test_past_the_multipliers_range_the_division_is_plain_and_agrees(header_results):
    got = header_results["big"]
    segs, total, rows, grid = twin_rows(BIG)
    assert got["total"] == total and got["grid"] == grid
    obs = [s for s, g in enumerate(segs) if g["id"] == capi.BUF_OBS][0]
    assert rows[obs]["m_ppe"] == 0 and got["segs"][obs][10] == 0  # x * d >= 2^32 here: no multiplier
    assert any(r["m_ppe"] != 0 for r in rows)
    for s in range(len(segs)):
        mine = got["rows"][got["rows"][:, 0] == s]
        b, e, lo, bo = sc.locate(segs, rows, s, mine[:, 1])
        assert np.array_equal(mine[:, 2:], np.stack([b, e, lo, bo], 1)), s
        assert mine[-1, 1] == rows[s]["pieces"] - 1


def check_layout(shp, defect=None):
    """The named checks of the layout: returns the names of the ones that fail."""
    B, N, K, D, ns, flags, cbf = shp
    segs, total = sc.layout(*shp, defect=defect)
    rows, grid = sc.table(segs, B, defect)
    failed = []
    ids = [g["id"] for g in segs]
    want_ids = list(range(sc.N_BUF)) + [sc.ID_RESET_MASK, sc.ID_RESET_FULL] + ([sc.ID_FRESH] if flags & capi.OBS_BOUNDARY_POINTS else []) + \
        ([sc.ID_CBF_GROUPS] if cbf == sc.CBF_GROUPED else [])
    if ids != want_ids:
        failed.append("ids")
    if any(g["offset"] % 16 for g in segs):
        failed.append("alignment")
    ends = [g["offset"] + g["blocks"] * B * g["w"] for g in segs]
    if any(e > nxt["offset"] for e, nxt in zip(ends, segs[1:])):
        failed.append("overlap")
    if total != sc.up16(ends[-1]) or total % 16:
        failed.append("total")
    live, blob = sc.coverage(segs, rows, grid, B, total)
    for g, cnt in zip(segs, live):
        n = g["blocks"] * B * g["w"]
        if not ((cnt[:n] == 1).all() and (cnt[n:] == 0).all()):
            failed.append("live_bytes_once")
            break
    want_blob = np.zeros_like(blob)
    for g, e in zip(segs, ends):
        want_blob[g["offset"]: e] = 1
    if not np.array_equal(blob, want_blob):
        failed.append("blob_bytes_once")
    return failed


@pytest.mark.parametrize("name", list(CONFIGS))
def test_offsets_alignment_no_overlap_totals_and_every_byte_exactly_once(name):
    assert check_layout(CONFIGS[name]) == []
    segs, _ = sc.layout(*CONFIGS[name])
    assert {g["id"] for g in segs} >= set(range(capi.BUF_COUNT if hasattr(capi, "BUF_COUNT") else 21))  # every SIGMAENV_BUF_* id
    ri = [g for g in segs if g["id"] == capi.BUF_REWARD_INFO][0]
    assert ri["blocks"] == 12 and ri["block_stride"] == CONFIGS[name][0] * CONFIGS[name][1] * 4 and all(g["blocks"] == 1 for g in segs if g is not ri)


def round_trips(shp, defect=None):
    """save on one handle, restore into one of other content; a masked restore; returns the names of the checks that fail"""
    rng = np.random.default_rng(11)
    a, b = sc.Handle(shp, rng, defect), sc.Handle(shp, rng, defect)
    B = shp[0]
    failed = []
    hdr, blob = a.save()
    if hdr["total_bytes"] != a.true_total:
        failed.append("total")
    b.restore(hdr, blob)
    if any(not np.array_equal(a.bufs[i], b.bufs[i]) for i in a.bufs):
        failed.append("whole_restore")
    if (b.observe_calls, b.cbf_groups_valid) != (a.observe_calls, a.cbf_groups_valid):
        failed.append("host_words_taken")
    c = sc.Handle(shp, rng, defect)
    c.observe_calls = a.observe_calls + 1
    before = {i: v.copy() for i, v in c.bufs.items()}
    mask = np.zeros(B, np.uint8)
    mask[[0, B - 1]] = 1
    mask[1:B - 1:3] = 1
    c.restore(hdr, blob, mask)
    on = mask != 0
    if any(not np.array_equal(c.env_bytes(i, on), a.env_bytes(i, on)) for i in a.bufs):
        failed.append("masked_envs_restored")
    keep = sc.Handle(shp, np.random.default_rng(0))
    keep.bufs = before
    if any(not np.array_equal(c.env_bytes(i, ~on), keep.env_bytes(i, ~on)) for i in a.bufs):
        failed.append("unmasked_envs_untouched")
    if c.observe_calls != a.observe_calls + 1:
        failed.append("host_words_kept_under_mask")
    return failed


@pytest.mark.parametrize("name", list(CONFIGS))
def test_save_restore_and_masked_restore_over_plain_arrays(name):
    assert round_trips(CONFIGS[name]) == []
    h = sc.Handle(CONFIGS[name], np.random.default_rng(3))
    hdr, blob = h.save()
    before = {i: v.copy() for i, v in h.bufs.items()}
    other = sc.Handle(CONFIGS[name], np.random.default_rng(4))
    theirs = {i: v.copy() for i, v in other.bufs.items()}
    other.restore(hdr, blob, np.zeros(CONFIGS[name][0], np.uint8))  # an all-zero mask changes no word
    assert all(np.array_equal(other.bufs[i], theirs[i]) for i in theirs)
    other.restore(hdr, blob, np.ones(CONFIGS[name][0], np.uint8))  # an all-ones mask is the unmasked restore
    assert all(np.array_equal(other.bufs[i], before[i]) for i in before)
    for k, v in (("n_envs", hdr["n_envs"] + 1), ("obs_flags", hdr["obs_flags"] ^ 1), ("version", 2), ("magic", 0)):
        with pytest.raises(ValueError, match=k):
            other.restore({**hdr, k: v}, blob)


def test_planted_defect_a_segment_left_out():
    assert "ids" in check_layout(CONFIGS["default"], "segment_left_out")
    assert "whole_restore" in round_trips(CONFIGS["default"], "segment_left_out") and "total" in round_trips(CONFIGS["default"], "segment_left_out")


def test_planted_defect_the_reward_info_block_stride_taken_as_n():
    assert "live_bytes_once" in check_layout(CONFIGS["default"], "reward_info_stride_n")
    assert "whole_restore" in round_trips(CONFIGS["cbf_attached"], "reward_info_stride_n")


def test_planted_defect_the_mask_indexed_by_piece():
    f = round_trips(CONFIGS["default"], "mask_by_piece")
    assert "masked_envs_restored" in f and "unmasked_envs_untouched" in f and "whole_restore" not in f


def test_planted_defect_an_odd_width_segment_rounded_down():
    f = check_layout(CONFIGS["boundary_points"], "odd_width_rounded_down")  # N = 3: u8 [B,3] `fresh` and u8 [B] `done` lose their tails
    assert "live_bytes_once" in f and "blob_bytes_once" in f
    assert "whole_restore" in round_trips(CONFIGS["boundary_points"], "odd_width_rounded_down")


def test_planted_defect_the_host_words_restored_under_a_mask():
    assert round_trips(CONFIGS["default"], "host_words_under_mask") == ["host_words_kept_under_mask"]


def test_planted_defect_an_off_by_one_total():
    assert check_layout(CONFIGS["default"], "total_off_by_one") == ["total"]
    assert "total" in round_trips(CONFIGS["default"], "total_off_by_one")


def test_the_header_the_mirror_and_the_entry_points():
    pub = open(os.path.join(ROOT, "include", "sigmaenv.h")).read()
    snap = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "sigmaenv_snapshot.h")).read()
    assert "#include <hip" not in snap and snap.count("#include") == 1 and "<stdint.h>" in snap  # plain C++, compiled alone above
    assert f"#define SIGMAENV_STATE_MAGIC 0x{sc.MAGIC:X}u" in pub and f"#define SNAP_MAGIC 0x{sc.MAGIC:X}u" in snap
    assert f"#define SIGMAENV_STATE_VERSION {sc.VERSION}u" in pub and f"#define SNAP_VERSION {sc.VERSION}u" in snap
    assert (capi.STATE_MAGIC, capi.STATE_VERSION) == (sc.MAGIC, sc.VERSION) and struct.pack("<I", sc.MAGIC) == b"SNAP"
    assert f"#define SNAP_N_BUF {capi.BUF_CBF_NOMINAL + 1}" in snap and f"SIGMAENV_BUF_COUNT = {sc.N_BUF}" in pub
    assert f"#define SNAP_OBS_BOUNDARY_POINTS {capi.OBS_BOUNDARY_POINTS} " in snap and f"#define SNAP_BUF_REWARD_INFO {capi.BUF_REWARD_INFO}" in snap
    assert "SIGMAENV_ABI_VERSION 5" in pub  # sigmaenv_config_t did not change
    # the ctypes mirror as the host compiler lays the struct out
    fields = [ln.strip() for ln in pub.split("typedef struct sigmaenv_state_header {")[1].split("} sigmaenv_state_header_t;")[0].splitlines() if ln.strip()]
    names = [n.strip().split("[")[0] for ln in fields for n in ln.split(";")[0].split(" ", 1)[1].split(",")]
    assert names == [n for n, _ in capi.StateHeader._fields_] and ctypes.sizeof(capi.StateHeader) == 64 and capi.StateHeader.total_bytes.offset == 48
    assert f"#define SIGMAENV_ISB_EPISODES {capi.ISB_EPISODES} " in pub and capi.ISB_EPISODES == 8
    for name in ("state_layout", "state_save", "state_restore"):
        assert "sigmaenv_" + name in capi.exported_symbols() and name in capi._PRODUCT_ONLY and f"int sigmaenv_{name}(" in pub, name
    mk = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "Makefile")).read()
    src = [ln for ln in mk.splitlines() if ln.startswith("SRC = ")][0].split()
    assert "sigmaenv_snapshot.h" in src and "sigmaenv_snapshot.inc" in src  # the build id covers them
    hip = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "sigmaenv.hip")).read()
    assert '#include "sigmaenv_snapshot.h"' in hip and '#include "sigmaenv_snapshot.inc"' in hip
    inc = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "sigmaenv_snapshot.inc")).read()
    assert "atomic" not in inc.split("namespace snap {")[1].split("}  // namespace snap")[0] and "__shared__" not in inc  # no atomics, no LDS
    if os.path.exists(capi.DEFAULT_LIB):
        lib = ctypes.CDLL(capi.DEFAULT_LIB)
        assert all(hasattr(lib, "sigmaenv_" + name) for name in ("state_layout", "state_save", "state_restore"))


def test_an_older_library_without_the_entry_points_still_loads(monkeypatch):
    """SIGMAENV_LIB_OLD_ABI=1: capi tolerates the missing sigmaenv_state_* as it does other late additions; SigmaEnv.snapshot is then absent, not wrong."""
    class Symbol:
        restype = argtypes = None

    class Old:  # a library that exports everything but the snapshot entry points
        def __init__(self, path):
            pass

        def __getattr__(self, k):
            if "sigmaenv_state_" in k:
                raise AttributeError(k)
            return Symbol()

    monkeypatch.setenv("SIGMAENV_LIB_OLD_ABI", "1")
    monkeypatch.setenv("SIGMAENV_LIB", __file__)
    monkeypatch.setattr(capi.C, "CDLL", Old)
    lib = capi.Library(__file__, "sigmaenv_", capi._PRODUCT_ONLY)
    assert not hasattr(lib, "state_save") and hasattr(lib, "isb_get") and hasattr(lib, "step")
    monkeypatch.delenv("SIGMAENV_LIB_OLD_ABI")
    with pytest.raises(AttributeError, match="sigmaenv_state_layout"):  # without the switch a missing entry point is an error
        capi.Library(__file__, "sigmaenv_", capi._PRODUCT_ONLY)
