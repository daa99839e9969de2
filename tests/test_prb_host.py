"""Host parts of the prioritized replay buffer (sigmaenv_prb_*; learn.PrioritizedBuffer): the ctypes mirror of sigmaenv_prb_refresh_args_t against the header as the
host C compiler lays it out, the bound entry points, the build id's source list, the level sizes, and the argument refusals that happen before any device call.
No GPU needed."""
import ctypes
import os
import shutil
import subprocess
import types

import pytest
import torch

import prb_check as pc
from sigmarl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("prb_create", "prb_destroy", "prb_extend", "prb_sample", "prb_refresh", "prb_get")


def test_refresh_args_layout_and_constants_match_the_header(tmp_path):
    if shutil.which("cc") is None:
        pytest.fail("no host C compiler: the header's layout cannot be checked")
    fields = [f[0] for f in capi.PrbRefreshArgs._fields_]
    consts = {"SIGMAENV_PRB_LEAVES": capi.PRB_LEAVES, "SIGMAENV_PRB_TOTAL": capi.PRB_TOTAL, "SIGMAENV_PRB_QMIN": capi.PRB_QMIN, "SIGMAENV_PRB_LEN": capi.PRB_LEN,
              "SIGMAENV_PRB_N_LEVELS": capi.PRB_N_LEVELS, "SIGMAENV_PRB_LEVEL_SUM": capi.PRB_LEVEL_SUM, "SIGMAENV_PRB_LEVEL_MIN": capi.PRB_LEVEL_MIN}
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sigmaenv.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(sigmaenv_prb_refresh_args_t));\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(sigmaenv_prb_refresh_args_t, {f}));\n' for f in fields)
                   + "".join(f'  printf("{c} %d\\n", {c});\n' for c in consts)
                   + '  printf("abi %d\\n", SIGMAENV_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(capi.PrbRefreshArgs)
    for f in fields:
        assert int(got[f]) == getattr(capi.PrbRefreshArgs, f).offset, f
    for c, v in consts.items():
        assert int(got[c]) == v, c
    assert int(got["abi"]) == capi.ABI_VERSION == 5  # new entry points only: no existing structure changed


def test_entry_points_are_bound_and_hashed_into_the_build_id():
    header = open(os.path.join(ROOT, "include", "sigmaenv.h")).read()
    for name in NAMES:
        assert "sigmaenv_" + name in capi.exported_symbols() and name in capi._PRODUCT_ONLY and f"sigmaenv_{name}(" in header
    mk = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "Makefile")).read()
    src = [ln for ln in mk.splitlines() if ln.startswith("SRC = ")][0].split()
    assert "sigmaenv_prb.h" in src and "sigmaenv_prb.inc" in src
    lib = ctypes.CDLL(capi.DEFAULT_LIB) if os.path.exists(capi.DEFAULT_LIB) else None
    if lib is not None:
        import torch  # noqa: F401  (HIP runtime load order, see capi.load_library)

        assert all(hasattr(lib, "sigmaenv_" + n) for n in NAMES)


def test_level_sizes_and_the_draw_id():
    assert capi.prb_level_sizes(1) == [1] and capi.prb_level_sizes(256) == [256] and capi.prb_level_sizes(257) == [257, 2]
    assert capi.prb_level_sizes(65536) == [65536, 256] and capi.prb_level_sizes(65537) == [65537, 257, 2] and capi.prb_level_sizes(4096 * 128) == [524288, 2048, 8]
    assert capi.prb_level_sizes(capi.PRB_MAX_CAPACITY) == [1 << 30, 1 << 22, 1 << 14, 64]  # PRB_MAX_LEVELS = 4
    for c in (1, 255, 300, 65792):
        assert capi.prb_level_sizes(c) == pc.level_sizes(c)
    assert capi.PRB_DRAW == pc.DRAW == 7400 and capi.PRB_FAN == pc.FAN == 256
    hdr = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "sigmaenv_prb.h")).read()
    table = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "sigmaenv_dist.h")).read()  # (PRB_DRAW is the draw table's entry)
    assert "#define PRB_DRAW DRAW_REPLAY " in hdr and "#define DRAW_REPLAY 7400u" in table and "#define PRB_FAN 256" in hdr and "#define PRB_MAX_LEVELS 4" in hdr


def test_refusals_before_any_device_call():
    """the constructor's checks come before sigmaenv_prb_create: an env without a library is never reached"""
    from sigmarl_amd import learn

    env = types.SimpleNamespace(B=4, N=3, D=5, device=torch.device("cpu"))
    for bad, exc in ((dict(capacity=0), ValueError), (dict(capacity=(1 << 30) + 1), ValueError), (dict(capacity=8, alpha=1.01), ValueError),
                     (dict(capacity=8, alpha=-0.5), ValueError), (dict(capacity=8, beta=-0.1), ValueError), (dict(capacity=8, beta=float("inf")), ValueError),
                     (dict(capacity=8, eps=-1.0), ValueError)):
        with pytest.raises(exc):
            learn.PrioritizedBuffer(env, **bad)
    with pytest.raises(TypeError):
        learn.update(env, None, None, None, None, None, {"observation": torch.zeros(2, 4, 3, 5)}, num_epochs=1, minibatch_size=4, clip_epsilon=0.2, entropy_coeff=0.0,
                     max_grad_norm=1.0, buffer=object())
