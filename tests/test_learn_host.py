"""Host parts of the learner-ready rollouts (sigmaenv_set_rollout_obs_record, sigmaenv_mlp32_forward_rows, sigmaenv_gae; sigmarl_amd/learn.py): the ctypes mirror of
sigmaenv_gae_args_t against the header as the host C compiler lays it out, the bound entry points, and the argument refusals that happen before any device call.
No GPU needed."""
import ctypes
import os
import shutil
import subprocess
import types

import pytest
import torch

from sigmarl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("cc") is None, reason="no host C compiler")
def test_gae_args_layout_matches_the_header(tmp_path):
    fields = [f[0] for f in capi.GaeArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sigmaenv.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(sigmaenv_gae_args_t));\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(sigmaenv_gae_args_t, {f}));\n' for f in fields)
                   + '  printf("abi %d\\n", SIGMAENV_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(capi.GaeArgs)
    for f in fields:
        assert int(got[f]) == getattr(capi.GaeArgs, f).offset, f
    assert int(got["abi"]) == capi.ABI_VERSION == 5  # no existing structure changed


def test_learn_entry_points_are_bound():
    for name in ("set_rollout_obs_record", "mlp32_forward_rows", "gae"):
        assert "sigmaenv_" + name in capi.exported_symbols()
    header = open(os.path.join(ROOT, "include", "sigmaenv.h")).read()
    for name in ("set_rollout_obs_record", "mlp32_forward_rows", "gae"):
        assert f"int sigmaenv_{name}(" in header


def test_the_build_id_covers_the_new_kernels():
    mk = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "Makefile")).read()
    src = [ln for ln in mk.splitlines() if ln.startswith("SRC = ")][0].split()
    assert "sigmaenv_learn.inc" in src


def _fake_env(B=4, N=3, D=5):
    return types.SimpleNamespace(B=B, N=N, D=D, device=torch.device("cpu"), parameters=None)


def test_rollout_refuses_an_observation_record_it_cannot_write():
    """Actor.rollout(obs_rec=...) checks the record before anything is enqueued: device, dtype, shape [T, B, N, D], contiguity."""
    from sigmarl_amd.actor import Actor

    env = _fake_env()
    for bad in (torch.zeros(2, 4, 3, 5),                          # host memory
                torch.zeros(2, 4, 3, 5, dtype=torch.float64),
                torch.zeros(2, 4, 15),
                "not a tensor"):
        with pytest.raises(TypeError, match="obs_rec"):
            Actor.rollout(None, env, 2, obs_rec=bad)


def test_gae_refuses_bad_arguments():
    from sigmarl_amd import learn

    env = _fake_env()
    W = env.N * (env.D + 1) + 1
    v = torch.zeros(2, 4)
    with pytest.raises(TypeError, match="slab"):
        learn.gae(env, torch.zeros(2, 4, W), v, v, 0.99, 0.9)     # host memory
    with pytest.raises(TypeError, match="slab"):
        learn.gae(env, torch.zeros(2, 4, W + 1), v, v, 0.99, 0.9)
    with pytest.raises(TypeError, match="slab"):
        learn.gae(env, None, v, v, 0.99, 0.9)


def test_collect_makes_its_own_records():
    from sigmarl_amd import learn

    with pytest.raises(TypeError, match="slab"):
        learn.collect(_fake_env(), None, None, 2, gamma=0.99, lmbda=0.9, slab=torch.zeros(1))
    with pytest.raises(ValueError, match="gamma"):
        learn.collect(_fake_env(), None, None, 2)


def test_parameters_carry_the_reference_discounts():
    from sigmarl_amd.params import Parameters

    p = Parameters()
    assert (p.gamma, p.lmbda) == (0.99, 0.9)  # sigmarl/helper_training.py Parameters defaults, read by learn.collect
    from sigmarl_amd import learn

    assert learn.TD_GAMMA == 0.9  # mappo_cavs.py:383
