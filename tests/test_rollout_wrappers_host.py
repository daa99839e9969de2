"""Host parts of the rollout wrappers (sigmaenv_rollout_f32_ex): the ctypes mirror of sigmaenv_rollout_opts_t against the header as the host C compiler lays it
out, the Parameters -> wrapper choice of the training collector, and the refusal of what the device rollout does not build.  No GPU needed."""
import ctypes
import os
import shutil
import subprocess

import pytest

from sigmarl_amd import capi
from sigmarl_amd.params import Parameters, check_rollout_wrapper, rollout_wrapper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("cc") is None, reason="no host C compiler")
def test_rollout_opts_layout_matches_the_header(tmp_path):
    fields = [f[0] for f in capi.RolloutOpts._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sigmaenv.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(sigmaenv_rollout_opts_t));\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(sigmaenv_rollout_opts_t, {f}));\n' for f in fields)
                   + '  printf("WRAP %d %d %d\\n", SIGMAENV_WRAP_PLAIN, SIGMAENV_WRAP_OPPONENT, SIGMAENV_WRAP_PRIORITIZED);\n'
                   '  printf("PRIORITY %d %d %d\\n", SIGMAENV_PRIORITY_NET, SIGMAENV_PRIORITY_RANDOM, SIGMAENV_PRIORITY_GIVEN);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(capi.RolloutOpts)
    for f in fields:
        assert int(got[f]) == getattr(capi.RolloutOpts, f).offset, f
    assert got["WRAP"].split() == [str(v) for v in (capi.WRAP_PLAIN, capi.WRAP_OPPONENT, capi.WRAP_PRIORITIZED)]
    assert got["PRIORITY"].split() == [str(v) for v in (capi.PRIORITY_NET, capi.PRIORITY_RANDOM, capi.PRIORITY_GIVEN)]


def test_rollout_entry_points_are_bound():
    for name in ("rollout_f32_ex", "priority_forward", "priority_rank", "priority_random"):
        assert "sigmaenv_" + name in capi.exported_symbols()


@pytest.mark.parametrize("flags,want", [
    (dict(), None),
    (dict(is_using_opponent_modeling=True), "opponent"),
    (dict(is_using_prioritized_marl=True), "prioritized"),
    (dict(is_using_opponent_modeling=True, is_using_prioritized_marl=True), "opponent"),  # the training collector's elif order (helper_training.py:708-740)
    (dict(is_using_cbf_training=True, is_using_opponent_modeling=True, is_using_prioritized_marl=True), None),  # CBF training first
])
def test_wrapper_follows_the_training_collector(flags, want):
    assert rollout_wrapper(Parameters(**flags)) == want


def test_communication_noise_is_refused_for_prioritized():
    p = Parameters(is_using_prioritized_marl=True, is_communication_noise=True)
    with pytest.raises(NotImplementedError):
        check_rollout_wrapper(p, "prioritized")
    check_rollout_wrapper(p, "opponent")  # (noise on the propagated actions belongs to prioritized propagation only)
    check_rollout_wrapper(Parameters(is_using_prioritized_marl=True), "prioritized")
    check_rollout_wrapper(None, "prioritized")
    with pytest.raises(ValueError):
        check_rollout_wrapper(p, "cbf")
