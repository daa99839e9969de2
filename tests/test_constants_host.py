"""CPU side of the tests away from the default constants: the swap check on the oracle alone, the shared-reciprocal division of the proximity penalty
against the plain division, and the pinned behaviour of degenerate thresholds.  The device half is tests/test_gpu_constants.py."""
import shutil
import subprocess

import numpy as np
import pytest

import constants_run as cr
import oracle_binding as ob
import perturbed_constants as pc
from sigmarl_amd import capi


def test_perturbed_set_breaks_every_coincidence():
    pc.check()
    with pytest.raises(AssertionError):  # the helper notices a restored coincidence
        pc.check(agents=dict(pc.AGENTS, l_f=pc.AGENTS["l_r"]))
    with pytest.raises(AssertionError):
        pc.check(parameters=dict(pc.PARAMETERS, ttc_low=0))
    with pytest.raises(AssertionError):
        pc.check(config_only=dict(pc.CONFIG_ONLY, distance_mask_agents=5 * pc.AGENTS["length"]))
    cfg = cr.build(cr.Case("cpm_entire", 4, 2, "distance"))[0]
    assert cfg.l_f != cfg.l_r and cfg.min_acc != -cfg.max_acc and cfg.threshold_near_other_agents_low == np.float32(0.05)
    assert set(pc.SWAP_PAIRS) == set(cr.SWAP_CASES)


@pytest.mark.parametrize("name", list(cr.SWAP_CASES) + list(cr.REPLACE_CASES))
def test_mutant_changes_the_named_buffers_on_the_oracle(name):
    """A config that differs from the perturbed one only by exchanging a coincident pair's two values (or by putting a field back to the value that is neutral /
    derived at the defaults) must change every buffer named for it: the chosen inputs reach the field -- a collision happens, a vehicle is near a boundary, a
    limit binds.  The GPU test runs the same cases on the device and holds each run to the oracle at its own config."""
    case, cfg, mut, what = cr.mutant_config(name)
    a, b = cr.oracle_run(case, cfg), cr.oracle_run(case, mut)
    n = cr.n_differing(a, b, what)
    print(name, "differing words per named buffer:", n)
    assert all(k > 0 for k in n), (name, n)
    if not case.unclamped and name != "cbf_deviation_penalties":
        r = a[capi.BUF_REWARD]
        assert (np.abs(r) < 1.0).mean() > 0.5  # the step reward does not sit on its final clamp in most entries


DIV_SRC = r"""
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
/* the device's shared-reciprocal division (sigmaenv_device.h: shared_rcp, div_shared) restated for the host.  The hardware reciprocal is accurate to 1 ulp, not
 * correctly rounded: every candidate within 1 ulp of 1 / b is tried as the seed. */
static float nudge(float x, int k) { uint32_t u; memcpy(&u, &x, 4); u += (uint32_t)k; memcpy(&x, &u, 4); return x; }
static float shared_rcp(float b, int k) { float y0 = nudge(1.0f / b, k); float e = fmaf(-b, y0, 1.0f); return fmaf(e, y0, y0); }
static float div_shared(float a, float b, float y) { float q = a * y; float r = fmaf(-b, q, a); q = fmaf(r, y, q); r = fmaf(-b, q, a); return fmaf(r, y, q); }
static float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }
int main(int argc, char** argv) {
  long bad = 0, n = 0;
  for (int s = 1; s + 1 < argc; s += 2) {
    float x0 = strtof(argv[s], 0), x1 = strtof(argv[s + 1], 0), den = x1 - x0;
    if (!(den >= 0x1p-60f && den <= 0x1p60f)) { printf("outside the guard: %a %a\n", x0, x1); return 2; }
    for (int k = -1; k <= 1; ++k) {
      float y = shared_rcp(den, k);
      for (int side = 0; side < 2; ++side) {              /* dense samples around both thresholds: every float within 4096 ulps of x0 and of x1 ... */
        float c = side ? x1 : x0;
        float d = c;
        for (int i = 0; i < 4096; ++i) d = nextafterf(d, -INFINITY);
        for (int i = 0; i < 8192; ++i, d = nextafterf(d, INFINITY)) {
          float x = clampf(d, x0, x1);
          float want = 1.0f - (x - x0) / den, got = 1.0f - div_shared(x - x0, den, y);
          bad += memcmp(&want, &got, 4) != 0; ++n;
        }
      }
      for (int i = 0; i <= 4096; ++i) {                   /* ... and 4097 evenly spaced ones from below x0 to above x1 */
        float d = x0 - 0.1f * den + (1.2f * den) * (float)i / 4096.0f;
        float x = clampf(d, x0, x1);
        float want = 1.0f - (x - x0) / den, got = 1.0f - div_shared(x - x0, den, y);
        bad += memcmp(&want, &got, 4) != 0; ++n;
      }
    }
  }
  printf("%ld %ld\n", bad, n);
  return bad != 0;
}
"""


@pytest.mark.skipif(shutil.which("cc") is None, reason="no host C compiler")
def test_penalty_term_through_the_shared_reciprocal_equals_plain_division(tmp_path):
    """The proximity penalty's 1 - (x - x0) / (x1 - x0) with the division through a hoisted reciprocal (step kernel, pen_term and its unstaged twin) is bit-identical
    to the plain division the oracle uses: for the perturbed threshold sets and 300 random sets inside the kernel's 2^-60 .. 2^60 guard, on dense distance samples
    around both thresholds, with the reciprocal seed anywhere within an ulp of 1 / (x1 - x0).  (The device half: zero differing words in test_gpu_constants.py.)"""
    src, exe = tmp_path / "div.c", tmp_path / "div"
    src.write_text(DIV_SRC)
    subprocess.check_call(["cc", "-std=c99", "-O1", "-ffp-contract=off", str(src), "-o", str(exe), "-lm"])
    P, M = pc.PARAMETERS, pc.MTV_THRESHOLDS
    sets = [(P["threshold_near_other_agents_c2c_low"], P["threshold_near_other_agents_c2c_high"]), (M["threshold_near_other_agents_low"], M["threshold_near_other_agents_high"]),
            (P["threshold_near_boundary_low"], P["threshold_near_boundary_high"]), (P["ttc_low"], P["ttc_high"]), (0.0, 0.3), (0.0, 0.22)]
    rng = np.random.default_rng(3)
    for _ in range(300):
        den = float(np.float32(2.0 ** rng.uniform(-59.0, 59.0)))
        x0 = float(np.float32(den * 2.0 ** rng.uniform(-6.0, 6.0))) if rng.integers(4) else 0.0
        x1 = float(np.float32(np.float32(x0) + np.float32(den)))
        if 2.0 ** -60 <= float(np.float32(x1) - np.float32(x0)) <= 2.0 ** 60:
            sets.append((x0, x1))
    args = [repr(float(np.float32(v))) for s in sets for v in s]
    out = subprocess.run([str(exe)] + args, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    bad, n = [int(v) for v in out.stdout.split()]
    assert bad == 0 and n > 1_000_000


@pytest.mark.parametrize("which", ["near_other_agents", "near_boundary", "ttc"])
def test_degenerate_thresholds_are_pinned_on_the_oracle(which):
    """threshold_high == threshold_low (include/sigmaenv.h, next to the fields): the reference's decreasing_fcn computes (x - x0) / 0 with x clamped to x0, i.e.
    0 / 0 = NaN, for every entry.  The library keeps that arithmetic: the penalty's RewardInfo channel is NaN for every agent and the step reward, clamped with
    fmin / fmax (which drop a NaN operand), is -1.  The device must agree word for word (test_gpu_constants.py)."""
    case = cr.Case("cpm_entire", 4, 3, "ttc" if which == "ttc" else "distance", steps=3)
    rec = cr.oracle_run(case, degenerate_config(case, which))
    ri = rec[capi.BUF_REWARD_INFO]
    if which != "near_boundary":  # (the boundary penalty has no RewardInfo channel outside the CBF rewards)
        assert np.isnan(ri[:, cr.RI["rew_near_other_agents"]]).all()
    assert (rec[capi.BUF_REWARD] == -1.0).all()
    assert np.isfinite(rec[capi.BUF_STATE]).all() and np.isfinite(rec[capi.BUF_OBS]).all()


def degenerate_config(case, which):
    cfg = cr.build(case)[0]
    if which == "near_other_agents":
        cfg.threshold_near_other_agents_low = cfg.threshold_near_other_agents_high
    elif which == "near_boundary":
        cfg.threshold_near_boundary_low = cfg.threshold_near_boundary_high
    else:
        cfg.ttc_low = cfg.ttc_high
    return cfg
