"""ONE perturbed set of the vehicle, reward and threshold constants, away from the reference's defaults (test helper, no test of its own).

At the defaults many fields of ``sigmaenv_config_t`` / ``sigmaenv_cbf_config_t`` coincide (l_f == l_r, max_speed == 1, min_acc == -max_acc, both near
penalties -0.2, both collision penalties -1, three lower thresholds 0, reward_reach_goal == 1, distance_mask_agents == 5 * length), so a kernel that reads
the wrong member of a pair agrees with the oracle and with every golden bit for bit.  The set below breaks every one of these coincidences and stays
physically sensible (same sign as the default, within about +-40 % of it; the lower thresholds, 0 by default, a small fraction of their upper ones), so
vehicles still drive, collide and finish.  ``check()`` asserts the inequalities at import: a later edit cannot quietly restore a coincidence.

``AGENTS``      overrides of ``capi.AGENTS`` (the reference's ``sigmarl.constants.AGENTS``, which the golden generator patches in place)
``PARAMETERS``  overrides of ``Parameters`` (what the reference exposes: reward_progress, both near penalties, four thresholds, ttc_low / ttc_high)
``CONFIG_ONLY`` fields the reference hard-codes (reward_reach_goal, both collision penalties: +-100 / r_p_normalizer; both CBF deviation penalties;
                distance_mask_agents: 5 * length; the mtv proximity thresholds: 0 and length) -- reachable through the C ABI only, so held by the
                device-vs-oracle tests and the swap check, not by a reference golden
``UNCLAMPED``   a second value set for reward_reach_goal and the collision penalties, below 1 in magnitude, for tests that must see them in the step reward
                before its final clamp(-1, 1)
"""
import math

from sigmarl_amd import capi

AGENTS = {
    "length": 0.25, "width": 0.11, "l_f": 0.09, "l_r": 0.07, "l_wb": 0.16,
    "max_speed": 1.3, "min_speed": -0.4,
    "max_steering": 28 * math.pi / 180, "min_steering": -26 * math.pi / 180,
    "max_acc": 4.0, "min_acc": -6.0, "max_steering_rate": 1.2, "min_steering_rate": -1.9,
}
PARAMETERS = {
    "reward_progress": 0.13, "penalty_near_boundary": -0.27, "penalty_near_other_agents": -0.13,
    "threshold_near_boundary_low": 0.004, "threshold_near_boundary_high": 0.028,
    "threshold_near_other_agents_c2c_low": 0.05, "threshold_near_other_agents_c2c_high": 0.41,
    "ttc_low": 0.2, "ttc_high": 2.9,
}
CONFIG_ONLY = {
    "reward_reach_goal": 1.3, "penalty_collide_with_agents": -1.2, "penalty_collide_with_boundaries": -0.8,
    "penalty_deviate_from_cbf_vel": -0.07, "penalty_deviate_from_cbf_steer": -0.04,
    "distance_mask_agents": 0.9,
}
MTV_THRESHOLDS = {"threshold_near_other_agents_low": 0.03, "threshold_near_other_agents_high": 0.21}  # the reference: 0 and length, hard-coded
UNCLAMPED = {"reward_reach_goal": 0.6, "penalty_collide_with_agents": -0.7, "penalty_collide_with_boundaries": -0.45}

# the pairs whose two members hold one value at the defaults: name -> (field a, field b) of sigmaenv_config_t
SWAP_PAIRS = {
    "wheelbase": ("l_f", "l_r"),
    "acc_bounds": ("min_acc", "max_acc"),                    # exchanged WITH their signs: (-6, 4) -> (-4, 6)
    "steering_rate_bounds": ("min_steering_rate", "max_steering_rate"),
    "near_penalties": ("penalty_near_boundary", "penalty_near_other_agents"),
    "collision_penalties": ("penalty_collide_with_agents", "penalty_collide_with_boundaries"),
    "cbf_deviation_penalties": ("penalty_deviate_from_cbf_vel", "penalty_deviate_from_cbf_steer"),
    "low_thresholds_boundary_agents": ("threshold_near_boundary_low", "threshold_near_other_agents_low"),
    "low_thresholds_agents_ttc": ("threshold_near_other_agents_low", "ttc_low"),
}
SIGNED_BOUND_PAIRS = ("acc_bounds", "steering_rate_bounds")

_VEHICLE_FIELDS = ("length", "width", "l_f", "l_r", "max_speed", "max_steering", "min_acc", "max_acc", "min_steering_rate", "max_steering_rate")
_PARAMETER_FIELDS = {  # Parameters name -> sigmaenv_config_t field
    "reward_progress": "reward_progress", "penalty_near_boundary": "penalty_near_boundary", "penalty_near_other_agents": "penalty_near_other_agents",
    "threshold_near_boundary_low": "threshold_near_boundary_low", "threshold_near_boundary_high": "threshold_near_boundary_high",
    "ttc_low": "ttc_low", "ttc_high": "ttc_high",
}


def _is_pow2(x):
    m, _ = math.frexp(abs(float(x)))
    return m == 0.5


def check(agents=AGENTS, parameters=PARAMETERS, config_only=CONFIG_ONLY, mtv=MTV_THRESHOLDS, unclamped=UNCLAMPED):
    """Every coincidence of the default point is broken; every value keeps the default's sign and stays within +-40 % of it."""
    A, P, X, D = agents, parameters, config_only, capi.AGENTS
    assert A["l_f"] != A["l_r"] and abs(A["l_wb"] - (A["l_f"] + A["l_r"])) < 1e-12
    assert A["max_speed"] != 1.0 and not _is_pow2(A["max_speed"])
    assert A["min_acc"] != -A["max_acc"] and A["min_steering_rate"] != -A["max_steering_rate"]
    assert A["min_steering"] != -A["max_steering"] and A["min_speed"] != D["min_speed"]
    for k in ("length", "width", "max_steering"):
        assert A[k] != D[k], k
    assert X["distance_mask_agents"] != 5 * A["length"] and X["distance_mask_agents"] != 5 * D["length"]
    assert P["penalty_near_boundary"] != P["penalty_near_other_agents"]
    assert X["penalty_collide_with_agents"] != X["penalty_collide_with_boundaries"]
    assert X["penalty_deviate_from_cbf_vel"] != X["penalty_deviate_from_cbf_steer"]
    assert X["reward_reach_goal"] != 1.0 and unclamped["reward_reach_goal"] != 1.0
    assert unclamped["penalty_collide_with_agents"] != unclamped["penalty_collide_with_boundaries"]
    assert all(abs(v) < 1.0 for v in unclamped.values())
    for lows in ((P["threshold_near_boundary_low"], P["threshold_near_other_agents_c2c_low"], P["ttc_low"]),
                 (P["threshold_near_boundary_low"], mtv["threshold_near_other_agents_low"], P["ttc_low"])):
        assert all(v != 0 for v in lows) and len(set(lows)) == 3, lows
    defaults_high = {"threshold_near_boundary_high": 0.02, "threshold_near_other_agents_c2c_high": 0.3, "ttc_high": 3.75}
    for k, v in defaults_high.items():
        assert P[k] != v, k
    assert mtv["threshold_near_other_agents_high"] not in (D["length"], A["length"])
    for lo, hi in ((P["threshold_near_boundary_low"], P["threshold_near_boundary_high"]),
                   (P["threshold_near_other_agents_c2c_low"], P["threshold_near_other_agents_c2c_high"]), (P["ttc_low"], P["ttc_high"]),
                   (mtv["threshold_near_other_agents_low"], mtv["threshold_near_other_agents_high"])):
        assert 0 < lo < hi and not _is_pow2(hi - lo), (lo, hi)
    # physically sensible: the default's sign, within about +-40 % of it (the lower thresholds have no default to be near: below a fifth of their upper one)
    near = dict(D, reward_progress=0.1, penalty_near_boundary=-0.2, penalty_near_other_agents=-0.2, reward_reach_goal=1.0, penalty_collide_with_agents=-1.0,
                penalty_collide_with_boundaries=-1.0, penalty_deviate_from_cbf_vel=-0.05, penalty_deviate_from_cbf_steer=-0.05,
                distance_mask_agents=5 * D["length"], **defaults_high)
    for src in (A, P, X):
        for k, v in src.items():
            if k in near:
                assert v * near[k] > 0 and 0.58 <= v / near[k] <= 1.42, (k, v, near[k])
    assert 0.58 <= mtv["threshold_near_other_agents_high"] / D["length"] <= 1.42


check()


def apply_agents(cfg, agents, cbf_cfg=None):
    """The vehicle constants ``agents`` (a dict like ``capi.AGENTS``, possibly partial) on a ``capi.Config`` (or None) and on a CBF config (or None), with
    everything ``make_config`` / ``make_cbf_config`` DERIVE from them the way the reference does: the mtv proximity threshold (length), distance_mask_agents
    (5 * length), the covering circles of the CBF config.  This is what a reference run with ``sigmarl.constants.AGENTS`` patched computes with."""
    if cfg is not None:
        for k in _VEHICLE_FIELDS:
            if k in agents:
                setattr(cfg, k, agents[k])
        if "length" in agents:
            if cfg.distance_type == capi.DIST_MTV:
                cfg.threshold_near_other_agents_high = agents["length"]  # road_traffic.py:264-270
            cfg.distance_mask_agents = agents["length"] * 5              # road_traffic.py:663
    if cbf_cfg is not None:
        for k in ("l_r", "l_wb", "min_speed", "min_steering"):
            if k in agents:
                setattr(cbf_cfg, k, agents[k])
        if "max_steering_rate" in agents:
            cbf_cfg.steering_rate_max = float(agents["max_steering_rate"])
        A, n = dict(capi.AGENTS, **agents), int(cbf_cfg.n_circles)
        length, width = A["length"], A["width"]
        cbf_cfg.circle_radius = float(math.hypot(length / n / 2, width / 2))  # rectangle_approximation.py:53-55
        for i in range(n):
            cbf_cfg.circle_x[i] = -length / 2 + length / n / 2 + i * (length / n)  # :64-69
    return cfg


def apply(cfg, cbf_cfg=None, unclamped=False):
    """The whole perturbed set on a ``capi.Config`` made from default ``Parameters`` (and on a CBF config where one is attached): vehicle constants, the
    ``Parameters``-exposed rewards and thresholds, and the fields only the C ABI reaches."""
    apply_agents(cfg, AGENTS, cbf_cfg)
    for name, field in _PARAMETER_FIELDS.items():
        setattr(cfg, field, PARAMETERS[name])
    if cfg.distance_type == capi.DIST_MTV:
        for k, v in MTV_THRESHOLDS.items():
            setattr(cfg, k, v)
    else:
        cfg.threshold_near_other_agents_low = PARAMETERS["threshold_near_other_agents_c2c_low"]
        cfg.threshold_near_other_agents_high = PARAMETERS["threshold_near_other_agents_c2c_high"]
    for k, v in CONFIG_ONLY.items():
        setattr(cfg, k, v)
    if unclamped:
        for k, v in UNCLAMPED.items():
            setattr(cfg, k, v)
    return cfg


def copy_config(cfg):
    out = type(cfg)()
    import ctypes

    ctypes.memmove(ctypes.byref(out), ctypes.byref(cfg), ctypes.sizeof(cfg))
    return out


def swapped(cfg, pair):
    """A copy of ``cfg`` that differs only by exchanging the two values of ``SWAP_PAIRS[pair]`` (bounds: exchanged with their signs, so the box stays a box)."""
    a, b = SWAP_PAIRS[pair]
    out = copy_config(cfg)
    va, vb = getattr(cfg, a), getattr(cfg, b)
    if pair in SIGNED_BOUND_PAIRS:
        va, vb = -vb, -va
    else:
        va, vb = vb, va
    setattr(out, a, va)
    setattr(out, b, vb)
    assert getattr(out, a) != getattr(cfg, a) and getattr(out, b) != getattr(cfg, b), pair
    return out
