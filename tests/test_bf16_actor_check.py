"""tests/bf16_actor_check.py on the host: the figures of its construction, a float32 twin of sigmaenv_actor_kernel that equals the float64 restatement bit for bit on
every certified row in two summation orders and with its hardware functions pushed an ulp either way, eight planted defects that the criterion catches -- and what the
flat bar of the dense-network tests (max <= 2e-2, mean <= 2e-3) does with the same defects."""
import numpy as np
import pytest

import bf16_actor_check as bc
import network_check as nc
import policy_head_check as ph

WIDTHS = [8, 16, 24, 32]
ORDERS = ["sequential", "blocks"]
F32 = np.float32


# ---- the twin: the kernel's operations in float32 numpy ---------------------------------------------------------------------------------------------
def trunc_bf16(v):
    return (np.ascontiguousarray(v, F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def half_up_bf16(v):
    """round half away from zero: differs from ties-to-even exactly on a tie above an even mantissa"""
    return ((np.ascontiguousarray(v, F32).view(np.uint32) + np.uint32(0x8000)) & np.uint32(0xFFFF0000)).view(F32)


def _push(v, ulps, where):
    if not ulps:
        return v
    return np.where(where, np.nextafter(v, F32(np.inf if ulps > 0 else -np.inf)), v)


def fast_tanh32(a, exp_ulp=0, rcp_ulp=0):
    """fast_tanh of sigmaenv_actor.inc in fp32 operations, exp2 and the reciprocal correctly rounded (exp2 through float64) or pushed one ulp -- but for exp2(0)
    and rcp(2), which the assumption of bf16_actor_check takes as exact"""
    a = np.asarray(a, F32)
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        p = a * F32(2.8853900817779268)
        e = _push(np.exp2(p.astype(np.float64)).astype(F32), exp_ulp, p != 0)
        s = F32(1.0) + e
        r = _push(F32(1.0) / s, rcp_ulp, s != 2)
        return F32(1.0) - F32(2.0) * r


def matmul32(h, w, b, order):
    """b + h w^T with fp32 accumulation; "sequential": over k from the bias on; "blocks": 32 terms summed pairwise, block after block onto the bias"""
    acc = np.broadcast_to(b[None], (h.shape[0], w.shape[0])).astype(F32)
    K = h.shape[1]
    if order == "sequential":
        for k in range(K):
            acc = acc + h[:, k:k + 1] * w[None, :, k]
        return acc
    for k0 in range(0, K, 32):
        t = h[:, None, k0:k0 + 32] * w[None, :, k0:k0 + 32]
        if t.shape[-1] < 32:
            t = np.concatenate([t, np.zeros(t.shape[:2] + (32 - t.shape[-1],), F32)], -1)
        while t.shape[-1] > 1:
            t = t[..., ::2] + t[..., 1::2]
        acc = acc + t[..., 0]
    return acc


DEFECTS = ["truncated activations", "truncated inputs", "ties rounded half up", "bias 255 of layer 2 dropped", "k slots 17 and 21 of layer 3 exchanged", "tanh off by 2e-5",
           "input column 23 dropped", "last row from the previous row's input", "a layer-4 weight of output 3 negated"]


def k_slot_feature(s):
    """the input feature in k slot s = 32 kb + 8 g + j of a chained layer (sigmaenv_pack.h, load_bf16_src)"""
    kb, g, j = s >> 5, (s >> 3) & 3, s & 7
    return 16 * (2 * kb + (j >> 2)) + 4 * g + (j & 3)


def twin(net, x, order="sequential", exp_ulp=0, rcp_ulp=0, defect=None):
    """loc_scale [rows, 4] float32 as the kernel forms it: bf16 inputs / weights / activations, fp32 accumulation, fast_tanh, the fp32 softplus of the head"""
    assert defect is None or defect in DEFECTS
    wb = [(w.astype(F32), b.astype(F32)) for w, b in bc.layers(net)]
    h = {"truncated inputs": trunc_bf16, "ties rounded half up": half_up_bf16}.get(defect, nc.bf16)(x)
    if defect == "input column 23 dropped":
        h[:, 23] = 0
    if defect == "last row from the previous row's input":
        h[-1] = h[-2]
    if defect == "bias 255 of layer 2 dropped":
        assert wb[1][1][255] != 0
        wb[1][1][255] = 0
    if defect == "k slots 17 and 21 of layer 3 exchanged":
        i, j = k_slot_feature(17), k_slot_feature(21)
        assert (i, j) == (9, 25) and (wb[2][0][:, i] != wb[2][0][:, j]).any()
        wb[2][0][:, [i, j]] = wb[2][0][:, [j, i]]
    if defect == "a layer-4 weight of output 3 negated":
        k = np.flatnonzero(wb[3][0][3])[0]
        wb[3][0][3, k] *= -1
    for l, (w, b) in enumerate(wb):
        a = matmul32(h, w, b, order)
        if l == 3:
            return np.concatenate([a[:, :2], ph.scale_of(a[:, 2:], F32)], 1).astype(F32)
        t = fast_tanh32(a, exp_ulp, rcp_ulp)
        if defect == "tanh off by 2e-5":
            t = t + F32(2e-5)
        h = (trunc_bf16 if defect == "truncated activations" else nc.bf16)(t)


# ---- the construction's figures -------------------------------------------------------------------------------------------------------------------------
def test_roundings():
    """bf16_from_f64 is round-to-nearest-even (== network_check.bf16 on fp32 numbers, ties included) and rounds ONCE where the way through fp32 rounds twice;
    midpoint_distance takes the finer spacing below a power of two."""
    g = np.random.default_rng(0)
    v = np.concatenate([g.normal(0, 1, 20000), [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 - 2.0 ** -9, 1 - 3 * 2.0 ** -9, 0.0, -0.3]]).astype(F32)
    assert np.array_equal(bc.bf16_from_f64(v.astype(np.float64)), nc.bf16(v).astype(np.float64))
    assert bc.bf16_from_f64(1 + 2.0 ** -8) == 1.0 and bc.bf16_from_f64(1 + 3 * 2.0 ** -8) == 1 + 2.0 ** -6  # ties: to the even mantissa, down and up
    t = 1 + 2.0 ** -8 + 2.0 ** -30                      # just above a midpoint: fp32 makes it the midpoint, which then goes down to even
    assert bc.bf16_from_f64(t) == 1 + 2.0 ** -7 and nc.bf16(F32(t)) == 1.0
    d = bc.midpoint_distance(np.array([1.0, 1.0 - 2.0 ** -10, 1.0 + 2.0 ** -10, 0.5, 0.0, 0.75 + 2.0 ** -9]))
    assert np.array_equal(d, [2.0 ** -9, 2.0 ** -10, 2.0 ** -8 - 2.0 ** -10, 2.0 ** -10, np.inf, 0.0])


def test_fast_tanh_error_bounds_the_twin():
    """E(a) over [-12, 12]: 7.13 * 2^-24 at worst (a = -1.53), at most 4 * 2^-24 for a > 0; the fp32 evaluation with correctly rounded hardware functions, and with
    each pushed one ulp either way (then up to 1.5 ulp from the real value, more than E assumes), stays inside E and inside MARGIN * E at every one of 400000 fp32
    arguments."""
    a = np.concatenate([np.linspace(-12, 12, 300001), np.random.default_rng(1).normal(0, 0.05, 100000)]).astype(F32)
    E = bc.fast_tanh_error(a)
    worst = int(E.argmax())
    print(f"worst E = {E[worst] / bc.U:.3f} * 2^-24 at a = {a[worst]:.3f}; for a > 0: {E[a > 0].max() / bc.U:.3f} * 2^-24")
    assert 7.0 * bc.U < E[worst] < 7.2 * bc.U and -1.7 < a[worst] < -1.4
    assert E[a > 0].max() <= 4.01 * bc.U  # (4 * 2^-24 as a -> 0, plus the float64 slop)
    t = np.tanh(a.astype(np.float64))
    for eu in (-1, 0, 1):
        for ru in (-1, 0, 1):
            err = np.abs(fast_tanh32(a, eu, ru).astype(np.float64) - t)
            nz = a != 0
            worst = float((err[nz] / E[nz]).max())
            print(f"exp2 {eu:+d} ulp, rcp {ru:+d} ulp: largest error / E = {worst:.3f}")
            assert worst <= (1.0 if eu == ru == 0 else bc.MARGIN), (eu, ru, worst)
    assert fast_tanh32(F32(0.0), 1, -1) == 0.0
    # below |a| = 2^-9 the error is no longer far below the bf16 spacing of tanh(a): MARGIN * E is a sixteenth of it and more
    small = F32(2.0 ** -9)
    assert bc.MARGIN * bc.fast_tanh_error(small) / 2.0 ** -17 > 1 / 17


@pytest.mark.parametrize("D", WIDTHS)
def test_the_construction_and_its_certified_share(D):
    """The pool of 1120 rows: dyadic bf16-exact weights, inputs that round (off the tie columns) by less than 0.45 ulp, ties above mantissas of both parities; the
    exactness certificate passes (almost) every row; at least 75 % of the rows are certified."""
    c = bc.case(D)
    for w, b in bc.layers(c.net):
        assert np.array_equal(w * 8, np.rint(w * 8)) and np.array_equal(b * 8, np.rint(b * 8)) and np.abs(b).max() <= 0.5
    w1, w2, w3, w4 = (w for w, _ in bc.layers(c.net))
    assert ((w2 != 0).sum(1) == 16).all() and ((w3 != 0).sum(1) == 16).all() and ((w4 != 0).sum(1) == 64).all() and ((w4 != 0).sum(0) == 1).all()
    assert np.abs(w1).max() == 1.0 and set(np.unique(np.abs(w4[w4 != 0]))) == {0.125}
    xb = nc.bf16(c.x)
    assert np.abs(xb).max() < 2 and np.array_equal(xb * 1024, np.rint(xb * 1024))
    assert (xb != c.x).mean() > 0.9                                    # the kernel's input rounding has work to do
    r = np.arange(c.x.shape[0])[:, None]
    tie = c.x[r, c.ties]
    on_tie = (tie != xb[r, c.ties]) & (np.abs(tie - trunc_bf16(tie)) == np.abs(half_up_bf16(tie) - tie))
    went_up = on_tie & (np.abs(xb[r, c.ties]) > np.abs(tie))
    assert on_tie.mean() > 0.5 and went_up.sum() > 100 and (on_tie & ~went_up).sum() > 100   # ties-to-even went both ways
    std = [float(a.std()) for a in c.ref["a"]]
    no_slack = int((c.cert["slack"] <= 1).sum())
    print(f"D = {D}: certified {c.certified.size} of {c.x.shape[0]} = {c.share:.3f}; rows failing exactness {no_slack}, least slack {c.cert['slack'].min():.3g}; "
          f"pre-activation std {np.round(std, 2)}")
    assert no_slack <= 0.01 * c.x.shape[0]
    assert all(1.0 < s < 3.0 for s in std)
    assert c.share >= bc.MIN_SHARE


def test_the_gpu_pool_holds_1120_certified_rows():
    """tests/test_gpu_bf16_actor_exact.py draws 1536 rows and runs 1120 certified ones"""
    import test_gpu_bf16_actor_exact as gpu
    for D in WIDTHS:
        assert bc.case(D, gpu.POOL).certified.size >= max(n for n, _ in gpu.ROWS)


# ---- the twin on certified rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDTHS)
def test_twin_equals_the_reference_on_every_certified_row(D):
    """Both summation orders; and in either, exp2 and rcp pushed one ulp up / down in all four combinations: the same words.  (What the uncertified rows do is printed.)"""
    c = bc.case(D)
    for order in ORDERS:
        for eu, ru in ([(0, 0)] if order == "sequential" else [(0, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)]):
            got = twin(c.net, c.x, order, eu, ru)
            r = bc.compare(got[c.certified], c, c.certified, f"twin {order} exp2 {eu:+d} ulp rcp {ru:+d} ulp")
            assert r["ok"], r["message"]
            rest = np.setdiff1d(np.arange(c.x.shape[0]), c.certified)
            differ = (got[rest, :2] != c.ref["out"][rest, :2].astype(F32)).any(1).sum()
            print(f"D = {D} {order} {eu:+d} {ru:+d}: {r['rows']} certified rows equal; {differ} of the {rest.size} uncertified rows differ in loc")


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defect_fails(defect):
    """Each defect, planted in the twin where it would sit in the kernel, fails ``compare`` on the certified rows (and the message says which rows and outputs)."""
    D = 24 if defect == "input column 23 dropped" else 32
    c = bc.case(D)
    x = c.x
    rows = c.certified
    if defect == "last row from the previous row's input":   # the last row of the launch must be a certified one
        rows = c.certified[c.certified <= c.certified[-1]]
        x = c.x[:c.certified[-1] + 1]
    got = twin(c.net, x, "blocks", defect=defect)
    r = bc.compare(got[rows], c, rows, defect)
    print(r["message"][:600])
    assert not r["ok"] and r["bad"].size >= 1
    assert "certificate ratio" in r["message"] and "pool row" in r["message"]
    if defect == "a layer-4 weight of output 3 negated":
        assert r["wrong_per_output"][:3] == [0, 0, 0] and r["wrong_per_output"][3] > 0
    if defect == "last row from the previous row's input":
        assert r["bad"].tolist() == [rows[-1]]


# ---- the flat bar the dense-network tests keep ------------------------------------------------------------------------------------------------------------
def dense_case(D, R):
    """The network and the inputs of test_gpu_networks.test_bf16_actor_against_its_restatement"""
    import torch
    from sigmarl_amd.actor import make_mlp
    from test_gpu_networks import make_input
    torch.manual_seed(D)
    mlp = make_mlp(D)
    with torch.no_grad():
        for m in mlp:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(1.7)
                m.bias.uniform_(-0.3, 0.3)
    return mlp, make_input(R, D, 300 + R)


def flat_bar(got, want_raw):
    """the assertions of test_gpu_networks.py:251-253 / test_gpu_actor.py:46-48"""
    e = np.abs(got[:, :2] - want_raw[:, :2])
    return bool(e.max() <= 2e-2 and np.abs(got[:, 2:] - ph.scale_of(want_raw[:, 2:])).max() <= 2e-2 and e.mean() <= 2e-3), float(e.max()), float(e.mean())


# What the flat bar does with each defect on the dense network, per width (True: lets it through).  Found by running this test, not chosen.
FLAT_BAR_CASES = [(8, 256), (16, 257), (24, 255), (32, 257)]
FLAT_BAR_LETS_THROUGH = {"truncated activations": {8: False, 16: False, 24: False, 32: False},
                         "bias 255 of layer 2 dropped": {8: False, 16: False, 24: True, 32: False},
                         "k slots 17 and 21 of layer 3 exchanged": {8: False, 16: False, 24: False, 32: False},
                         "tanh off by 2e-5": {8: True, 16: True, 24: True, 32: True}}


@pytest.mark.parametrize("D,R", FLAT_BAR_CASES)
def test_what_the_flat_bar_lets_through(D, R):
    """The reason for the bit-exact test, as found.  On the dense network of test_gpu_networks.test_bf16_actor_against_its_restatement (weights x 1.7, the rows of that
    test) the twin WITH a defect is held to network_check.emulated_bf16 at the flat bar max <= 2e-2, mean <= 2e-3 (the sound twin: max 1.7e-4 .. 8.3e-4, mean 1.9e-6 ..
    7.4e-6).  D = 8 / 16 / 24 / 32, (max, mean) of the loc error:
      a tanh off by 2e-5            PASSES at every width: (2.6e-3, 5.9e-4) / (2.9e-3, 5.5e-4) / (3.0e-3, 5.5e-4) / (3.1e-3, 5.8e-4) -- a third of the bar;
      bias 255 of layer 2 dropped   PASSES at D = 24 (4.4e-3, 1.1e-3), fails elsewhere: (1.1e-2, 4.6e-3) / (3.6e-2, 1.7e-2) / - / (1.6e-2, 7.0e-3): it depends on the
                                    weights that happen to leave feature 255;
      truncated activations         fails, by the MEAN alone and by 8 to 18 %: (1.0e-2, 2.18e-3) / (8.3e-3, 2.26e-3) / (9.4e-3, 2.35e-3) / (8.9e-3, 2.15e-3); its maximum
                                    is half the bar;
      k slots 17 and 21 exchanged   fails clearly: max 8e-2 .. 1.3e-1 (dense weights of 0.1 differ enough from column to column).
    So the flat bar does catch a crude permutation error on dense weights, catches a truncating conversion only just, and does not see an activation function that
    is wrong in the fifth digit or -- depending on the draw -- a lost bias; on the constructed network every one of them fails ``compare`` on hundreds of rows
    (test_planted_defect_fails)."""
    mlp, x = dense_case(D, R)
    want = nc.emulated_bf16(mlp, x)
    ok, emax, emean = flat_bar(twin(mlp, x, "blocks"), want)
    print(f"D = {D}, sound twin: max {emax:.2e} mean {emean:.2e}")
    assert ok
    for defect, through in FLAT_BAR_LETS_THROUGH.items():
        ok, emax, emean = flat_bar(twin(mlp, x, "blocks", defect=defect), want)
        print(f"D = {D}, {defect}: max {emax:.2e} (bar 2e-2) mean {emean:.2e} (bar 2e-3): {'passes' if ok else 'fails'} the flat bar")
        assert ok == through[D], defect
