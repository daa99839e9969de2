"""The fp32 network differentiated on the device (sigmaenv_mlp32_forward_save / sigmaenv_mlp32_backward, Mlp32.apply / Actor.apply / Critic.apply): every case is
held to both layers of tests/gradient_check.py -- the backward given the device's own saved activations within a derived count of roundings, the saved activations
and the gradients end to end against float64 autograd with the fp32 autograd's own error as the yardstick --, dense rows and the same rows inside a record give the
same bits, as do two runs, a loaded and a fresh handle, and the C entry point and ``loss.backward()``.  At the four row counts where the dW kernel's row partition
changes (THRESHOLDS: 16384 .. 20481 rows, what a minibatch of the workload has) the actor and the critic are held to both layers again, and -- the bound there being no
more than a third of what one lost row moves -- exactly: one-row probes whose dW / db are a single product (gc.check_one_row), an output-layer db that is an exact
sum.  Every backward of this module runs on a workspace of exactly the floats it asks for, followed by guard words (c_grad)."""
import ctypes as C

import numpy as np
import pytest

import gradient_check as gc

pytestmark = pytest.mark.gpu

LOW, HIGH = [-1.0, -0.6], [1.0, 0.6]
ACTOR, CRITIC, TWO, ODD, WIDE = [32, 256, 256, 256, 4], [512, 256, 256, 256, 1], [7, 256, 1], [35, 256, 256, 32], [600, 256, 256, 256, 1]
CROSS = 838  # partition(838) = (256, 4): three range boundaries inside, a short last range of 70 rows (asserted below)
ROWS = [0, 1, 63, 64, 65, 130, 200, CROSS]
# (the wide network is exact-only by its size; the others are asked to run split -- the mode must not matter -- and the actor in both)
NETS = [(ACTOR, "split"), (ACTOR, "exact"), (CRITIC, "split"), (TWO, "split"), (ODD, "split"), (WIDE, "split")]


def same(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def make_net(dims, seed):
    import torch

    torch.manual_seed(seed)
    layers = []
    for l in range(len(dims) - 1):
        layers += [torch.nn.Linear(dims[l], dims[l + 1])] + ([torch.nn.Tanh()] if l + 2 < len(dims) else [])
    net = torch.nn.Sequential(*layers)
    with torch.no_grad():
        for m in net:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(1.5)  # (some saturated units: 1 - a^2 small)
                m.bias.uniform_(-0.3, 0.3)
    return net


@pytest.fixture(scope="module")
def env():
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters

    e = SigmaEnv(Parameters(n_agents=4, scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False), n_envs=8, device="cuda:0")
    e.reset_random(seed=3)
    yield e
    e.close()


_nets = {}


def network(dims, mode):
    """(torch module on the CPU, Mlp32) per (dims, mode), made once."""
    from sigmarl_amd.actor import Mlp32

    key = (tuple(dims), mode)
    if key not in _nets:
        mlp = make_net(dims, 1 + len(_nets))
        _nets[key] = (mlp, Mlp32(mlp, mode=mode))
    return _nets[key]


def inputs(rows, dims, seed=11):
    rng = np.random.default_rng(seed + rows)
    x = ((rng.random((rows, dims[0])) * 2 - 1) * 1.5).astype(np.float32)
    dout = (rng.standard_normal((rows, dims[-1])) / max(rows, 1)).astype(np.float32)  # the scale of a mean loss
    if rows > 12:
        x[7] = 0.0
        dout[11] = 0.0
    return x, dout


def in_record(x):
    """The rows of ``x`` inside a record: an odd row stride, the smallest prime factor of the row count as the number of blocks with a gap between the blocks, the
    base at a storage offset of 3 floats (4-byte aligned only); everything around the rows is NaN.  Returns (tensor, (offset, rpb, row_stride, n_blocks, block_stride))."""
    import torch

    rows, K = x.shape
    nb = next((p for p in (2, 3, 5, 7) if rows % p == 0), 1) if rows > 1 else 1
    rpb = rows // nb if rows else 0
    W = K + 3 if (K + 3) % 2 else K + 4
    bstride = rpb * W + 5
    rec = torch.full((3 + nb * bstride + W,), float("nan"), dtype=torch.float32)
    for t in range(nb):
        for b in range(rpb):
            o = 3 + t * bstride + b * W
            rec[o:o + K] = torch.from_numpy(x[t * rpb + b])
    return rec.cuda(), (3, rpb, W, nb, bstride)


GUARD, GUARD_WORD = 4096, 0x5A5AA5A5  # the words after the workspace: written by no kernel


def c_grad(env, net, base, spec, dout, index=None):
    """The C entry points on rows ``spec`` of ``base`` (``index``: a CUDA int32 tensor of blocks of ``spec``'s record, the ``_indexed`` entry points): (y, acts,
    grad_w, grad_b, g); every output buffer and the workspace start as NaN.  The workspace is exactly what sigmaenv_mlp32_backward_workspace asks for, followed by
    GUARD words of a fixed pattern that must come back unchanged."""
    import torch

    offset, rpb, rs, nb, bs = spec
    n, L, lib = rpb * (nb if index is None else index.numel()), len(net._keep[1]), env.lib
    dims = [int(d) for d in net._keep[0]]
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")  # noqa: E731
    y, acts = nan(n, net.out_dim), nan(L - 1, n, 256)
    nf = C.c_uint64()
    h = net.handle(lib, env)
    assert lib.mlp32_backward_workspace(h, n, C.byref(nf)) == 0
    length, nr = gc.partition(n)
    assert nf.value == (L - 1) * n * 256 + nr * (max(dims[l] * dims[l + 1] for l in range(L)) + 256)
    ws = nan(int(nf.value) + GUARD)
    ws[int(nf.value):].view(torch.int32).fill_(GUARD_WORD)
    gw, gb = [nan(dims[l + 1], dims[l]) for l in range(L)], [nan(dims[l + 1]) for l in range(L)]
    d = torch.from_numpy(dout).cuda()
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    PA = C.c_void_p * L
    src = C.c_void_p(base.data_ptr() + 4 * offset)
    tail = (p(acts), p(d), p(ws), PA(*[t.data_ptr() for t in gw]), PA(*[t.data_ptr() for t in gb]))
    if index is None:
        rc = lib.mlp32_forward_save(env.h, h, src, rpb, rs, nb, bs, p(y), p(acts))
        assert rc == 0, lib.last_error(env.h)
        rc = lib.mlp32_backward(env.h, h, src, rpb, rs, nb, bs, *tail)
    else:
        rc = lib.mlp32_forward_save_indexed(env.h, h, src, rpb, rs, nb, bs, p(index), index.numel(), p(y), p(acts))
        assert rc == 0, lib.last_error(env.h)
        rc = lib.mlp32_backward_indexed(env.h, h, src, rpb, rs, nb, bs, p(index), index.numel(), *tail)
    assert rc == 0, lib.last_error(env.h)
    env.sync()
    assert (ws[int(nf.value):].view(torch.int32) == GUARD_WORD).all(), "the backward wrote past the workspace it asks for"
    return y, acts, gw, gb, ws[: (L - 1) * n * 256].view(L - 1, n, 256)


def test_the_crossing_row_count_crosses_the_partition_three_times():
    length, n = gc.partition(CROSS)
    assert n == 4 and 0 < CROSS - 3 * length < length and CROSS % 64 != 0


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("dims,mode", NETS, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_gradients_hold_both_layers_and_do_not_depend_on_the_row_layout(env, dims, mode, rows):
    import torch

    mlp, net = network(dims, mode)
    want = "exact" if dims[0] > 592 else mode
    assert net._mode_in_force(env.lib) == want  # (split handles stay split: the saving forward and the backward run the exact chain regardless)
    x, dout = inputs(rows, dims)
    xd = torch.from_numpy(x).cuda()
    dense = (0, rows, dims[0], 1, 0)
    y, acts, gw, gb, g = c_grad(env, net, xd, dense, dout)
    # the same bits: a second run, and the same rows inside a record
    y2, acts2, gw2, gb2, g2 = c_grad(env, net, xd, dense, dout)
    rec, spec = in_record(x)
    y3, acts3, gw3, gb3, g3 = c_grad(env, net, rec, spec, dout)
    for other in ((y2, acts2, gw2, gb2, g2), (y3, acts3, gw3, gb3, g3)):
        assert same(y, other[0]) and same(acts, other[1]) and same(g, other[4])
        assert all(same(a, b) for a, b in zip(gw + gb, other[2] + other[3]))
    assert net._mode_in_force(env.lib) == want
    if rows == 0:
        assert all((t == 0).all() and not torch.signbit(t).any() for t in gw + gb)
        return
    # y: forward_rows in EXACT mode, bit for bit
    net.set_mode("exact")
    ye = net.forward_rows(env, rec, *spec)
    env.sync()
    net.set_mode(mode)
    assert same(ye.reshape(rows, -1), y)
    cpu = lambda ts: [t.cpu().numpy() for t in ts]  # noqa: E731
    what = f"{'x'.join(map(str, dims))} {mode} rows={rows}"
    # layer 1: the backward given the device's own activations
    r1 = gc.check_backward(gc.weights_of(mlp), x, acts.cpu().numpy(), dout, cpu(gw), cpu(gb), g.cpu().numpy(), what=what)
    # layer 2: the saved activations and the gradients end to end
    gc.check_acts(acts.cpu().numpy(), mlp, x, what=what)
    r2 = gc.check_end_to_end([t for q in zip(cpu(gw), cpu(gb)) for t in q], mlp, x, dout, what=what)
    print(what, "layer 1", {k: round(v, 4) for k, v in r1["ratios"].items()}, "end to end", {k: round(v, 4) for k, v in r2["ratios"].items()})


def test_zero_dout_rows_are_as_if_absent(env):
    """Rows whose dout is zero -- scattered over tiles and ranges -- leave dW / db bit for bit what the remaining rows alone give when the removed rows are
    whole leading ranges, and within the layer-1 bound of the remaining rows' float64 gradients in general."""
    import torch

    mlp, net = network(ODD, "split")
    length, _ = gc.partition(CROSS)
    x, dout = inputs(CROSS, ODD)
    dout[:length] = 0.0   # the whole first range: its partial sums are +0
    y, acts, gw, gb, g = c_grad(env, net, torch.from_numpy(x).cuda(), (0, CROSS, ODD[0], 1, 0), dout)
    xs, ds = x[length:], dout[length:]
    assert gc.partition(len(xs))[0] == length  # (the same range length: the remaining ranges are the same chains)
    y1, acts1, gw1, gb1, g1 = c_grad(env, net, torch.from_numpy(xs).cuda(), (0, len(xs), ODD[0], 1, 0), ds)
    assert all(same(a, b) for a, b in zip(gw + gb, gw1 + gb1))
    # scattered zero rows: held to the float64 gradients of the other rows alone
    x, dout = inputs(200, ODD)
    keep = np.ones(200, bool)
    keep[[0, 5, 63, 64, 65, 127, 199]] = False
    dout[~keep] = 0.0
    y, acts, gw, gb, g = c_grad(env, net, torch.from_numpy(x).cuda(), (0, 200, ODD[0], 1, 0), dout)
    ref = gc.backward64(gc.weights_of(mlp), x[keep], acts.cpu().numpy()[:, keep], dout[keep])
    full = gc.backward64(gc.weights_of(mlp), x, acts.cpu().numpy(), dout)
    for l in range(len(gw)):
        assert gc.worst_ratio(gw[l].cpu().numpy(), ref["dW"][l], full["bound_dW"][l]) <= 1.0
        assert gc.worst_ratio(gb[l].cpu().numpy(), ref["db"][l], full["bound_db"][l]) <= 1.0
    assert (g.cpu().numpy()[:, ~keep] == 0).all()


# ---- past the partition's thresholds -------------------------------------------------------------------------------------------------
THRESHOLDS = gc.THRESHOLDS  # the four row counts at which grad::range_len changes the shape of the dW / db sums
BIG_NETS = [(ACTOR, "exact"), (CRITIC, "split")]  # (the critic's 512 inputs: four input blocks of 128 in dW_0)
BIG_IDS = dict(ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)) if isinstance(v, list) else str(v))
INDEXED = {16385: (5, 3277), 20481: (3, 6827)}    # rows = rows per block x index entries


def test_the_threshold_row_counts_are_where_the_partition_changes():
    for rows, (length, n, last) in THRESHOLDS.items():
        assert gc.partition(rows) == (length, n) and rows - (n - 1) * length == last and 0 < last <= length
    assert gc.partition(16384)[1] == gc.MAX_RANGES == gc.partition(20480)[1] and gc.partition(16384)[0] == gc.MIN_RANGE
    assert all(rpb * m == rows and rows in THRESHOLDS for rows, (rpb, m) in INDEXED.items())


def frames_record(frames, seed):
    """A record of ``frames`` blocks of ``rpb`` rows (odd row stride, a gap between the blocks, the base at a storage offset of 3 floats, NaN around the rows) and
    an index of ``m`` entries into it, not sorted and with duplicates: (record on the device, spec, index on the device, the indexed rows gathered dense [m rpb, K])"""
    import torch

    xf, m = frames
    Fr, rpb, K = xf.shape
    W = K + 3 if (K + 3) % 2 else K + 4
    bstride = rpb * W + 5
    rec = torch.full((3 + Fr * bstride + W,), float("nan"), dtype=torch.float32)
    rec[3:3 + Fr * bstride].view(Fr, bstride)[:, : rpb * W].view(Fr, rpb, W)[:, :, :K] = torch.from_numpy(xf)
    idx = np.random.default_rng(seed).integers(0, Fr, m).astype(np.int32)
    idx[-1] = idx[0]
    assert len(np.unique(idx)) < m and (np.diff(idx) < 0).any()
    return rec.cuda(), (3, rpb, W, Fr, bstride), torch.from_numpy(idx).cuda(), np.ascontiguousarray(xf[idx].reshape(m * rpb, K))


def indexed_case(rows, dims):
    """the indexed form of ``rows``: a record of 1000 frames, the index over it"""
    rpb, m = INDEXED[rows]
    xf = ((np.random.default_rng(rows).random((1000, rpb, dims[0])) * 2 - 1) * 1.5).astype(np.float32)
    return frames_record((xf, m), rows)


@pytest.mark.parametrize("rows", list(THRESHOLDS))
@pytest.mark.parametrize("dims,mode", BIG_NETS, **BIG_IDS)
def test_gradients_hold_both_layers_past_the_partition_thresholds(env, dims, mode, rows):
    """The rows inside a record (odd stride, blocks with gaps, NaN around them; outputs and workspace start as NaN, the workspace is guarded -- c_grad) against both
    layers of the criterion with its own constants, and the same bits from the dense rows."""
    import torch

    mlp, net = network(dims, mode)
    x, dout = inputs(rows, dims)
    rec, spec = in_record(x)
    y, acts, gw, gb, g = c_grad(env, net, rec, spec, dout)
    assert not any(torch.isnan(t).any() for t in gw + gb + [y, acts, g])
    other = c_grad(env, net, torch.from_numpy(x).cuda(), (0, rows, dims[0], 1, 0), dout)
    assert same(y, other[0]) and same(acts, other[1]) and same(g, other[4]) and all(same(a, b) for a, b in zip(gw + gb, other[2] + other[3]))
    cpu = lambda ts: [t.cpu().numpy() for t in ts]  # noqa: E731
    what = f"{'x'.join(map(str, dims))} {mode} rows={rows}"
    acts_h = acts.cpu().numpy()
    r1 = gc.check_backward(gc.weights_of(mlp), x, acts_h, dout, cpu(gw), cpu(gb), g.cpu().numpy(), what=what)
    gc.check_acts(acts_h, mlp, x, what=what)
    r2 = gc.check_end_to_end([t for q in zip(cpu(gw), cpu(gb)) for t in q], mlp, x, dout, what=what)
    print(what, "layer 1", {k: round(v, 4) for k, v in r1["ratios"].items()}, "end to end", {k: round(v, 4) for k, v in r2["ratios"].items()})


@pytest.mark.parametrize("rows", list(INDEXED))
@pytest.mark.parametrize("dims,mode", BIG_NETS, **BIG_IDS)
def test_indexed_entry_points_equal_the_dense_gather_past_the_thresholds(env, dims, mode, rows):
    import torch

    mlp, net = network(dims, mode)
    rec, spec, index, x = indexed_case(rows, dims)
    dout = inputs(rows, dims)[1]
    y, acts, gw, gb, g = c_grad(env, net, rec, spec, dout, index)
    assert not any(torch.isnan(t).any() for t in gw + gb + [y, acts, g])
    yd, actsd, gwd, gbd, gd = c_grad(env, net, torch.from_numpy(x).cuda(), (0, rows, dims[0], 1, 0), dout)
    assert same(y, yd) and same(acts, actsd) and same(g, gd)
    assert all(same(a, b) for a, b in zip(gw + gb, gwd + gbd))


def hold_one_row_probes(env, net, dims, x, base, spec, index, what):
    """Per probe row r: the backward of a dout that is zero but in row r (entries of magnitude about 1).  Every other row of the device's g_l is an exact zero, so
    every dW / db chain is zeros plus one term and gc.check_one_row holds each layer with == to the one product of the device's own g_l[r] and a_l[r]."""
    import torch

    rows, L = len(x), len(dims) - 1
    rng = np.random.default_rng(rows)
    small = [0] * L
    assert len(set(gc.probe_rows(rows))) == 8 and all(0 <= r < rows for r in gc.probe_rows(rows))
    for r in gc.probe_rows(rows):
        dout = np.zeros((rows, dims[-1]), np.float32)
        dout[r] = rng.uniform(0.5, 1.5, dims[-1]) * rng.choice([-1.0, 1.0], dims[-1])
        y, acts, gw, gb, g = c_grad(env, net, base, spec, dout, index)
        inside = int(torch.count_nonzero(g[:, r]))  # (a NaN left in the workspace counts as non-zero)
        assert 0 < inside == int(torch.count_nonzero(g)), f"{what} probe {r}: g is not zero outside the row"
        g_rows = list(g[:, r].cpu().numpy()) + [dout[r]]
        a_rows = [x[r]] + list(acts[:, r].cpu().numpy())
        for l in range(L):
            small[l] += gc.check_one_row(rows, g_rows[l], a_rows[l], gw[l].cpu().numpy(), gb[l].cpu().numpy(), what=f"{what} probe {r} layer {l}")
    print(what, "probes", gc.probe_rows(rows), "products below 2^-120 held to the bound, per layer:", small)
    assert small[L - 1] == 0


@pytest.mark.parametrize("rows", list(THRESHOLDS))
@pytest.mark.parametrize("dims,mode", BIG_NETS, **BIG_IDS)
def test_one_row_of_dout_is_added_once_in_its_own_range(env, dims, mode, rows):
    import torch

    mlp, net = network(dims, mode)
    x = inputs(rows, dims)[0]
    hold_one_row_probes(env, net, dims, x, torch.from_numpy(x).cuda(), (0, rows, dims[0], 1, 0), None, f"{'x'.join(map(str, dims))} rows={rows}")


@pytest.mark.parametrize("dims,mode", BIG_NETS, **BIG_IDS)
def test_one_row_of_dout_is_added_once_through_the_index(env, dims, mode):
    mlp, net = network(dims, mode)
    rec, spec, index, x = indexed_case(16385, dims)
    hold_one_row_probes(env, net, dims, x, rec, spec, index, f"{'x'.join(map(str, dims))} indexed rows=16385")


@pytest.mark.parametrize("rows", list(THRESHOLDS))
@pytest.mark.parametrize("dims,mode", BIG_NETS, **BIG_IDS)
def test_db_of_the_output_layer_is_the_exact_sum_of_a_dyadic_dout(env, dims, mode, rows):
    """dout = multiples of 2^-10 below 1 in magnitude, in every row: a column's sum of magnitudes stays below 2^14, so every partial sum in any order is a multiple
    of 2^-10 below 2^14 -- 24 bits: exact.  db of the output layer (the sum of dout over the rows) therefore equals the float64 sum."""
    import torch

    mlp, net = network(dims, mode)
    x = inputs(rows, dims)[0]
    dout = (np.random.default_rng(rows).integers(-1023, 1024, (rows, dims[-1])) / 1024.0).astype(np.float32)
    assert np.abs(dout.astype(np.float64)).sum(0).max() < 2.0 ** 14
    y, acts, gw, gb, g = c_grad(env, net, torch.from_numpy(x).cuda(), (0, rows, dims[0], 1, 0), dout)
    assert not any(torch.isnan(t).any() for t in gw + gb)
    assert np.array_equal(gb[-1].cpu().numpy().astype(np.float64), dout.astype(np.float64).sum(0))


@pytest.mark.parametrize("dims", [ACTOR, WIDE], ids=lambda v: "x".join(map(str, v)))
def test_gradients_after_load_equal_a_fresh_handle(env, dims):
    import torch
    from sigmarl_amd.actor import Mlp32

    w0, w1 = make_net(dims, 21), make_net(dims, 22)
    a, b = Mlp32(w0), Mlp32(w1)
    x, dout = inputs(130, dims)
    xd = torch.from_numpy(x).cuda()
    spec = (0, 130, dims[0], 1, 0)
    before = c_grad(env, a, xd, spec, dout)
    a.load(env, w1.cuda())
    ra, rb = c_grad(env, a, xd, spec, dout), c_grad(env, b, xd, spec, dout)
    assert same(ra[0], rb[0]) and same(ra[1], rb[1]) and same(ra[4], rb[4])
    assert all(same(p, q) for p, q in zip(ra[2] + ra[3], rb[2] + rb[3]))
    assert not same(ra[2][0], before[2][0])  # (the load had an effect)
    a.close()
    b.close()


def test_bad_arguments_are_refused_before_any_launch(env):
    import torch

    mlp, net = network(TWO, "split")
    lib, h = env.lib, net.handle(env.lib, env)
    x = torch.zeros((64, 8), device="cuda")
    y, acts, ws = torch.zeros((64, 1), device="cuda"), torch.zeros((1, 64, 256), device="cuda"), torch.zeros((1 << 16,), device="cuda")
    gw, gb = [torch.zeros((256, 7), device="cuda"), torch.zeros((1, 256), device="cuda")], [torch.zeros(256, device="cuda"), torch.zeros(1, device="cuda")]
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    PA = C.c_void_p * 2
    W, B = PA(*[t.data_ptr() for t in gw]), PA(*[t.data_ptr() for t in gb])
    EINVAL = lib.mlp32_forward_save(env.h, None, p(x), 64, 8, 1, 0, p(y), p(acts))
    assert EINVAL != 0 and b"null network" in lib.last_error(env.h)
    assert lib.mlp32_forward_save(env.h, h, p(x), 64, 6, 1, 0, p(y), p(acts)) == EINVAL        # row_stride below the input width
    assert lib.mlp32_forward_save(env.h, h, None, 64, 8, 1, 0, p(y), p(acts)) == EINVAL
    assert lib.mlp32_forward_save(env.h, h, p(x), 64, 8, 1, 0, p(y), C.c_void_p(acts.data_ptr() + 4)) == EINVAL  # acts: 16-byte alignment
    assert b"16-byte" in lib.last_error(env.h)
    assert lib.mlp32_forward_save(env.h, h, C.c_void_p(x.data_ptr() + 2), 63, 8, 1, 0, p(y), p(acts)) == EINVAL
    good = (env.h, h, p(x), 64, 8, 1, 0, p(acts), p(y), p(ws), W, B)
    assert lib.mlp32_backward(*good[:7], None, *good[8:]) == EINVAL
    assert lib.mlp32_backward(*good[:8], None, *good[9:]) == EINVAL
    assert lib.mlp32_backward(*good[:9], C.c_void_p(ws.data_ptr() + 4), *good[10:]) == EINVAL
    assert lib.mlp32_backward(*good[:10], None, B) == EINVAL
    assert lib.mlp32_backward(*good[:10], PA(gw[0].data_ptr(), None), B) == EINVAL and b"layer 1" in lib.last_error(env.h)
    assert lib.mlp32_backward(*good[:3], -1, *good[4:]) == EINVAL
    nf = C.c_uint64(5)
    assert lib.mlp32_backward_workspace(h, -1, C.byref(nf)) == EINVAL and lib.mlp32_backward_workspace(None, 4, C.byref(nf)) == EINVAL
    assert lib.mlp32_backward_workspace(h, 0, C.byref(nf)) == 0 and nf.value == 0
    # The refusal table: what each of the eight row-taking entry points returns for argument sets that are refused before any launch or have no row (then the
    # backward writes zero gradients, nothing else runs).  The codes are literals recorded from the library as it was when every entry point carried its own checks
    # (-22 = SIGMAENV_EINVAL, 0 = SIGMAENV_OK).  The network has 7 inputs; x is 2 blocks of 32 rows; padded: one segment of 5 floats read as 7 columns.
    idx = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    at = lambda t, off: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    base = dict(src=p(x), rpb=32, rs=8, nb=2, bs=256, index=p(idx), n_index=2, pad=(5, 7), out=p(y), acts=p(acts), dout=p(y), ws=p(ws))
    FWD, SAVE, BACK = ["forward_rows", "forward_rows_pad"], ["forward_save", "forward_save_indexed", "forward_save_indexed_pad"], ["backward", "backward_indexed", "backward_indexed_pad"]
    EVERY = FWD + SAVE + BACK
    INDEXED, PADDED = [n for n in EVERY if "indexed" in n], [n for n in EVERY if n.endswith("_pad")]
    PLAIN = [n for n in EVERY if n not in PADDED]

    def call(name, **over):
        a = dict(base, **over)
        rows, ix, back = (a["src"], a["rpb"], a["rs"], a["nb"], a["bs"]), (a["index"], a["n_index"]), (a["acts"], a["dout"], a["ws"], W, B)
        args = {"forward_rows": rows + (a["out"],), "forward_rows_pad": rows + a["pad"] + (a["out"],), "forward_save": rows + (a["out"], a["acts"]),
                "forward_save_indexed": rows + ix + (a["out"], a["acts"]), "forward_save_indexed_pad": rows + ix + a["pad"] + (a["out"], a["acts"]),
                "backward": rows + back, "backward_indexed": rows + ix + back, "backward_indexed_pad": rows + ix + a["pad"] + back}[name]
        return getattr(lib, "mlp32_" + name)(env.h, h, *args)

    table = [  # (the argument set, what differs from `base`, the entry points it applies to, the recorded code)
        ("null in", dict(src=None), EVERY, -22),
        ("null out", dict(out=None), FWD + SAVE, -22),
        ("null acts", dict(acts=None), SAVE + BACK, -22),
        ("acts 4-byte aligned", dict(acts=at(acts, 4)), SAVE + BACK, -22),
        ("workspace 4-byte aligned", dict(ws=at(ws, 4)), BACK, -22),
        ("row_stride one below the width", dict(rs=6), PLAIN, -22),
        ("row_stride one below the padded row's width", dict(rs=4), PADDED, -22),
        ("negative rows_per_block", dict(rpb=-1), EVERY, -22),
        ("negative n_blocks", dict(nb=-1), EVERY, -22),
        ("negative n_index", dict(n_index=-1), INDEXED, -22),
        ("2^31 rows", dict(rpb=65536, nb=32768, n_index=32768), EVERY, -22),
        ("negative block_stride, two blocks", dict(bs=-8), EVERY, -22),
        ("null index, n_index 2", dict(index=None), INDEXED, -22),
        ("seg_src above seg_dst", dict(pad=(8, 7)), PADDED, -22),
        ("seg_dst does not divide the input width", dict(pad=(3, 4)), PADDED, -22),
        ("no rows: rows_per_block 0", dict(rpb=0), EVERY, 0),
        ("no rows: n_blocks 0", dict(nb=0), [n for n in EVERY if n not in INDEXED], 0),
        ("no rows: n_index 0", dict(n_index=0), INDEXED, 0),
        ("no rows: null index, n_index 0", dict(index=None, n_index=0), INDEXED, 0),
        ("no rows and a null in", dict(rpb=0, src=None), FWD, -22),
        ("no rows and a null in", dict(rpb=0, src=None), SAVE + BACK, 0),
        ("no rows: null index, n_index 0, null in", dict(index=None, n_index=0, src=None), INDEXED, 0),
    ]
    wrong = []
    for label, over, names, code in table:
        for name in names:
            rc = call(name, **over)
            print(f"{label:45s} {name:26s} {rc}")
            if rc != code:
                wrong.append((label, name, rc, code))
            if "row_stride" in label and not lib.last_error(env.h).startswith(b"mlp32_" + name.encode() + b":"):
                wrong.append((label, name, lib.last_error(env.h), "the entry point's name in front of the message"))
    assert not wrong, wrong
    env.sync()
    assert all((t == 0).all() for t in gw + gb + [y])  # nothing ran


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def ppo_loss(torch, out, action, old_logp, adv):
    """The PPO head on the actor's four outputs per row: Normal(loc, softplus scale) log-probability of the recorded pre-squash action, ratio, clip, entropy."""
    loc, scale = out[..., :2], torch.nn.functional.softplus(out[..., 2:] + 0.54) + 1e-4
    dist = torch.distributions.Normal(loc, scale)
    ratio = torch.exp(dist.log_prob(action).sum(-1) - old_logp)
    return -torch.min(ratio * adv, ratio.clamp(0.8, 1.2) * adv).mean() - 0.01 * dist.entropy().sum(-1).mean()


@pytest.mark.parametrize("which", ["actor", "critic"])
def test_apply_fills_the_modules_grads_with_the_c_entry_points_bits(env, which):
    import torch
    from sigmarl_amd.actor import Actor, Critic

    rows = 200
    rng = np.random.default_rng(3)
    if which == "actor":
        mlp = make_net(ACTOR, 31).cuda()
        net = Actor(mlp, low=LOW, high=HIGH)
        m32, dims = net._mlp32, ACTOR
        action = torch.from_numpy(rng.standard_normal((rows, 2)).astype(np.float32)).cuda()
        old, adv = torch.from_numpy(rng.standard_normal(rows).astype(np.float32) - 2).cuda(), torch.from_numpy(rng.standard_normal(rows).astype(np.float32)).cuda()
        loss_of = lambda out: ppo_loss(torch, out, action, old, adv)  # noqa: E731
    else:
        mlp = make_net([env.N * env.D, 256, 256, 256, 1], 32).cuda()
        net = m32 = Critic(mlp)
        dims = [env.N * env.D, 256, 256, 256, 1]
        target = torch.from_numpy(rng.standard_normal((rows, 1)).astype(np.float32)).cuda()
        loss_of = lambda out: torch.nn.functional.smooth_l1_loss(out, target)  # noqa: E731
    x, _ = inputs(rows, dims)
    xd = torch.from_numpy(x).cuda()
    out = net.apply(env, xd) if which == "actor" else Mlp32_apply(net, env, xd)
    assert out.grad_fn is not None and tuple(out.shape) == (rows, dims[-1])
    loss = loss_of(out)
    loss.backward()
    torch.cuda.synchronize()
    params = [t for m in gc.linears(mlp) for t in (m.weight, m.bias)]
    assert all(t.grad is not None and torch.isfinite(t.grad).all() for t in params)
    # the same dout through the C entry points
    leaf = out.detach().clone().requires_grad_()
    loss_of(leaf).backward()
    y, acts, gw, gb, g = c_grad(env, m32, xd, (0, rows, dims[0], 1, 0), leaf.grad.cpu().numpy())
    assert same(y, out.detach())
    assert all(same(t.grad, ref) for t, ref in zip(params, [t for q in zip(gw, gb) for t in q]))
    # clip_grad_norm_ and Adam work unchanged; the optimiser's step makes the device weights stale until load
    torch.nn.utils.clip_grad_norm_(mlp.parameters(), 0.5)
    opt = torch.optim.Adam(mlp.parameters(), lr=1e-3)
    opt.step()
    with pytest.raises(RuntimeError, match="load"):
        net.apply(env, xd) if which == "actor" else Mlp32_apply(net, env, xd)
    net.load(env, mlp)
    out2 = net.apply(env, xd) if which == "actor" else Mlp32_apply(net, env, xd)
    torch.cuda.synchronize()
    assert not same(out2.detach(), out.detach())
    with pytest.raises(NotImplementedError):
        net.apply(env, xd.clone().requires_grad_()) if which == "actor" else Mlp32_apply(net, env, xd.clone().requires_grad_())
    net.close()


def Mlp32_apply(net, env, x):
    """``Mlp32.apply`` of a ``Critic`` (whose own ``apply`` takes record rows)."""
    from sigmarl_amd.actor import Mlp32

    return Mlp32.apply(net, env, x)


def test_critic_apply_reads_record_rows_in_place(env):
    """Critic.apply on the time slices [1, 3) of a [T, Bt, W] slab and of an obs_rec, for an env shard at env_first: the values of Mlp32.apply on the rows copied dense,
    bit for bit, and the same gradients."""
    import torch
    from sigmarl_amd.actor import Critic

    N, D, B = env.N, env.D, env.B
    W, Bt, T, e0 = N * (D + 1) + 1, B + 3, 4, 2
    mlp = make_net([N * D, 256, 256, 256, 1], 41).cuda()
    critic = Critic(mlp)
    g = torch.Generator().manual_seed(5)
    for rec in (torch.rand((T, Bt, W), generator=g).cuda(), torch.rand((T, Bt, N, D), generator=g).cuda()):
        v = critic.apply(env, rec, T=2, env_first=e0, t_first=1)
        assert tuple(v.shape) == (2, B) and v.grad_fn is not None
        (v * v).sum().backward()
        grads = [p.grad.clone() for p in mlp.parameters()]
        mlp.zero_grad()
        dense = rec.reshape(T, Bt, -1)[1:3, e0:e0 + B, : N * D].reshape(2 * B, N * D).contiguous()
        vd = Mlp32_apply(critic, env, dense)
        (vd * vd).sum().backward()
        torch.cuda.synchronize()
        assert same(v.detach().reshape(-1), vd.detach().reshape(-1))
        assert all(same(a, p.grad) for a, p in zip(grads, mlp.parameters()))
        mlp.zero_grad()
    critic.close()


def test_collect_update_load_collect_loop():
    """16 agents x 8 envs, T = 4: collect -> two updates (PPO head on Actor.apply over the recorded observations read in place, smooth-L1 on Critic.apply) ->
    load -> collect, with finite losses."""
    import torch
    from sigmarl_amd import learn
    from sigmarl_amd.actor import Actor, Critic, make_mlp
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters

    e = SigmaEnv(Parameters(n_agents=16, scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False, max_steps=6), n_envs=8,
                 device="cuda:0")
    e.reset_random(seed=3)
    torch.manual_seed(1)
    amod, cmod = make_mlp(e.D).cuda(), make_mlp(e.N * e.D, n_out=1).cuda()
    actor, critic = Actor(amod, low=LOW, high=HIGH), Critic(cmod)
    opt = torch.optim.Adam(list(amod.parameters()) + list(cmod.parameters()), lr=3e-4)
    T, B, N, D = 4, e.B, e.N, e.D
    torch.cuda.synchronize()
    batch = learn.collect(e, actor, critic, T, gamma=0.99, lmbda=0.9, seed=5, counter0=0)
    e.sync()
    losses = []
    obs_rows = (batch["observation"], 0, T * B * N, D, 1, 0)
    act = torch.atanh((batch["action"] / torch.tensor(HIGH, device="cuda")).clamp(-0.999, 0.999))  # the pre-squash action of this test's head
    adv = batch["advantage"]
    adv = (adv - adv.mean()) / (adv.std() + 1e-6)
    with torch.no_grad():  # the old log-probability under the same head (ratio 1 at the first update)
        o = actor.apply(e, rows=obs_rows).view(T, B, N, 4)
        old = torch.distributions.Normal(o[..., :2], torch.nn.functional.softplus(o[..., 2:] + 0.54) + 1e-4).log_prob(act).sum(-1)
    for _ in range(2):
        out = actor.apply(e, rows=obs_rows).view(T, B, N, 4)
        la = ppo_loss(torch, out, act, old, adv)
        v = critic.apply(e, batch["observation"], T=T)
        lc = torch.nn.functional.smooth_l1_loss(v.unsqueeze(-1).expand(T, B, N), batch["value_target"])
        loss = la + lc
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(amod.parameters()) + list(cmod.parameters()), 1.0)
        opt.step()
        losses.append(float(loss))
        with pytest.raises(RuntimeError, match="load"):
            actor.apply(e, rows=obs_rows)
        actor.load(e, amod)
        critic.load(e, cmod)
    batch2 = learn.collect(e, actor, critic, T, gamma=0.99, lmbda=0.9, seed=5, counter0=T)
    e.sync()
    assert all(np.isfinite(losses)) and torch.isfinite(batch2["advantage"]).all() and torch.isfinite(batch2["state_value"]).all()
    actor.close()
    critic.close()
    e.close()
