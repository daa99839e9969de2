"""The fp64 criterion of tests/network_check.py against numpy restatements of the network kernels: an fp32 forward in another summation order passes it (that
is the precision class of torch.nn in fp32, which the kernels restate), and each defect a matrix-core MLP kernel typically has fails it -- at the suite's
shapes.  Runs without a GPU; it keeps later edits of the criterion's constants honest."""
import numpy as np
import pytest
import torch

import network_check as nc

# (depth, in_dim, out_dim, rows, weight scale): the actor (D = 32, 35; the 1.7 x weights of tests/test_gpu_actor.py), the critic (16 x 32 inputs, one value),
# and shapes of the GPU sweep (tests/test_gpu_networks.py): depth 2 / 3, ragged widths and row counts
SHAPES = [
    (4, 32, 4, 256, 1.0),
    (4, 35, 4, 200, 1.7),
    (4, 512, 1, 77, 1.0),
    (2, 17, 32, 65, 1.0),
    (3, 257, 5, 31, 1.7),
]
# one output value: the criterion must not fail an fp32 forward there (the B term), but a single value cannot tell a 1e-5 tanh error from fp32 rounding noise
ONE_VALUE = [(2, 1, 1, 1, 1.0), (4, 1024, 1, 1, 1.0), (3, 4096, 1, 1, 1.0)]


def _net(depth, in_dim, out_dim, scale, seed):
    torch.manual_seed(seed)
    dims = [in_dim] + [256] * (depth - 1) + [out_dim]
    layers = []
    for a, b in zip(dims[:-1], dims[1:]):
        layers += [torch.nn.Linear(a, b), torch.nn.Tanh()]
    mlp = torch.nn.Sequential(*layers[:-1])
    with torch.no_grad():
        for m in mlp:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(scale)
                m.bias.uniform_(-0.3, 0.3)
    return mlp


def _case(depth, in_dim, out_dim, rows, scale, seed=0):
    mlp = _net(depth, in_dim, out_dim, scale, seed)
    g = np.random.default_rng(seed)
    x = (g.random((rows, in_dim), dtype=np.float32) * 2 - 1) * 1.5
    ws = [m.weight.detach().numpy().astype(np.float32) for m in mlp if isinstance(m, torch.nn.Linear)]
    bs = [m.bias.detach().numpy().astype(np.float32) for m in mlp if isinstance(m, torch.nn.Linear)]
    return mlp, x, ws, bs


# ---- numpy restatements: layer(x [rows, K] fp32, w [F, K], b [F], l) -> fp32 [rows, F]; act(y fp32) -> fp32 -------------------------------------
def _fma_chain(order):
    """an fp32 fma chain over k in the given order (one rounding per step: the exact product, exact in fp64, is added and rounded to fp32)"""
    def layer(x, w, b, l):
        acc = np.broadcast_to(b, (x.shape[0], w.shape[0])).astype(np.float32)
        x64, w64 = x.astype(np.float64), w.astype(np.float64)
        for k in order(x.shape[1]):
            acc = (acc + x64[:, k:k + 1] * w64[:, k][None, :]).astype(np.float32)
        return acc
    return layer


def _blocked16(x, w, b, l):
    """k in blocks of 16, each block summed exactly and rounded once (what v_mfma_f32_32x32x16_f16 does with its 16 products), the blocks added in fp32"""
    acc = np.broadcast_to(b, (x.shape[0], w.shape[0])).astype(np.float32)
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    for k0 in range(0, x.shape[1], 16):
        acc = (acc + (x64[:, k0:k0 + 16] @ w64[:, k0:k0 + 16].T).astype(np.float32)).astype(np.float32)
    return acc


def _exact(x, w, b, l):
    return (x.astype(np.float64) @ w.astype(np.float64).T + b).astype(np.float32)


def _split(x, w, b, l, drop_wlo_xhi=False):
    """the split-fp16 product of sigmaenv_mlp32s.inc: inputs x 2^4 (hidden activations x 2^8), weights x 2^8, each as hi + lo fp16; w_lo x_lo dropped"""
    sx, sw = (16.0 if l == 0 else 256.0), 256.0
    xs, ws = x * np.float32(sx), w * np.float32(sw)
    xh = xs.astype(np.float16).astype(np.float64)
    xl = (xs - xh.astype(np.float32)).astype(np.float16).astype(np.float64)
    wh = ws.astype(np.float16).astype(np.float64)
    wl = (ws - wh.astype(np.float32)).astype(np.float16).astype(np.float64)
    y = xh @ wh.T + xl @ wh.T + (0.0 if drop_wlo_xhi else xh @ wl.T)
    return (y / (sx * sw) + b).astype(np.float32)


def _tanh(y):
    return np.tanh(y).astype(np.float32)


def _forward(ws, bs, x, layer=_exact, act=_tanh, x_in=None):
    h = (x_in or (lambda v: v))(x.astype(np.float32))
    for l, (w, b) in enumerate(zip(ws, bs)):
        h = layer(h, w, b, l)
        if l + 1 < len(ws):
            h = act(h)
    return h


def _drop_last_kblock(x, w, b, l):
    """layer 0 without its last k block of 8 (a ragged input width: the block holds the in_dim % 8 last columns)"""
    if l == 0:
        kq = (x.shape[1] - 1) // 8 * 8
        x = x.copy()
        x[:, kq:] = 0.0
    return _exact(x, w, b, l)


def _bf16_act(y):
    return nc.bf16(np.tanh(y).astype(np.float32))


def _tanh_biased(y):
    return (np.tanh(y) + 1e-5).astype(np.float32)


def _tanh_wobbly(y):
    return (np.tanh(y) + 1e-5 * np.sin(997.0 * y)).astype(np.float32)


PASS = {
    "fma chain, k reversed": dict(layer=_fma_chain(lambda K: range(K - 1, -1, -1))),
    "fma chain, k forward": dict(layer=_fma_chain(lambda K: range(K))),
    "blocks of 16": dict(layer=_blocked16),
    "split fp16, all three products": dict(layer=_split),
}
FAIL = {
    "split fp16 without w_lo x_hi": dict(layer=lambda x, w, b, l: _split(x, w, b, l, drop_wlo_xhi=True)),
    "inputs rounded to fp16": dict(x_in=lambda v: v.astype(np.float16).astype(np.float32)),
    "hidden activations rounded to bf16": dict(act=_bf16_act),
    "tanh + 1e-5": dict(act=_tanh_biased),
    "tanh +- 1e-5": dict(act=_tanh_wobbly),
}


@pytest.mark.parametrize("shape", SHAPES + ONE_VALUE, ids=[f"d{s[0]}-in{s[1]}-out{s[2]}-r{s[3]}" for s in SHAPES + ONE_VALUE])
def test_fp32_restatements_pass(shape):
    for seed in range(3):
        mlp, x, ws, bs = _case(*shape, seed=seed)
        refs = nc.references(mlp, x)
        for name, kw in PASS.items():
            r = nc.measure(_forward(ws, bs, x, **kw), *refs)
            assert r["ok"], (name, seed, r)


@pytest.mark.parametrize("shape", SHAPES, ids=[f"d{s[0]}-in{s[1]}-out{s[2]}-r{s[3]}" for s in SHAPES])
def test_defects_fail(shape):
    for seed in range(3):
        mlp, x, ws, bs = _case(*shape, seed=seed)
        refs = nc.references(mlp, x)
        for name, kw in FAIL.items():
            r = nc.measure(_forward(ws, bs, x, **kw), *refs)
            assert not r["ok"], (name, seed, r)


@pytest.mark.parametrize("shape", [s for s in SHAPES + ONE_VALUE if s[1] % 8], ids=[f"d{s[0]}-in{s[1]}-r{s[3]}" for s in SHAPES + ONE_VALUE if s[1] % 8])
def test_a_dropped_last_k_block_fails(shape):
    mlp, x, ws, bs = _case(*shape)
    refs = nc.references(mlp, x)
    r = nc.measure(_forward(ws, bs, x, layer=_drop_last_kblock), *refs)
    assert not r["ok"], r


def test_check_accepts_torch_outputs_and_rejects_nan():
    mlp, x, ws, bs = _case(3, 9, 3, 40, 1.0)
    with torch.no_grad():
        got = mlp(torch.from_numpy(x))
    nc.check(got, mlp, torch.from_numpy(x), "torch fp32 itself")
    got[3, 1] = float("nan")
    with pytest.raises(AssertionError):
        nc.check(got, mlp, x, "a NaN")


def test_bf16_restatement_rounds_to_nearest_even():
    v = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -2.5, 1.0 + 2.0 ** -9], np.float32)
    assert nc.bf16(v).tolist() == [1.0, 1.0, 1.0 + 2 * 2.0 ** -7, -2.5, 1.0]
