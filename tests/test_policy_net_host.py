"""The actor-critic network (sparc_amd/policy_net.py) on the host side: the ABI mirror of
``wedm_net_desc`` and the export with its refusals (no device is needed); the NumPy float32 fma against libm's ``fmaf``; the
tanh of the definition against ``np.tanh`` in float64; every product of `policy_net_reference` against the same formula in
float64 under the bound of an fma chain; the whole against ``torch.autograd`` in float64; the tree; hand-worked cases; and
the training stacks of tests/_resume_common.py with a `PolicyNet` on the CPU oracle backend, cut at every control step.

Measured here (and recorded in DESIGN.md section 4.22; the bounds below are 8 times them):
    tanh: at most 2.40 ulp of the result from np.tanh in float64, over the grid of `test_tanh...`
    end to end, relative to 1 + the sum of absolute summands: outputs 2.6e-7, gradient 1.8e-7"""
from __future__ import annotations

import ctypes as C
import ctypes.util
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from sparc_amd import PolicyNet, _abi, _lib
from sparc_amd.policy_net import (back32, fma32, layer32, layout, policy_net_reference, rowsum32, tanh32, tree32)
from tests import _policy_net_common as pc
from tests._normalize_common import same_bits

ROOT = Path(__file__).resolve().parent.parent
TANH_ULP_MEASURED, OUT_MEASURED, GRAD_MEASURED = 2.40, 2.6e-7, 1.8e-7
U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ 1. the C-ABI
def test_desc_struct_mirror_matches_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wedm_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(wedm_net_desc));']
    for field, _ in _abi.NetDesc._fields_:
        lines.append(f'  printf("{field} %zu\\n", offsetof(wedm_net_desc, {field}));')
    lines += ['  printf("consts %d %d %d abi %d\\n", WEDM_NET_MAX_HIDDEN, WEDM_NORM_MAX_COLUMNS, WEDM_NORM_MAX_TILES, WEDM_ABI_VERSION);',
              '  printf("flagbits %d %d %d %d\\n", WEDM_NET_FORWARD, WEDM_NET_BACKWARD, WEDM_NET_FOLD, WEDM_NET_ACCUMULATE);',
              '  printf("acts %d %d\\n", WEDM_NET_RELU, WEDM_NET_TANH);', "  return 0;", "}"]
    src = tmp_path / "desc.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "desc"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    out = dict(row.split(" ", 1) for row in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("size")) == C.sizeof(_abi.NetDesc)
    assert out.pop("consts") == f"{_abi.NET_MAX_HIDDEN} {_abi.NORM_MAX_COLUMNS} {_abi.NORM_MAX_TILES} abi 4" == "128 160 4096 abi 4"
    assert out.pop("flagbits") == f"{_abi.NET_FORWARD} {_abi.NET_BACKWARD} {_abi.NET_FOLD} {_abi.NET_ACCUMULATE}" == "1 2 4 8"
    assert out.pop("acts") == f"{_abi.NET_RELU} {_abi.NET_TANH}" == "0 1" and _abi.NET_ACTIVATIONS == ("relu", "tanh")
    assert {k: int(v) for k, v in out.items()} == {f: getattr(_abi.NetDesc, f).offset for f, _ in _abi.NetDesc._fields_}


def test_the_call_is_exported_and_the_abi_version_stays():
    assert "wedm_policy_net" in _lib.EXPORTS and hasattr(_lib.HipBackend, "policy_net")
    L = _lib.load()
    assert L.wedm_policy_net is not None and L.wedm_abi_version() == _abi.ABI_VERSION == 4
    assert "int32_t wedm_policy_net(const wedm_net_desc* desc, void* stream);" in (ROOT / "include" / "wedm_hip.h").read_text()


def test_bad_arguments_are_refused_before_anything_is_launched():
    """Every pointer below is an address nobody owns: a call that launched would fault (and on a machine without a device
    fail with WEDM_ERR_HIP); every case returns WEDM_ERR_BAD_ARG with a text."""
    L = _lib.load()
    A = 0x1000000   # blocks 0x100000 apart: the largest, partials, is 7 178 floats
    names = ("theta", "obs", "index", "params", "value", "grad_params", "grad_value", "partials", "grad_theta")
    at = {name: A + 0x100000 * i for i, name in enumerate(names)}
    ALL = _abi.NET_FORWARD | _abi.NET_BACKWARD | _abi.NET_FOLD
    n_theta = layout(13, (64, 64), 9)["n_theta"][0]

    def desc(**kw):
        f = dict(at, obs_stride=14, param_stride=20, grad_stride=20, n_src=150, obs_dim=13, hidden1=64, hidden2=64, n_modes=9,
                 activation=_abi.NET_TANH, rows=100, flags=ALL)
        f.update(kw)
        return _abi.NetDesc(**f)

    def refused(d, what):
        assert L.wedm_policy_net(C.byref(d), None) == _abi.ERR_BAD_ARG, what
        text = L.wedm_last_error(None)
        assert text.startswith(b"wedm_policy_net: ") and len(text) > len(b"wedm_policy_net: "), what

    assert L.wedm_policy_net(None, None) == _abi.ERR_BAD_ARG and L.wedm_last_error(None).startswith(b"wedm_policy_net:")
    for flags in (0, 16, -1, 1 << 30, _abi.NET_FORWARD | 32, _abi.NET_ACCUMULATE):
        refused(desc(flags=flags), ("flags", flags))
    for rows in (0, -5, _abi.NORM_MAX_TILES * 256 + 1, 2 ** 31 - 1):
        refused(desc(rows=rows), ("rows", rows))
    for n_src in (0, -1):
        refused(desc(n_src=n_src), ("n_src", n_src))
    for D in (0, -1, _abi.NORM_MAX_COLUMNS + 1):
        refused(desc(obs_dim=D, obs_stride=200), ("obs_dim", D))
    for h in (0, 8, 15, 17, 24, 144, -16):
        refused(desc(hidden1=h), ("hidden1", h))
        refused(desc(hidden2=h), ("hidden2", h))
    for n_modes in (0, -1, _abi.HEAD_MAX_MODES + 1):
        refused(desc(n_modes=n_modes), ("n_modes", n_modes))
    for act in (-1, 2):
        refused(desc(activation=act), ("activation", act))
    refused(desc(obs_stride=12), "obs_stride below D")
    refused(desc(param_stride=16), "param_stride below P")
    refused(desc(grad_stride=16), "grad_stride below P")
    # every block a phase needs: null, and one byte off
    for name in names:
        if name != "index":
            refused(desc(**{name: None}), ("null", name))
        refused(desc(**{name: at[name] + 1}), ("one byte off", name))
    refused(desc(index=at["index"] + 4), "index to 8 bytes")
    for flags, name in ((_abi.NET_FORWARD, "params"), (_abi.NET_FORWARD, "value"), (_abi.NET_BACKWARD, "grad_params"),
                        (_abi.NET_BACKWARD, "grad_value"), (_abi.NET_BACKWARD, "partials"), (_abi.NET_FOLD, "partials"),
                        (_abi.NET_FOLD, "grad_theta"), (_abi.NET_FORWARD, "theta"), (_abi.NET_BACKWARD, "obs")):
        refused(desc(flags=flags, **{name: None}), ("null in its phase alone", flags, name))
    # an output block on an input block: the same address, its last element
    refused(desc(params=at["obs"]), "params on obs")
    refused(desc(value=at["theta"] + (n_theta - 1) * 4), "value on theta's last element")
    refused(desc(partials=at["grad_params"] + (99 * 20 + 16) * 4), "partials on grad_params' last element")
    refused(desc(grad_theta=at["grad_value"] + 99 * 4), "grad_theta on grad_value's last element")
    refused(desc(grad_theta=at["index"] + 99 * 8), "grad_theta on index's last element")
    refused(desc(params=at["theta"] - (99 * 20 + 17) * 4 + 4), "params' last element on theta")


# (D, M, hidden) -> theta in LDS in the forward, the parked node in LDS, theta in LDS in the backward: `net_make_shape` of
# csrc/wedm_policy_net.h worked by hand.  In floats against 40 960: src 256, the activations 128 (H1 + 4) + 128 (H2 + 4), in
# the backward go 4 608, then the park (n_theta) where it fits, then the staged theta (rows of N + 4) where it fits.
LDS_PLANS = (
    (13, 9, (16, 16), True, True, True),       # backward 9 984 + 802 + 994
    (13, 9, (32, 128), True, True, False),     # backward 26 368 + 6 994 = 33 362, + 7 698 = 41 060; forward 21 760 + 7 698
    (13, 9, (64, 128), True, False, False),    # backward 30 464 + 11 538 = 42 002; forward 25 856 + 12 370 = 38 226
    (13, 9, (80, 128), False, False, False),   # forward 27 904 + 14 706 = 42 610
    (17, 9, (128, 32), True, True, False),     # backward 26 368 + 7 026 = 33 394, + 7 746 = 41 140
    (16, 19, (128, 128), False, False, False),  # forward 34 048 + 23 400
    (160, 19, (16, 128), True, True, False),   # backward 24 320 + 8 364 = 32 684, + 9 592 = 42 276
    (160, 19, (48, 112), True, False, False),  # backward 26 368 + 16 380 = 42 748; forward 21 760 + 17 672 = 39 432
    (160, 19, (48, 128), False, False, False),  # forward 23 808 + 18 968 = 42 776
    (1, 1, (48, 128), True, True, False),      # backward 28 416 + 7 658 = 36 074, + 8 378 = 44 452; forward 23 808 + 8 378
    (1, 1, (80, 128), True, False, False),     # backward 32 512 + 11 818 = 44 330; forward 27 904 + 12 666 = 40 570
    (1, 1, (96, 128), False, False, False),    # forward 29 952 + 14 810 = 44 762
)


@pytest.mark.parametrize("D,M,hidden,forward_theta,park,backward_theta", LDS_PLANS)
def test_the_mirror_of_net_make_shape_gives_the_rows_worked_by_hand(D, M, hidden, forward_theta, park, backward_theta):
    O = 9 + M
    assert pc.lds_plan(D, *hidden, O, False) == (False, forward_theta)
    assert pc.lds_plan(D, *hidden, O, True) == (park, backward_theta)


def test_the_mirror_of_net_make_shape_never_stages_theta_beside_a_park_in_partials():
    """The staged copy has rows of N + 4, so it is larger than n_theta: where the park does not fit, it does not either.
    `net_make_shape` sizes the workspace from the same dims as `layout`."""
    for D in (1, 6, 13, 160):
        for M in (1, 8, 19):
            for H1 in range(16, 129, 16):
                for H2 in range(16, 129, 16):
                    park, theta = pc.lds_plan(D, H1, H2, 9 + M, True)
                    assert park or not theta, (D, M, H1, H2)
                    assert theta <= pc.lds_plan(D, H1, H2, 9 + M, False)[1]   # the forward has go's 4 608 floats more room


# ------------------------------------------------------------------------------------------------ 2. the float32 fma
def _fmaf():
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype, libm.fmaf.argtypes = C.c_float, [C.c_float] * 3
    return lambda a, b, c: np.array([libm.fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], dtype=np.float32)


def test_the_numpy_fma_is_libms_fmaf():
    fmaf, rng, n = _fmaf(), np.random.default_rng(0), 30000
    mag = lambda lo, hi: (rng.standard_normal(n) * 10.0 ** rng.integers(lo, hi, n)).astype(np.float32)   # noqa: E731
    sets = {"random": (mag(-20, 20), mag(-20, 20), mag(-25, 25))}
    a, b = mag(-10, 10), mag(-10, 10)
    sets["exact cancellation of the rounded product"] = (a, b, -(a * b))
    # halfway: a * b = +-(1 - 2^-46) exactly and c = +-(2^24 + 2 m), whose float32 neighbours are 2 apart: the float64 sum
    # rounds to an odd integer, a tie of float32, and loses the 2^-46 that decides it -- rounded to nearest and cast, it
    # goes to the even neighbour; the residual is not zero and says which side the sum lies on
    m = rng.integers(0, 1000, n).astype(np.float32)
    scale = (2.0 ** rng.integers(-60, 60, n)).astype(np.float32)
    sa, sc = (np.where(rng.integers(0, 2, n) == 1, np.float32(1), np.float32(-1)) for _ in range(2))
    a = sa * np.float32(1.0 + 2.0 ** -23) * scale
    b = np.full(n, 1.0 - 2.0 ** -23, dtype=np.float32)
    sets["halfway"] = (a, b, sc * (np.float32(2.0 ** 24) + 2 * m) * scale)
    sets["subnormal results"] = (mag(-25, -15), mag(-25, -15), (rng.standard_normal(n) * 1e-40).astype(np.float32))
    halfway_seen = False
    for name, (a, b, c) in sets.items():
        got, want = fma32(a, b, c), fmaf(a, b, c)
        assert same_bits(got, want), (name, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        if name.startswith("halfway"):
            p = a.astype(np.float64) * b.astype(np.float64)
            s = p + c.astype(np.float64)
            resid = (p - (s - (s - p))) + (c.astype(np.float64) - (s - p))
            naive = s.astype(np.float32)   # the float64 sum rounded to nearest, then cast: double rounding
            halfway_seen |= bool(((resid != 0) & (naive.view(np.uint32) != want.view(np.uint32))).any())
    assert halfway_seen, "no triple on which the rounding to odd matters"
    assert same_bits(fma32(np.float32(0.0), np.float32(-0.0), np.float32(-0.0)), np.float32(-0.0))
    assert same_bits(fma32(np.float32(0.0), np.float32(0.0), np.float32(-0.0)), np.float32(0.0))


# ------------------------------------------------------------------------------------------------ 3. the tanh
def test_tanh_against_float64_on_every_64th_float32_up_to_ten():
    top = int(np.float32(10.0).view(np.uint32))
    bits = np.concatenate([np.arange(0, top + 1, 64, dtype=np.uint32), np.array([1, 0x007FFFFF, 0x00800000, top], dtype=np.uint32)])
    bits.sort()
    x = bits.view(np.float32)
    h = tanh32(x)
    ref = np.tanh(x.astype(np.float64))
    ulp = np.maximum(np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64), 2.0 ** -149)
    err = np.abs(h.astype(np.float64) - ref) / ulp
    worst = float(err.max())
    print(f"tanh: largest error {worst:.3f} ulp at {x[err.argmax()]!r}")
    assert worst <= 8 * TANH_ULP_MEASURED
    assert bool((np.diff(h) >= 0).all()), "monotone on the grid"
    assert bool((np.abs(h) <= 1).all()) and float(h.max()) == 1.0
    assert same_bits(tanh32(-x), -h), "odd"
    special = np.array([0.0, -0.0, np.inf, -np.inf, 10.5, -1e30, np.nan], dtype=np.float32)
    got = tanh32(special)
    assert same_bits(got[:6], np.array([0.0, -0.0, 1.0, -1.0, 1.0, -1.0], dtype=np.float32)) and np.isnan(got[6])
    assert same_bits(h[:3], x[:3]), "the smallest subnormals are fixed points"


# ------------------------------------------------------------------------------------------------ 4. products and the whole
def _chain_bound(K, mag):
    return (K + 2) * U * mag


@pytest.mark.parametrize("activation", ("relu", "tanh"))
def test_every_product_against_float64_under_the_bound_of_an_fma_chain(activation):
    rows, D, hidden, M = 300, 13, (32, 48), 9
    call = pc.draw_call(rows, D, hidden, M, "repeats", seed=21)
    res = pc.define(call, activation)
    lay = layout(D, hidden, M)
    th = call["theta"].astype(np.float64)
    W = {k: th[at: at + int(np.prod(s))].reshape(s) for k, (at, s) in lay.items() if k != "n_theta"}
    f64 = lambda a: a.astype(np.float64)   # noqa: E731
    # the layers, fed the definition's own float32 inputs
    for inp, w, b, got in ((res["x"], "W1", "b1", res["a1"]), (res["h1"], "W2", "b2", res["a2"]), (res["h2"], "W3", "b3", res["out"])):
        want = f64(inp) @ W[w] + W[b]
        mag = np.abs(W[b]) + np.abs(f64(inp)) @ np.abs(W[w])
        assert (np.abs(f64(got) - want) <= _chain_bound(W[w].shape[0], mag)).all(), w
    # the back-propagated products (before act')
    for g, w, name in ((res["go"], "W3", "dh2"), (res["da2"], "W2", "dh1")):
        got = back32(g, W[w].astype(np.float32))
        want, mag = f64(g) @ W[w].T, np.abs(f64(g)) @ np.abs(W[w]).T
        assert (np.abs(f64(got) - want) <= _chain_bound(W[w].shape[1], mag)).all(), name
    # the row sums: a chunk's chain of 64 and the tree's depth (two levels in the tile, one over two tiles)
    depth = 3
    ones = np.ones((rows, 1), dtype=np.float32)
    for inp, g, name in ((res["x"], res["da1"], "W1"), (res["h1"], res["da2"], "W2"), (res["h2"], res["go"], "W3")):
        ext = np.concatenate([inp, ones], axis=1)
        at = lay[name][0]
        got = res["grad_theta"][at: at + ext.shape[1] * g.shape[1]].reshape(ext.shape[1], g.shape[1])
        want, mag = f64(ext).T @ f64(g), np.abs(f64(ext)).T @ np.abs(f64(g))
        assert (np.abs(f64(got) - want) <= _chain_bound(64 + depth, mag)).all(), f"d{name}"


# the last: an odd number of column tiles in both hidden layers, O % 4 == 1 and D % 4 == 2
@pytest.mark.parametrize("M,D,hidden", ((1, 13, (32, 48)), (9, 13, (32, 48)), (19, 13, (32, 48)), (8, 6, (48, 80))),
                         ids=("1", "9", "19", "8-D6-48x80"))
@pytest.mark.parametrize("activation", ("relu", "tanh"))
def test_the_definition_against_torch_float64_autograd(M, D, hidden, activation):
    rng = np.random.default_rng(100 + M)
    rows, P = 4096, 8 + M
    lay = layout(D, hidden, M)
    th = (rng.standard_normal(lay["n_theta"][0]) * 0.3).astype(np.float32)
    obs = rng.standard_normal((rows, D)).astype(np.float32)
    gp, gv = rng.standard_normal((rows, P)).astype(np.float32), rng.standard_normal(rows).astype(np.float32)
    if activation == "relu":
        # a pre-activation within rounding distance of 0 may have another sign in float32 than in float64, and act' jumps
        # there: rows that hold one (a few in 4096) are drawn again, so that both sides differentiate the same function
        w64 = {k: th[at: at + int(np.prod(s))].reshape(s).astype(np.float64) for k, (at, s) in lay.items() if k != "n_theta"}
        for _ in range(50):
            x64 = obs.astype(np.float64)
            a1 = x64 @ w64["W1"] + w64["b1"]
            m1 = np.abs(x64) @ np.abs(w64["W1"]) + np.abs(w64["b1"])
            g1 = np.maximum(a1, 0.0)
            a2 = g1 @ w64["W2"] + w64["b2"]
            m2 = g1 @ np.abs(w64["W2"]) + np.abs(w64["b2"]) + m1 @ np.abs(w64["W2"])
            near = (np.abs(a1) <= 200 * U * m1).any(axis=1) | (np.abs(a2) <= 200 * U * m2).any(axis=1)
            if not near.any():
                break
            obs[near] = rng.standard_normal((int(near.sum()), D)).astype(np.float32)
        assert not near.any()
    res = policy_net_reference(th, obs, hidden=hidden, n_modes=M, activation=activation, grad_params=gp, grad_value=gv)
    t = torch.tensor(th.astype(np.float64), requires_grad=True)
    part = lambda src: {k: src[at: at + int(np.prod(s))].view(s) for k, (at, s) in lay.items() if k != "n_theta"}   # noqa: E731
    w, f = part(t), (torch.tanh if activation == "tanh" else torch.relu)
    X, go = torch.tensor(obs.astype(np.float64)), torch.tensor(np.concatenate([gp, gv[:, None]], 1).astype(np.float64))
    h1 = f(X @ w["W1"] + w["b1"])
    h2 = f(h1 @ w["W2"] + w["b2"])
    out = h2 @ w["W3"] + w["b3"]
    (out * go).sum().backward()
    with torch.no_grad():
        a = part(t.detach().abs())
        out_mag = 1 + (h2.abs() @ a["W3"] + a["b3"])
        dact = (lambda h: 1 - h * h) if activation == "tanh" else (lambda h: (h > 0).double())
        d2 = (go @ w["W3"].T) * dact(h2)
        d1 = (d2 @ w["W2"].T) * dact(h1)
        ones = torch.ones(rows, 1, dtype=torch.float64)
        mag = 1 + torch.cat([(torch.cat([i.abs(), ones], 1).T @ g.abs()).reshape(-1) for i, g in ((X, d1), (h1, d2), (h2, go))])
    e_out = float((np.abs(res["out"].astype(np.float64) - out.detach().numpy()) / out_mag.numpy()).max())
    e_grad = float((np.abs(res["grad_theta"].astype(np.float64) - t.grad.numpy()) / mag.numpy()).max())
    print(f"M = {M}, {activation}: outputs {e_out:.3g}, gradient {e_grad:.3g}")
    assert e_out <= 8 * OUT_MEASURED and e_grad <= 8 * GRAD_MEASURED
    assert same_bits(res["params"], res["out"][:, :P]) and same_bits(res["value"], res["out"][:, P])


# ------------------------------------------------------------------------------------------------ 5. the tree, hand-worked cases
def test_the_row_sum_is_the_tree_over_chunks_and_an_index_changes_no_bit():
    rng = np.random.default_rng(5)
    rows, K, N = 300, 3, 2
    u, v = rng.standard_normal((rows, K)).astype(np.float32), rng.standard_normal((rows, N)).astype(np.float32)
    tiles, root = rowsum32(u, v)

    def chunk(c):
        acc = np.zeros((K, N), dtype=np.float32)
        for r in range(64 * c, min(64 * c + 64, rows)):
            acc = fma32(u[r][:, None], v[r][None, :], acc)
        return acc

    def tree(nodes, width):   # a plain recursion over a padded range: a right half that holds nothing is skipped
        if width == 1:
            return nodes[0]
        half = width // 2
        left = tree(nodes[:half], half)
        return left + tree(nodes[half:], half) if len(nodes) > half else left

    chunks = [chunk(c) for c in range(5)]
    want_tiles = [tree(chunks[0:4], 4), tree(chunks[4:5], 4)]
    assert same_bits(tiles, np.stack(want_tiles)) and same_bits(root, tree(want_tiles, 2))
    assert same_bits(tree32(np.stack(chunks))[0], root)
    # through the definition: the same rows through an index into a shuffled store
    call = pc.draw_call(rows, 5, (16, 16), 3, None, seed=8)
    plain = pc.define(call, "tanh")
    store = np.zeros((rows + 9, 5), dtype=np.float32)
    where = rng.permutation(rows + 9)[:rows].astype(np.int64)
    store[where] = call["obs"]
    through = pc.define(dict(call, obs=store, index=where), "tanh")
    for k in ("params", "value", "partials", "grad_theta"):
        assert same_bits(plain[k], through[k]), k


def test_hand_worked_cases():
    D, hidden, M = 3, (16, 16), 2
    lay = layout(D, hidden, M)
    call = pc.draw_call(70, D, hidden, M, None, seed=4)
    # all-zero go: an all-+0.0 gradient
    zero = dict(call, grad_params=np.zeros_like(call["grad_params"]), grad_value=np.zeros_like(call["grad_value"]))
    res = pc.define(zero, "tanh")
    assert same_bits(res["grad_theta"], np.zeros_like(res["grad_theta"])) and same_bits(res["partials"], np.zeros_like(res["partials"]))
    # a -0.0 bias with a zero observation: a = -0.0, at every padding of D (the weights are negative, so every product
    # is (+0.0)(w) = -0.0; one +0.0 product, such as a padded k-step could add, would make it +0.0)
    for D in (1, 3, 5):
        lay = layout(D, hidden, M)
        n_theta = lay["n_theta"][0]
        th = np.random.default_rng(D).standard_normal(n_theta).astype(np.float32)
        at = lay["b1"][0]
        th[:at] = -np.abs(th[:at]) - np.float32(0.1)
        th[at: at + 16] = -0.0
        obs = np.zeros((2, D), dtype=np.float32)
        res = policy_net_reference(th, obs, hidden=hidden, n_modes=M, activation="tanh")
        assert same_bits(res["a1"], np.full((2, 16), -0.0, dtype=np.float32)) and same_bits(res["h1"], res["a1"])
    # an index outside the store is never read: the store is followed by NaN, the row's input and gradient are +0.0
    D = 3
    lay = layout(D, hidden, M)
    call = pc.draw_call(6, D, hidden, M, None, seed=9)
    store = np.concatenate([call["obs"], np.full((3, D), np.nan, dtype=np.float32)])
    idx = np.array([0, 6 + 3, -1, 3, 2 ** 40, 5], dtype=np.int64)
    res = policy_net_reference(call["theta"], store[:6], hidden=hidden, n_modes=M, index=idx, grad_params=call["grad_params"],
                               grad_value=call["grad_value"])
    bad = np.array([False, True, True, False, True, False])
    assert same_bits(res["x"][bad], np.zeros((3, D), dtype=np.float32)) and same_bits(res["go"][bad], np.zeros((3, 8 + M + 1), dtype=np.float32))
    assert np.isfinite(res["grad_theta"]).all() and np.isfinite(res["params"]).all()
    only = policy_net_reference(call["theta"], store[:6], hidden=hidden, n_modes=M, index=idx[~bad], grad_params=call["grad_params"][~bad],
                                grad_value=call["grad_value"][~bad])
    assert same_bits(res["params"][~bad], only["params"])
    at, shape = lay["W3"]   # a bad row adds +0.0 products only: the weight gradients of the good rows alone
    assert np.array_equal(res["grad_theta"][at: at + shape[0] * shape[1]], only["grad_theta"][at: at + shape[0] * shape[1]])


# ------------------------------------------------------------------------------------------------ 6. PolicyNet
class _Head:
    """What `PolicyNet` asks of a head."""

    def __init__(self, modes=(5, 9, 13)):
        self.modes, self.param_dim, self.device, self._native = tuple(modes), 8 + len(modes), torch.device("cpu"), None


def test_policy_net_on_the_cpu_is_the_definition_and_its_state_dict_refuses_other_dims():
    net = PolicyNet(13, _Head(), hidden=(32, 16), activation="relu", seed=3)
    again = PolicyNet(13, _Head(), hidden=(32, 16), activation="relu", seed=3)
    assert same_bits(net.theta, again.theta) and net.theta.requires_grad and net.theta.is_leaf
    assert net.W1.shape == (13, 32) and net.b3.shape == (12,) and net.W2.data_ptr() == net.theta.data_ptr() + (14 * 32) * 4
    obs = torch.randn(70, 13, generator=torch.Generator().manual_seed(1))
    want = policy_net_reference(net.theta, obs, hidden=(32, 16), n_modes=3, activation="relu")
    params, value = net.forward(obs)
    assert same_bits(params, want["params"]) and same_bits(value, want["value"]) and not params.requires_grad
    params, value = net(obs)
    assert params.requires_grad and value.requires_grad
    gp, gv = torch.randn(70, 11), torch.randn(70)
    torch.autograd.backward((params, value), (gp, gv))
    want = policy_net_reference(net.theta, obs, hidden=(32, 16), n_modes=3, activation="relu", grad_params=gp, grad_value=gv)
    assert same_bits(net.theta.grad, want["grad_theta"])
    params, value = net(obs)   # a second backward adds to theta.grad with one float32 addition
    torch.autograd.backward((params, value), (gp, gv))
    assert same_bits(net.theta.grad, want["grad_theta"] + want["grad_theta"])
    opt = torch.optim.Adam([net.theta], lr=1e-3)
    opt.step()
    assert not same_bits(net.theta, again.theta)
    # checkpoints
    sd = net.state_dict()
    again.load_state_dict(sd)
    assert same_bits(again.theta, net.theta)
    for other in (PolicyNet(12, _Head(), hidden=(32, 16), activation="relu"), PolicyNet(13, _Head(), hidden=(32, 32), activation="relu"),
                  PolicyNet(13, _Head(), hidden=(32, 16), activation="tanh"), PolicyNet(13, _Head((5, 9)), hidden=(32, 16), activation="relu")):
        before = other.theta.detach().clone()
        with pytest.raises(ValueError, match="dims"):
            other.load_state_dict(sd)
        assert same_bits(other.theta, before)
    for bad in (dict(hidden=(32,)), dict(hidden=(32, 20)), dict(hidden=(16, 256)), dict(activation="gelu")):
        with pytest.raises(ValueError):
            PolicyNet(13, _Head(), **bad)
    with pytest.raises(ValueError):
        net(obs, index=torch.arange(3))
    with pytest.raises(ValueError):
        net.forward(obs.double())


# ------------------------------------------------------------------------------------------------ 7. the stack
@pytest.mark.parametrize("variant", ("in-kernel", "frozen", "host-reset"))
def test_the_stack_with_a_policy_net_resumes_byte_for_byte_at_every_cut(variant, tmp_path):
    pc.check_resume_at_every_cut(variant, "cpu", tmp_path)
