"""The shape handling of `wedm_policy_net` on the MI355X (sparc_amd/csrc/wedm_policy_net.h), swept
where tests/test_policy_net.py takes samples: every pair of hidden widths (an odd number of column tiles after full pairs,
every instantiation of `wedm_net_kernel` and every place `net_make_shape` gives the parked node and ``theta``), every mode
count (every k-padding of the output layer, the second column tile of one column) and the edges of the observation width,
the pass and chunk edges with the park in LDS and in ``partials``, and the fold past eight tiles: whole calls, the FOLD
phase alone on synthetic partials up to `NORM_MAX_TILES`, and `PolicyNet` on a workspace that holds stale tiles.  Every
comparison is against `policy_net_reference` (`tree32` for the fold alone) on every byte of every block, inputs and guard
bands included; nothing here has a tolerance."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from sparc_amd import PolicyNet, _abi
from sparc_amd.policy_net import ACTIVATIONS, layout, policy_net_reference, tree32
from tests import _policy_net_common as pc
from tests._normalize_common import same_bits
from tests.test_policy_net import ALL, Problem, device_policy_net
from tests.test_rollout import DEV, Banded, poisoned

pytestmark = pytest.mark.gpu

WIDTHS = tuple(range(16, 129, 16))
SWEEP_ROWS, SWEEP_D, SWEEP_M = 200, 6, 8   # one tile in two passes, the second of 72 rows; D % 4 == 2; O = 17
PADS = dict(obs_pad=2, grad_pad=3)
NAN32 = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]


def check(p: Problem) -> list:
    """The whole call on the device: what differs from the definition (nothing, it is hoped)."""
    want = p.expect()
    device_policy_net(p.desc(ALL))
    g = p.res["grad_theta"]
    assert np.isfinite(g).all() and np.abs(g).sum() > 0
    return p.differences(want)


# ------------------------------------------------------------------------------------------------ 1. every width pair
def sweep():
    """(H1, H2, activation) of every call of the width sweep."""
    return [(H1, H2, activation) for H1 in WIDTHS for H2 in WIDTHS for activation in ACTIVATIONS]


@pytest.mark.parametrize("H1", WIDTHS)
def test_every_second_width_and_both_activations_under_this_first_width(H1):
    bad = {}
    for H2 in WIDTHS:
        call = pc.draw_call(SWEEP_ROWS, SWEEP_D, (H1, H2), SWEEP_M, "repeats", seed=8 * H1 + H2 // 16, **PADS)
        for activation in ACTIVATIONS:
            diff = check(Problem(call, activation, param_pad=3))
            if diff:
                bad[(H1, H2, activation)] = diff
    assert bad == {}


def test_the_width_sweep_runs_every_reachable_lds_state():
    """Forward: ``theta`` in LDS or in global memory; backward: (park, theta) in (LDS, LDS), (LDS, global), (partials,
    global) -- with both activations, all eight instantiations of `wedm_net_kernel` and both parks."""
    O = 9 + SWEEP_M
    forward = {(a, pc.lds_plan(SWEEP_D, H1, H2, O, False)) for H1, H2, a in sweep()}
    backward = {(a, pc.lds_plan(SWEEP_D, H1, H2, O, True)) for H1, H2, a in sweep()}
    assert forward == {(a, (False, t)) for a in ACTIVATIONS for t in (True, False)}
    assert backward == {(a, s) for a in ACTIVATIONS for s in ((True, True), (True, False), (False, False))}


# ------------------------------------------------------------------------------------------------ 2. modes, observation width
@pytest.mark.parametrize("M", range(1, 20))
def test_every_mode_count_under_three_column_tiles_into_one(M):
    """O = 10 ... 28: every k-padding of `bprop`'s chain, `wgrad`'s second column tile from absent (O <= 16) over one column
    (O = 17) to twelve."""
    call = pc.draw_call(200, 7, (48, 16), M, "repeats", seed=300 + M, **PADS)
    assert check(Problem(call, ACTIVATIONS[(M + 1) % 2], param_pad=3)) == []   # relu for odd M


D_EDGES = (2, 3, 15, 16, 31, 47, 63, 64, 65, 159, 160)


@pytest.mark.parametrize("i", range(len(D_EDGES)), ids=[f"D{D}" for D in D_EDGES])
def test_the_edges_of_the_observation_width(i):
    """D + 1 on both sides of a k tile of 16 (the ones row the last row of a full tile, and alone in the next), D on both
    sides of a k-step of 4, the largest D.  The stride is padded for half of them, for each activation."""
    D = D_EDGES[i]
    call = pc.draw_call(200, D, (16, 48), 8, "repeats", seed=400 + D, obs_pad=3 if i % 4 in (0, 3) else 0, grad_pad=3)
    assert check(Problem(call, ACTIVATIONS[i % 2], param_pad=3)) == []


@pytest.mark.parametrize("D", (1, 2, 3, 6, 7))
def test_a_negative_zero_kept_by_the_padded_k_steps_reaches_the_outputs(D):
    """The one place where the sign of a padded step's product can reach a byte the call writes: the first layer's chain
    starts at its bias and is padded from D to a multiple of 4.  Under an all-zero observation, -0.0 biases and negative
    W1, a1 is -0.0, and so is h1 under tanh; with -0.0 biases and positive W2 and W3 behind it the row's a2, h2 and outputs
    are -0.0 too, and one +0.0 product in the first layer's padding turns every one of them into +0.0.  (ReLU maps -0.0 to
    +0.0, and every other padded chain starts at +0.0, which no zero product of either sign changes: there the padding's
    sign reaches no output, and the inputs of tests/test_policy_net.py's hostile values, whose -0.0 stays in a1, cannot
    show it.)"""
    rows, hidden, M = 70, (48, 16), 8
    call = pc.draw_call(rows, D, hidden, M, "repeats", seed=450 + D, **PADS)
    lay, th = layout(D, hidden, M), call["theta"]
    for name, sign in (("W1", -1.0), ("W2", 1.0), ("W3", 1.0)):
        at, shape = lay[name]
        th[at: at + shape[0] * shape[1]] = np.float32(sign) * (np.abs(th[at: at + shape[0] * shape[1]]) + np.float32(0.1))
    for name in ("b1", "b2", "b3"):
        at, shape = lay[name]
        th[at: at + shape[0]] = -0.0
    call["obs"][5:25, :D] = 0.0
    call["index"][5:25] = np.arange(5, 25)   # the zero rows are reached
    p = Problem(call, "tanh", param_pad=3)
    assert check(p) == []
    for name in ("a1", "h1", "a2", "h2", "out"):
        zero = p.res[name][5:25]
        assert (np.signbit(zero) & (zero == 0)).all(), name


# ------------------------------------------------------------------------------------------------ 3. pass and chunk edges
EDGE_ROWS = (127, 128, 129, 191, 192, 193, 385)
EDGE_NETS = {"park in LDS": (16, 48), "park in partials": (96, 128)}


@pytest.mark.parametrize("where", tuple(EDGE_NETS))
@pytest.mark.parametrize("rows", EDGE_ROWS)
def test_pass_and_chunk_edges_with_the_park_in_lds_and_in_partials(rows, where):
    hidden = EDGE_NETS[where]
    park, _ = pc.lds_plan(SWEEP_D, *hidden, 9 + SWEEP_M, True)
    assert park == (where == "park in LDS")
    activation = ACTIVATIONS[(EDGE_ROWS.index(rows) + tuple(EDGE_NETS).index(where)) % 2]
    call = pc.draw_call(rows, SWEEP_D, hidden, SWEEP_M, "repeats", seed=500 + rows, **PADS)
    assert check(Problem(call, activation, param_pad=3)) == []


# ------------------------------------------------------------------------------------------------ 4. the deep fold
FOLD_NET = dict(D=1, hidden=(16, 16), M=1)   # n_theta = 474
FOLD_TILES = (5, 7, 8, 9, 11, 13, 16, 17, 21, 24, 33, 53, 64, 65)
FOLD_LAST = (1, 64, 129, 256)   # rows of the last tile


@pytest.mark.parametrize("tiles", FOLD_TILES)
def test_whole_calls_whose_fold_is_deeper_than_one_tile_per_group(tiles):
    """5, 7, 8: one tile per group, groups 4 to 7 present; from 9 on a group walks its counter; 53: a group of 5 of 8 tiles
    (two subtrees joined from the top) before an absent one; 65: 16 tiles per group."""
    rows = 256 * (tiles - 1) + FOLD_LAST[FOLD_TILES.index(tiles) % 4]
    call = pc.draw_call(rows, FOLD_NET["D"], FOLD_NET["hidden"], FOLD_NET["M"], None, seed=600 + tiles)
    assert check(Problem(call, ACTIVATIONS[FOLD_TILES.index(tiles) % 2])) == []


N_THETA = layout(FOLD_NET["D"], FOLD_NET["hidden"], FOLD_NET["M"])["n_theta"][0]
COL_NAN, COL_NAN_ONCE, COL_INF_BOTH, COL_INF, COL_NEG_ZERO, COL_SUBNORMAL = 5, 6, 7, 8, 9, 10
SPECIAL = (COL_NAN, COL_NAN_ONCE, COL_INF_BOTH, COL_INF)


@functools.lru_cache(maxsize=None)
def synthetic_partials() -> np.ndarray:
    """``[NORM_MAX_TILES, 474]``, read-only, a call of t tiles takes the first t: normal draws times 2^k, k uniform in
    [-12, 12), a fiftieth each -0.0 and subnormals of either sign; a column of NaN with a payload, one with such a NaN in
    tile 3 alone, one of +inf and -inf in turn, one of +inf, one of -0.0, one of positive subnormals."""
    rng = np.random.default_rng(4)
    shape = (_abi.NORM_MAX_TILES, N_THETA)
    v = (rng.normal(size=shape) * 2.0 ** rng.integers(-12, 12, size=shape)).astype(np.float32)
    v[rng.random(shape) < 0.02] = -0.0
    sub = rng.integers(1, 0x00800000, size=shape).astype(np.uint32) | (rng.integers(0, 2, size=shape).astype(np.uint32) << np.uint32(31))
    v = np.where(rng.random(shape) < 0.02, sub.view(np.float32), v)
    payload = np.array([0x7FA12345], dtype=np.uint32).view(np.float32)[0]
    v[:, COL_NAN] = payload
    v[3, COL_NAN_ONCE] = payload
    v[:, COL_INF_BOTH] = np.where(np.arange(shape[0]) % 2 == 0, np.inf, -np.inf)
    v[:, COL_INF] = np.inf
    v[:, COL_NEG_ZERO] = -0.0
    v[:, COL_SUBNORMAL] = np.abs(sub[:, COL_SUBNORMAL].view(np.float32))
    assert (v[:, COL_NAN].view(np.uint32) == 0x7FA12345).all()
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def left_to_right() -> np.ndarray:
    """Row t - 1: the plain float32 sum of the first t tiles, the lower index first."""
    with np.errstate(all="ignore"):
        return np.cumsum(synthetic_partials(), axis=0, dtype=np.float32)


def canon(x: np.ndarray) -> np.ndarray:
    return np.where(x != x, NAN32, x).astype(np.float32)


FOLD_COUNTS = {"1 to 40": tuple(range(1, 41)), "255 to 257": (255, 256, 257), "1000": (1000,), "the most": (_abi.NORM_MAX_TILES,)}


@pytest.mark.parametrize("accumulate", (False, True), ids=("store", "accumulate"))
@pytest.mark.parametrize("counts", tuple(FOLD_COUNTS))
def test_the_fold_alone_is_the_tree_over_synthetic_partials(counts, accumulate):
    """`NET_FOLD` by itself, with and without `NET_ACCUMULATE` (onto a gradient that holds -0.0 in places, under the column
    of -0.0 among them).  From four tiles on the tree is another sum than the one from left to right (at three they are the
    same expression, (a + b) + c), and the inputs show it: they differ in a finite column at every such count."""
    assert N_THETA == 474
    v, plain = synthetic_partials(), left_to_right()
    before = np.random.default_rng(2).normal(size=N_THETA).astype(np.float32)
    before[::5] = -0.0
    before[COL_NEG_ZERO] = -0.0
    bad = {}
    for tiles in FOLD_COUNTS[counts]:
        with np.errstate(all="ignore"):
            root = tree32(v[:tiles])[0]
            want = canon(before + root if accumulate else root)
        finite = np.isfinite(root) & np.isfinite(plain[tiles - 1])
        if tiles > 3:
            assert not finite[list(SPECIAL)].any() and (root[finite] != plain[tiles - 1][finite]).any(), tiles
        host = v[:tiles].copy()
        partials = Banded(host)
        grad = Banded(before if accumulate else poisoned((N_THETA,), np.float32))
        desc = _abi.NetDesc(partials=partials.t.data_ptr(), grad_theta=grad.t.data_ptr(), n_src=1, obs_dim=FOLD_NET["D"], obs_stride=1,
                            hidden1=FOLD_NET["hidden"][0], hidden2=FOLD_NET["hidden"][1], n_modes=FOLD_NET["M"], param_stride=9, grad_stride=9,
                            activation=_abi.NET_RELU, rows=256 * (tiles - 1) + 1, flags=_abi.NET_FOLD | (_abi.NET_ACCUMULATE if accumulate else 0))
        device_policy_net(desc)
        torch.cuda.synchronize()
        diff = [name for name, ok in (("grad_theta", same_bits(grad.t, want)), ("input partials", same_bits(partials.t, host)),
                                      ("band of grad_theta", grad.bands_intact()), ("band of partials", partials.bands_intact())) if not ok]
        if diff:
            where = np.flatnonzero(grad.t.cpu().numpy().view(np.uint32) != want.view(np.uint32))
            bad[tiles] = (diff, where[:8].tolist())
    assert bad == {}
    assert same_bits(want[[COL_NAN, COL_NEG_ZERO]], np.array([NAN32, -0.0], dtype=np.float32))


class _Native:
    """What `PolicyNet` asks of a head's backend."""

    @staticmethod
    def policy_net(desc) -> None:
        device_policy_net(desc)


class _Head:
    """What `PolicyNet` asks of a head: one mode, the network on the GPU."""
    modes, param_dim, device, _native = (5,), 9, torch.device(DEV), _Native()


def test_the_adapter_folds_ten_tiles_then_two_over_stale_ones_then_accumulates():
    D, hidden, P = 3, (16, 32), 9
    net = PolicyNet(D, _Head(), hidden=hidden, activation="tanh", seed=7)
    assert net._native is not None
    theta = net.theta.detach().cpu().numpy().copy()
    gen = torch.Generator().manual_seed(9)

    def backward(rows):
        obs, gp, gv = (torch.randn(shape, generator=gen) for shape in ((rows, D + 2), (rows, P), (rows,)))
        params, value = net(obs.to(DEV))
        want = policy_net_reference(theta, obs[:, :D].numpy().copy(), hidden=hidden, n_modes=1, activation="tanh", grad_params=gp.numpy(),
                                    grad_value=gv.numpy())
        assert same_bits(params, want["params"]) and same_bits(value, want["value"])
        torch.autograd.backward((params, value), (gp.to(DEV), gv.to(DEV)))
        assert np.isfinite(want["grad_theta"]).all() and np.abs(want["grad_theta"]).sum() > 0
        return want

    first = backward(2305)   # nine full tiles and a row: ten tiles, two to a group of the fold
    assert net._partials.shape[0] == 10
    assert same_bits(net.theta.grad, first["grad_theta"]) and same_bits(net._partials, first["partials"])
    net.theta.grad = None
    second = backward(300)   # two tiles; the workspace keeps the eight behind them, which the fold must not read
    assert net._partials.shape[0] == 10 and same_bits(net._partials[:2], second["partials"]) and same_bits(net._partials[2:], first["partials"][2:])
    assert same_bits(net.theta.grad, second["grad_theta"])
    assert not same_bits(second["grad_theta"], tree32(np.concatenate([second["partials"], first["partials"][2:]]))[0])
    third = backward(300)    # theta.grad exists: ACCUMULATE, one float32 addition per element
    assert same_bits(net.theta.grad, (second["grad_theta"] + third["grad_theta"]).astype(np.float32))
    assert same_bits(net.theta, theta)
