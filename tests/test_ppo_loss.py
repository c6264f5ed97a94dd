"""PPO's loss on the MI355X (sparc_amd/csrc/wedm_ppo.h, sparc_amd/ppo.py): `wedm_ppo_loss` against
`ppo_loss_definition` on every byte of everything it may write -- the gradient blocks with their padding columns, the tile
partials, the statistics, the count words, each between guard bands -- at the wave and block edges, through LDS and
directly, with and without a mask, an index, value clipping and the gradient; every mode count from 1 to 19; a wide
regime (ratios of 0 and +inf, clip = 0, advantages and returns from subnormal to 1e30); the fold alone against an independent
tile tree in every class of tiles per lane up to 4096 tiles, with signed zeros and non-finite nodes, and whole calls at the
first row count of the larger classes; the phases apart; hostile rows; `PPOLoss` through `WireEDMVectorEnv`, `PolicyHead` and
`RolloutBuffer` without a host synchronisation or an allocation; and the call on a side stream behind a gate."""
from __future__ import annotations

import gc

import numpy as np
import pytest
import torch

from sparc_amd import PolicyHead, PPOLoss, RolloutBuffer, WireEDMVectorEnv, _abi
from sparc_amd.ppo import device_ppo_loss, ppo_loss_definition
from tests._gae_common import is_subnormal
from tests._normalize_common import same_bits
from tests._policy_head_common import ALL_M, HI, LO, LOG_SPAN, make_hostile, random_params, zero_probability_rows
from tests._ppo_common import (CLIP_VALUE, COEFS, FOLD_TILES, STORED, definition_kw, draw_minibatch, draw_partials,
                                draw_wide_minibatch, padded_tiles, telling_partials, tile_tree_stats)
from tests._snapshot_common import make
from tests._stream_gate import Gate, check_control, gated, seconds_on
from tests.test_rollout import DEV, FILL, Banded, poisoned

pytestmark = pytest.mark.gpu
EXTRA = 37   # entries of a store beyond the minibatch's rows
OUTPUTS = ("grad_params", "grad_value", "partials", "stats", "count")
OUTSIDE = (-1, -2 ** 63, 2 ** 40, 2 ** 63 - 1)   # and n_src itself: indices that name no entry


class Problem:
    """A minibatch of ``rows`` rows of ``M`` modes on the device and the host.  Dense: params ``[rows, P + pad_in]`` (NaN in
    the padding) and value.  Stored: blocks of ``rows + 37`` entries; a call without an index reads the first ``rows`` of
    them.  Outputs start as 0xA5 bytes, grad_params ``[rows, P + pad_out]``; every block lies between guard bands.
    ``index``: None, "perm" (a permutation of the rows) or "wild" (entries of the whole store with repeats, and some outside
    it); ``valid``: None, "some" or "none" (all zero)."""

    def __init__(self, rows, M, seed, pad_in=0, pad_out=0, hostile=False, wide=None):
        self.rows, self.M, self.P, self.si, self.so = rows, M, 8 + M, 8 + M + pad_in, 8 + M + pad_out
        self.tiles = -(-rows // 256)
        rng = self.rng = np.random.default_rng(seed)
        n = rows + EXTRA
        # ``wide``: None, or the keywords of `draw_wide_minibatch`
        h = self.host = draw_minibatch(rng, n, M, pad_in) if wide is None else draw_wide_minibatch(rng, n, M, pad_in, **wide)
        h["params"], h["value"] = h["params"][:rows].copy(), h["value"][:rows].copy()
        if hostile:
            bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], dtype=np.float32)
            h["params"] = make_hostile(rng, h["params"], M)
            for name in ("value", "advantage", "returns", "old_log_prob", "old_value"):
                hit = rng.choice(h[name].shape[0], h[name].shape[0] // 4, replace=False)
                h[name][hit] = bad[rng.integers(0, bad.size, hit.size)]
            h["mode_index"] = np.resize(np.array([-1, M, -2 ** 31, 2 ** 31 - 1, 1 << 20, 3, 0, -7], dtype=np.int32), n)
        h["valid_some"], h["valid_none"] = h.pop("valid"), np.zeros(n, dtype=np.uint8)
        h["index_perm"] = rng.permutation(rows).astype(np.int64)
        wild = rng.integers(0, n, rows).astype(np.int64)
        hit = rng.choice(rows, max(1, rows // 8), replace=False)
        wild[hit] = np.resize(np.array(OUTSIDE + (n,), dtype=np.int64), hit.size)
        h["index_wild"] = wild
        self.inputs = tuple(h)
        h["grad_params"] = poisoned((rows, self.so), np.float32)
        h["grad_value"] = poisoned((rows,), np.float32)
        h["partials"] = poisoned((self.tiles, _abi.PPO_SUMS), np.float64)
        h["stats"] = poisoned((_abi.PPO_STATS,), np.float64)
        h["count"] = poisoned((_abi.PPO_COUNT_WORDS,), np.int32)
        self.blocks = {name: Banded(a) for name, a in h.items()}

    def poison(self):
        for name in OUTPUTS:
            self.host[name].view(np.uint8)[...] = FILL
            self.blocks[name].raw.fill_(FILL)

    def n_src(self, index):
        return self.rows + EXTRA if index == "wild" else self.rows

    def desc(self, index=None, valid=None, clip_value=False, grads=True, flags=0, lo=0, **coefs):
        """The descriptor of rows [lo, rows): every per-row block entered ``lo`` rows further on."""
        b = self.blocks
        at = lambda name, per_row: b[name].t.data_ptr() + lo * per_row   # noqa: E731
        c = {**COEFS, **coefs}
        d = _abi.PpoDesc(
            params=at("params", 4 * self.si), value=at("value", 4), index=at(f"index_{index}", 8) if index else None,
            u=at("u", 16), mode_index=at("mode_index", 4), old_log_prob=at("old_log_prob", 4), advantage=at("advantage", 4),
            returns=at("returns", 4), old_value=at("old_value", 4) if clip_value else None,
            valid=at(f"valid_{valid}", 1) if valid else None, grad_params=at("grad_params", 4 * self.so) if grads else None,
            grad_value=at("grad_value", 4) if grads else None, partials=b["partials"].t.data_ptr(), stats=b["stats"].t.data_ptr(),
            count=b["count"].t.data_ptr(), param_stride=self.si, grad_stride=self.so, n_src=self.n_src(index) - lo,
            clip=c["clip"], vf_coef=c["vf_coef"], ent_coef=c["ent_coef"], clip_value=CLIP_VALUE if clip_value else 0.0,
            n_modes=self.M, rows=self.rows - lo, flags=flags | (_abi.PPO_CLIP_VALUE if clip_value else 0))
        d.lo[:], d.hi[:], d.log_span[:] = LO, HI, LOG_SPAN
        return d

    def call(self, **kw):
        device_ppo_loss(self.desc(**kw), DEV)

    def definition(self, index=None, valid=None, clip_value=False, lo=0, **coefs):
        h, n = self.host, self.n_src(index)
        stored = {name: h[name][lo:n] for name in STORED if name in h}
        return ppo_loss_definition(h["params"][lo:], h["value"][lo:], index=h[f"index_{index}"][lo:] if index else None,
                                   valid=h[f"valid_{valid}"][lo:n] if valid else None,
                                   **{**stored, **definition_kw(self.M, clip_value, **coefs)})

    def expect(self, out, index=None, valid=None, grads=True, lo=0):
        """The output blocks as the call has to leave them: the definition's values in their places, 0xA5 elsewhere."""
        want = {name: poisoned(self.host[name].shape, self.host[name].dtype) for name in OUTPUTS}
        if grads:
            want["grad_params"][lo:, : self.P] = out["grad_params"]
            want["grad_value"][lo:] = out["grad_value"]
        want["partials"][: out["partials"].shape[0]] = out["partials"]
        want["stats"][:] = out["stats"]
        if index or valid:
            want["count"][:] = out["count"]
        return want

    def differences(self, want=None):
        torch.cuda.synchronize()
        ref = {**self.host, **(want or {})}
        bad = [name for name, b in self.blocks.items() if not same_bits(b.t, ref[name])]
        return bad + [f"band of {name}" for name, b in self.blocks.items() if not b.bands_intact()]

    def check(self, what, **kw):
        call_kw = {k: v for k, v in kw.items() if k != "flags"}
        want = self.expect(self.definition(**{k: v for k, v in call_kw.items() if k != "grads"}),
                           **{k: v for k, v in call_kw.items() if k in ("index", "valid", "grads", "lo")})
        self.poison()
        self.call(**kw)
        assert self.differences(want) == [], (what, kw)
        return want


VARIANTS = (dict(), dict(valid="some"), dict(valid="none", index="perm"), dict(index="perm"), dict(valid="some", index="wild"),
            dict(valid="none"), dict(index="wild"), dict(grads=False), dict(grads=False, valid="some", index="wild"))


# ------------------------------------------------------------------------------------------------ 1. the call
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_the_call_equals_the_definition_on_every_byte(rows):
    """The wave (64) and block (256) edges by M in {1, 2, 9} by the staged and the direct path of params and of grad_params
    (stride P and P + 3, independently) by value clipping, each with: no mask, a mask with zeros, a mask of zeros; no index,
    a permutation, an index with repeats and entries outside a store of rows + 37; and without the gradient blocks.
    Outputs start as 0xA5 bytes and the padding columns, the count words of a call that does not count and the gradient
    blocks of a call without them must come out as they were; no input may change."""
    for M in (1, 2, 9):
        for pad_in in (0, 3):
            for pad_out in (0, 3):
                p = Problem(rows, M, seed=1000 * rows + 100 * M + 10 * pad_in + pad_out, pad_in=pad_in, pad_out=pad_out)
                for clip_value in (False, True):
                    for variant in VARIANTS:
                        p.check((rows, M, pad_in, pad_out), clip_value=clip_value, **variant)


@pytest.mark.parametrize("M", ALL_M)
def test_every_mode_count_equals_the_definition_on_every_byte(M):
    """Every M the header promises (`MODES[M]`; P = 9..27, P divisible by 4 among them) at a lone row and at a full block
    followed by a one-row block (rows 1 and 257) by the staged and the direct path of params and of grad_params (stride P
    and P + 3, independently), with a mask and an index (repeats, entries outside the store) and without, with value
    clipping and without: ``stats``, ``partials``, ``grad_params``, ``grad_value``, ``count``, the bands and the inputs."""
    for rows in (1, 257):
        for pad_in in (0, 3):
            for pad_out in (0, 3):
                p = Problem(rows, M, seed=3000 * rows + 100 * M + 10 * pad_in + pad_out, pad_in=pad_in, pad_out=pad_out)
                for clip_value in (False, True):
                    for variant in (dict(), dict(valid="some", index="wild")):
                        want = p.check((rows, M, pad_in, pad_out), clip_value=clip_value, **variant)
                if rows > 1:
                    assert np.isfinite(want["stats"]).all() and want["stats"][0] > 100 and want["stats"][1] > 0


WIDE = {"finite-ratios": dict(hostile_u=False, move=300.0), "ratios-0-and-inf": dict(hostile_u=False, move=800.0),
        "hostile-u": dict(hostile_u=True, move=800.0)}


@pytest.mark.parametrize("regime", list(WIDE))
@pytest.mark.parametrize("M", [3, 8, 19])
def test_the_wide_regime_equals_the_definition_on_every_byte(M, regime):
    """257 rows of `draw_wide_minibatch`: `wide_params` (w_j exactly 0), advantages and returns of the kinds normal / +-0 /
    tiny 1e-30 / huge 1e30 / subnormal 1e-41, ``clip`` in {0.2, 0}, and ``old_log_prob`` moved in every fourth row by up to
    +-300 (ratios from 1e-130 to 1e130: every sum stays a number, and the statistics are compared as numbers) or by up to
    +-800 (ratios of exactly 0 and +inf; +inf times an advantage of 0 is a NaN in the policy loss, times a negative one
    +inf); and, in the third regime, a stored ``u`` that saturates the tanh, is +-1e30, +-inf, NaN or a subnormal.  Every
    byte equals the definition's (a NaN is 0x7FC00000 / 0x7FF8000000000000 in both)."""
    rows = 257
    for pad in (0, 3):
        p = Problem(rows, M, seed=4000 + 100 * M + 10 * pad + list(WIDE).index(regime), pad_in=pad, pad_out=pad, wide=WIDE[regime])
        h = p.host
        assert zero_probability_rows(h["params"], M).any()
        assert all(is_subnormal(h[k][:rows]).sum() >= 10 and (h[k][:rows] == 0.0).sum() >= 10 and (np.abs(h[k][:rows]) > 1e28).sum() >= 10
                   for k in ("advantage", "returns"))
        for clip in (0.2, 0.0):
            for variant in (dict(), dict(valid="some", index="wild", clip_value=True)):
                p.check(("wide", M, pad, clip), clip=clip, **variant)
                out = p.definition(clip=clip, **variant)
                live, gp, stats = out["live"], out["grad_params"], out["stats"]
                assert np.isfinite(gp[live]).all(1).any() and (gp[live] != 0.0).any() and np.isfinite(stats[[4, 5]]).all()
                if regime == "finite-ratios" and not variant:   # (a wild index pairs a row with another row's stored entry)
                    assert np.isfinite(stats).all() and np.isfinite(out["partials"]).all()
                    assert clip != 0.0 or stats[7] >= 1.0 - 1e-15, "clip = 0: every ratio but an exact 1 lies outside"
                if regime != "finite-ratios" and not variant:
                    assert (live & (out["ratio"] == 0.0)).any() and (live & np.isposinf(out["ratio"])).any()
                if regime == "hostile-u":
                    assert np.isnan(gp[live]).any() and np.isnan(stats[2:]).any()


def test_bases_off_16_bytes_take_the_direct_path_and_aligned_ones_the_staged():
    """Stride P = 9 floats with the per-row blocks entered one row further on (36 bytes): neither base is 16-byte aligned;
    entered four rows further on (144 bytes) both are again."""
    p = Problem(301, 1, seed=7)
    for lo in (1, 4):
        assert (p.blocks["params"].t[lo:].data_ptr() % 16 == 0) == (lo == 4)
        for variant in (dict(), dict(valid="some"), dict(valid="some", clip_value=True)):
            p.check(("lo", lo), lo=lo, **variant)


def test_a_fold_lane_with_more_than_one_tile_and_a_last_tile_of_one_row():
    rows = 256 * 257 + 1
    p = Problem(rows, 2, seed=8)
    want = p.check("large", valid="some", index="perm", clip_value=True)
    assert want["stats"][0] == p.host["valid_some"][:rows].sum() and want["partials"][-1][0] in (0.0, 1.0)
    p.check("large, dense")


class FoldAlone:
    """FOLD by itself (``flags=PPO_FOLD``) over a ``partials`` block that the test wrote: ``partials``, ``stats`` and ``count``
    lie between guard bands, and every pointer that FOLD does not read is NULL, which the entry point accepts.  `fold`
    returns the names of the blocks and bands that differ from what the call has to leave: ``stats`` as
    `tile_tree_stats` gives it, everything else as it was."""

    def __init__(self, partials: np.ndarray):
        self.host = {"partials": np.ascontiguousarray(partials, dtype=np.float64), "stats": poisoned((_abi.PPO_STATS,), np.float64),
                     "count": poisoned((_abi.PPO_COUNT_WORDS,), np.int32)}
        self.tiles = self.host["partials"].shape[0]
        self.blocks = {name: Banded(a) for name, a in self.host.items()}
        self.want = tile_tree_stats(self.host["partials"])

    def fold(self, rows: int) -> list:
        assert -(-rows // 256) == self.tiles
        b = self.blocks
        b["stats"].raw.fill_(FILL)
        d = _abi.PpoDesc(partials=b["partials"].t.data_ptr(), stats=b["stats"].t.data_ptr(), count=b["count"].t.data_ptr(),
                         param_stride=10, grad_stride=10, n_src=rows, n_modes=2, rows=rows, flags=_abi.PPO_FOLD, **COEFS)
        d.lo[:], d.hi[:], d.log_span[:] = LO, HI, LOG_SPAN
        device_ppo_loss(d, DEV)
        torch.cuda.synchronize()
        want = {**self.host, "stats": self.want}
        return [name for name, blk in b.items() if not same_bits(blk.t, want[name])] + \
            [f"band of {name}" for name, blk in b.items() if not blk.bands_intact()]


@pytest.mark.parametrize("tiles", FOLD_TILES)
def test_the_fold_alone_is_the_tile_tree_in_every_class_of_tiles_per_lane(tiles):
    """256 to 4096 tiles, either side of every step of the fold's tiles per lane (1, 2, 4, 8, 16), with the last tile full
    and holding one row.  The data (`draw_partials`) tells the tree from the left-to-right sum and from a lane that adds
    its tiles one after the other: `telling_partials` asserts that before anything runs.  Only ``stats`` changes."""
    f = FoldAlone(telling_partials(tiles, seed=tiles))
    assert (f.host["partials"][:, 0] == 0).any() and np.isfinite(f.want).all() and f.want[0] > 0
    for rows in (256 * tiles, 256 * tiles - 255):
        assert f.fold(rows) == [], (tiles, rows)


NEG_ZERO_BITS = 0x8000000000000000
ODD_NAN = np.array([0xFFF4000000000123], dtype=np.uint64).view(np.float64)[0]   # signalling, signed, with a payload
# ((column, value) pairs written into tile 0, pairs written into the last tile); columns 2..6 are the five sums
NON_FINITE = ((((3, np.inf),), ((2, ODD_NAN),)),
              (((4, ODD_NAN),), ((5, np.inf),)),
              (((6, np.inf),), ((6, -np.inf),)),
              ((), ((2, -ODD_NAN), (6, np.inf))))


@pytest.mark.parametrize("tiles", [512, 513, 1024, 2048, 2049, 4096])
def test_signed_zeros_and_non_finite_values_through_the_fold_alone(tiles):
    """Five sum columns of -0.0 under a positive count: where the tiles fill the tree (512, 1024, 2048, 4096) no +0.0 is ever
    added and the five means are -0.0; at 513 and 2049 the definition's padding makes them +0.0.  Then an odd NaN or an
    infinity in the last tile and another in tile 0, and +inf against -inf in one column: every NaN comes out as
    0x7FF8000000000000, whichever operand or operation made it."""
    zeros = np.zeros((tiles, 7))
    zeros[:, 0], zeros[:, 2:] = 3.0, -0.0
    f = FoldAlone(zeros)
    bits = f.want.view(np.uint64)
    assert f.want[0] == 3.0 * tiles and all(bits[3:] == (NEG_ZERO_BITS if tiles & (tiles - 1) == 0 else 0))
    assert f.fold(256 * tiles) == [], (tiles, "signed zeros")
    for case, (first, last) in enumerate(NON_FINITE):
        p = draw_partials(np.random.default_rng(10 * tiles + case), tiles)
        for col, x in first:
            p[0, col] = x
        for col, x in last:
            p[-1, col] = x
        f = FoldAlone(p)
        hit = sorted({col for col, _ in first + last})
        assert np.isfinite(f.want[:2]).all() and not np.isfinite(f.want[[c + 1 for c in hit]]).any() and np.isnan(f.want).any()
        assert all(w == 0x7FF8000000000000 for w in f.want.view(np.uint64)[np.isnan(f.want)])
        assert f.fold(256 * tiles - 255) == [], (tiles, "non-finite", case)


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("rows", [131_073, 262_145, 524_289])
def test_whole_calls_at_the_first_row_count_of_four_eight_and_sixteen_tiles_per_fold_lane(rows, dense):
    """COUNT, MAIN and FOLD in one call at 513, 1025 and 2049 tiles (a last tile of one row, a tree half padding): with a
    mask, a permutation and value clipping, and dense."""
    p = Problem(rows, 2, seed=rows % 1000)
    assert p.tiles == rows // 256 + 1 and padded_tiles(p.tiles) == 2 * (p.tiles - 1)
    if dense:
        want = p.check("large, dense")
        assert want["stats"][0] == rows
    else:
        want = p.check("large", valid="some", index="perm", clip_value=True)
        assert want["stats"][0] == p.host["valid_some"][:rows].sum() and want["partials"][-1][0] in (0.0, 1.0)
    assert same_bits(tile_tree_stats(want["partials"]), want["stats"])


def test_the_phases_apart_equal_the_one_call_and_a_second_call_the_first():
    p = Problem(1000, 9, seed=9)
    kw = dict(valid="some", index="wild", clip_value=True)
    want = p.check("one call", **kw)
    torch.cuda.synchronize()
    first = {name: p.blocks[name].raw.clone() for name in p.blocks}
    p.poison()
    for flag in (_abi.PPO_COUNT, _abi.PPO_MAIN, _abi.PPO_FOLD):
        p.call(flags=flag, **kw)
    assert p.differences(want) == []
    assert all(same_bits(p.blocks[name].raw, first[name]) for name in p.blocks)
    p.call(**kw)
    torch.cuda.synchronize()
    assert all(same_bits(p.blocks[name].raw, first[name]) for name in p.blocks), "the same inputs twice give the same bytes"
    # a phase alone writes its own blocks only
    p.poison()
    p.call(flags=_abi.PPO_COUNT, **kw)
    only_count = {name: poisoned(p.host[name].shape, p.host[name].dtype) for name in OUTPUTS}
    only_count["count"] = want["count"]
    assert p.differences(only_count) == []
    p.poison()
    p.call(flags=_abi.PPO_COUNT)   # neither a mask nor an index: nothing is launched
    assert p.differences({name: poisoned(p.host[name].shape, p.host[name].dtype) for name in OUTPUTS}) == []


# ------------------------------------------------------------------------------------------------ 2. hostile rows
@pytest.mark.parametrize("pad", [0, 3])
def test_hostile_rows_reach_numbers_only(pad):
    """NaN, +-inf and +-1e30 in params, value, advantage, returns, old_log_prob and old_value, stored mode indices from -2^31
    to 2^31 - 1, indices outside the store: the bands are intact and every output equals the definition's on every byte (a
    NaN is 0x7FC00000 / 0x7FF8000000000000 in both).  Nothing here provokes a fault: it pins that data never forms an
    address without a check."""
    p = Problem(600, 9, seed=20 + pad, pad_in=pad, pad_out=pad, hostile=True)
    for variant in (dict(), dict(valid="some", index="wild"), dict(index="perm", clip_value=True), dict(clip_value=True, grads=False)):
        want = p.check("hostile", **variant)
        assert np.isnan(want["stats"][2:]).any()
    assert np.isnan(want["partials"]).any() and np.isfinite(want["partials"]).any()


# ------------------------------------------------------------------------------------------------ 3. through the stack
def test_ppo_loss_through_the_vector_env_the_head_the_rollout_buffer_and_a_network():
    """64 environments x 13 segments, four control steps driven by a two-layer network's sampled actions, then two epochs of
    two minibatches through ``PPOLoss.backward(rollout=, index=)``.  In the first epoch the gradient buffers and the
    statistics are the definition's on the same minibatch, byte for byte; the second runs without a host synchronisation
    and `PPOLoss.backward` leaves `memory_allocated` as it was."""
    n, T = 64, 4
    vec = WireEDMVectorEnv(make(DEV, n, "autoreset", "s13"), max_episode_steps=3000)
    modes = (5, 9, 13)
    head = PolicyHead(vec, modes=modes, bounds={"servo": (-0.2, 0.4), "ON_time": (1.0, 4.0), "OFF_time": (20.0, 60.0)}, seed=111)
    ppo = PPOLoss(head, clip=0.2, vf_coef=0.5, ent_coef=0.01, clip_value=0.3)
    assert ppo._native is not None
    buf = RolloutBuffer(vec, T, extras={"log_prob": torch.float32})
    gen = torch.Generator(device=DEV).manual_seed(5)
    D, Hd, P = len(vec.obs_names), 32, head.param_dim
    leaf = lambda *shape: (0.1 * torch.randn(*shape, generator=gen, device=DEV)).requires_grad_(True)   # noqa: E731
    W1, b1, Wp, bp, Wv, bv = leaf(D, Hd), leaf(Hd), leaf(Hd, P), leaf(P), leaf(Hd, 1), leaf(1)

    def net(obs):
        """(everything the graph keeps alive, params, value): held by the caller, `memory_allocated` is the same before and
        after a backward pass that frees the graph."""
        x = torch.nan_to_num(obs)
        x1 = x * 1e-3
        h = torch.tanh(x1 @ W1 + b1)
        v = h @ Wv + bv
        return (obs, x, x1, h, v), h @ Wp + bp, v.squeeze(1)

    obs, _ = vec.reset(seed=33)
    vec.env.state.workpiece_position = torch.linspace(10.4, 25.0, n, dtype=torch.float64, device=DEV)
    vec.env.state.wire_position = 10.0
    with torch.no_grad():
        for _ in range(T):
            _, params, value = net(obs)
            out = head.sample(params)
            nxt, reward, term, trunc, _ = vec.step(out.action)
            buf.add(obs, head.stored(out), value, reward, term, trunc, log_prob=out.log_prob)
            obs = nxt
        buf.finish(net(obs)[2])
    vec.env.check_errors()
    flat = buf.flat()
    with torch.no_grad():
        W1 += 0.05 * torch.randn(D, Hd, generator=gen, device=DEV)   # the policy has moved on: ratios other than 1
    perm = torch.randperm(T * n, device=DEV, generator=gen)
    parts = torch.tensor_split(perm, 2)
    kw = dict(modes=modes, lo=head._lo, hi=head._hi, log_span=head._log_span, clip=0.2, vf_coef=0.5, ent_coef=0.01, clip_value=0.3)
    held = []   # (what the loss keeps of a call until its next one stays alive here, so that the second epoch frees nothing either)
    for idx in parts:   # the first epoch: against the definition
        keep = net(flat["obs"][idx])
        held.append(keep)
        stats = ppo.backward(keep[1], keep[2], rollout=buf, index=idx)
        B = idx.shape[0]
        want = ppo_loss_definition(keep[1].detach(), keep[2].detach(), index=idx, u=flat["action.u"], mode_index=flat["action.mode_index"],
                                   old_log_prob=flat["log_prob"], advantage=flat["advantage_norm"], returns=flat["returns"],
                                   old_value=flat["value"], valid=flat["valid"], **kw)
        assert same_bits(ppo._grad[: B * P].view(B, P), want["grad_params"]) and same_bits(ppo._grad[B * P: B * (P + 1)], want["grad_value"])
        assert same_bits(stats.tensor, want["stats"]) and float(stats.n) == float(flat["valid"][idx].sum()) > 0
        assert float(stats.n_bad) == 0 and float(stats.clip_fraction) >= 0 and np.isfinite(want["stats"]).all()
    assert float(W1.grad.abs().sum()) > 0 and bool(W1.grad.isfinite().all()) and float(Wv.grad.abs().sum()) > 0
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for idx in parts:   # the second epoch: no synchronisation, no allocation
            keep = net(flat["obs"][idx])
            held.append(keep)
            before = torch.cuda.memory_allocated()
            stats = ppo.backward(keep[1], keep[2], rollout=buf, index=idx)
            after = torch.cuda.memory_allocated()
            assert after == before, (before, after)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        gc.enable()
    assert stats.tensor.data_ptr() == ppo.stats.tensor.data_ptr() and stats.tensor.device.type == "cuda"
    # loss(): the same gradients, scaled by what is upstream of the scalar
    for t in (W1, b1, Wp, bp, Wv, bv):
        t.grad = None
    keep = net(flat["obs"][parts[0]])
    ppo.backward(keep[1], keep[2], rollout=buf, index=parts[0])
    direct = W1.grad.clone()
    W1.grad = None
    keep = net(flat["obs"][parts[0]])
    (2.0 * ppo.loss(keep[1], keep[2], rollout=buf, index=parts[0])).backward()
    assert same_bits(W1.grad, 2.0 * direct), "a factor of two is exact"


# ------------------------------------------------------------------------------------------------ 4. on a side stream
def test_ppo_loss_behind_the_gate():
    """257 rows (a block of 256 and a block with one live lane) of 9 modes with a mask and an index, so that COUNT (two
    launches), MAIN and FOLD all run; ``params`` is the gated input.  The control is a twin problem reading the same
    ``params`` on the default stream."""
    rows, M = 257, 9
    kw = dict(valid="some", index="wild", clip_value=True)
    p, q = (Problem(rows, M, seed=30) for _ in range(2))
    warm = Problem(rows, M, seed=31)
    warm.call(**kw)
    gate = Gate(seconds_on(torch.cuda.default_stream(), lambda: warm.call(**kw)))
    q.blocks["params"] = p.blocks["params"]
    params_b = random_params(np.random.default_rng(300), rows, M, 0)
    dev_b = torch.from_numpy(params_b).to(DEV)
    p.host["params"] = params_b
    want_b, want_a = p.expect(p.definition(**kw), index="wild", valid="some"), q.expect(q.definition(**kw), index="wild", valid="some")
    differ = ("grad_params", "partials", "stats")   # (the count words follow the mask and the index alone, grad_value the values)
    assert all(want_a[name].tobytes() != want_b[name].tobytes() for name in differ)
    p.poison()
    q.poison()
    gated(gate, lambda: p.blocks["params"].t.copy_(dev_b), lambda: p.call(**kw), lambda: q.call(**kw))
    assert p.differences(want_b) == [], "wedm_ppo_loss behind the gate"   # outputs, inputs (params holds B), every guard band
    assert all(b.bands_intact() for b in q.blocks.values())
    check_control(all(same_bits(q.blocks[name].t, want_a[name]) for name in OUTPUTS),
                  any(same_bits(q.blocks[name].t, want_b[name]) for name in differ), gate, "wedm_ppo_loss")
