"""What tests/test_ppo_loss_host.py (the definition, on the host) and tests/test_ppo_loss.py (the kernels, on the MI355X)
share: seeded minibatches whose rows reach every branch of the loss, the definition's keywords, and the tree over the
tiles as a plain recursion with the orders of addition it must be told from.  TEST SEAM ONLY."""
from __future__ import annotations

import numpy as np

from sparc_amd.policy_head import EVALUATE, policy_head_definition
from tests._policy_head_common import CONSTS, MODES, random_params, random_stored, wide_params, wide_stored

CLIP, CLIP_VALUE, VF_COEF, ENT_COEF = 0.2, 0.2, 0.5, 0.01
COEFS = dict(clip=CLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF)
STORED = ("u", "mode_index", "old_log_prob", "advantage", "returns", "old_value", "valid")


def draw_minibatch(rng: np.random.Generator, rows: int, M: int, pad: int = 0, p_invalid: float = 0.15, u_limit: float = 0.0):
    """``rows`` dense rows: params ``[rows, 8 + M + pad]`` (padding NaN), value, and the stored blocks at the sampling
    position of every row: u and a mode index drawn at the parameters, ``old_log_prob`` the definition's log-probability
    moved by up to +-0.5 (ratios on either side of a clip range of 0.2 and inside it), advantages of both signs,
    ``old_value`` up to 0.5 from the value (a value clip of 0.2 active on either side and not), returns around them, and
    ``valid`` zero with probability ``p_invalid``.  ``u_limit > 0`` keeps ``|u|`` below it."""
    params = random_params(rng, rows, M, pad)
    u, k = random_stored(rng, params, M)
    if u_limit:
        u = np.clip(u, -u_limit, u_limit)
    lp = policy_head_definition(EVALUATE, params, modes=MODES[M], u=u, mode_index=k, **CONSTS)["log_prob64"]
    value = rng.normal(size=rows).astype(np.float32)
    return {"params": params, "value": value, "u": u, "mode_index": k,
            "old_log_prob": (lp + rng.uniform(-0.5, 0.5, rows)).astype(np.float32),
            "advantage": rng.normal(size=rows).astype(np.float32),
            "returns": (value + rng.normal(size=rows)).astype(np.float32),
            "old_value": (value + rng.uniform(-0.5, 0.5, rows)).astype(np.float32),
            "valid": (rng.random(rows) >= p_invalid).astype(np.uint8)}


VALUE_KINDS = ("normal", "zero", "tiny", "huge", "subnormal")   # N(0,1) x 1, +-0, 1e-30, 1e30, 1e-41 (a float32 subnormal)


def mixed_values(rng: np.random.Generator, n: int, first: int = 0) -> np.ndarray:
    """float32 ``[n]``, entry i of kind ``VALUE_KINDS[(first + i) % 5]``: a unit normal times the kind's magnitude (times 0.0
    it is a zero with the normal's sign)."""
    scale = np.array([1.0, 0.0, 1e-30, 1e30, 1e-41])[(first + np.arange(n)) % len(VALUE_KINDS)]
    return (rng.normal(size=n) * scale).astype(np.float32)


def draw_wide_minibatch(rng: np.random.Generator, rows: int, M: int, pad: int = 0, p_invalid: float = 0.15, hostile_u: bool = True,
                        move: float = 800.0, u_limit: float = 0.0):
    """`draw_minibatch` in the wide regime: `wide_params`; ``u`` drawn at the parameters (``hostile_u``: `wide_stored`, with
    saturating, huge, infinite, NaN and subnormal entries; ``u_limit > 0`` keeps ``|u|`` below it); ``old_log_prob`` the
    definition's log-probability (where that is not finite: 0) moved by up to +-0.5, and in every fourth row by up to
    +-``move`` (at 800: ratios of exactly 0 and +inf); advantages and returns of `VALUE_KINDS`, out of step with each other."""
    params = wide_params(rng, rows, M, pad)
    u, k = wide_stored(rng, params, M) if hostile_u else random_stored(rng, params, M)
    if u_limit:
        u = np.clip(u, -u_limit, u_limit)
    lp = policy_head_definition(EVALUATE, params, modes=MODES[M], u=u, mode_index=k, **CONSTS)["log_prob64"]
    lp = np.where(np.abs(lp) < 1e30, lp, 0.0)   # (a NaN compares false)
    i = np.arange(rows)
    shift = np.where(i % 4 == 1, rng.uniform(-move, move, rows), rng.uniform(-0.5, 0.5, rows))
    shift = np.where(i % 16 == 1, move, np.where(i % 16 == 9, -move, shift))   # (the full move, either way, in every 16 rows)
    value = rng.normal(size=rows).astype(np.float32)
    return {"params": params, "value": value, "u": u, "mode_index": k,
            "old_log_prob": (lp + shift).astype(np.float32),
            "advantage": mixed_values(rng, rows), "returns": mixed_values(rng, rows, first=2),
            "old_value": (value + rng.uniform(-0.5, 0.5, rows)).astype(np.float32),
            "valid": (rng.random(rows) >= p_invalid).astype(np.uint8)}


def definition_kw(M: int, clip_value: bool = False, **coefs):
    return dict(modes=MODES[M], **CONSTS, **{**COEFS, **coefs}, clip_value=CLIP_VALUE if clip_value else None)


# ------------------------------------------------------------------------------------------------ the tree over the tiles
FOLD_TILES = (256, 257, 512, 513, 1000, 1024, 1025, 2048, 2049, 3000, 4095, 4096)   # either side of every tiles-per-lane class
_NAN64 = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]


def padded_tiles(tiles: int) -> int:
    """The smallest power of two that holds ``tiles``."""
    padded = 1
    while padded < tiles:
        padded *= 2
    return padded


def stats_of_roots(S: np.ndarray, vf_coef: float = VF_COEF, ent_coef: float = ENT_COEF) -> np.ndarray:
    """The eight ``stats`` words from the seven roots, by the header's formulas (a NaN: 0x7FF8000000000000)."""
    with np.errstate(all="ignore"):
        n = S[0]
        s = 1.0 / n if n > 0 else 0.0
        pl, vl, en = S[2] * s, S[3] * s, S[4] * s
        stats = np.array([n, S[1], (pl + vf_coef * vl) - ent_coef * en, pl, vl, en, S[5] * s, S[6] * s])
    return np.where(stats != stats, _NAN64, stats)


def tile_tree(partials: np.ndarray) -> np.ndarray:
    """The header's tree over the tile index, written as it reads and sharing nothing with `pairwise_sum`:
    ``tree(lo, hi) = tree(lo, mid) + tree(mid, hi)`` over the padded power of two, the lower index on the left; a leaf at or
    past ``tiles`` is +0.0 and is added like any other.  ``partials``: float64 ``[tiles, 7]``; returns the seven roots."""
    x = np.asarray(partials, dtype=np.float64)
    tiles, zero = x.shape[0], np.zeros(x.shape[1:])

    def tree(lo: int, hi: int) -> np.ndarray:
        if hi - lo == 1:
            return x[lo] if lo < tiles else zero
        mid = (lo + hi) // 2
        return tree(lo, mid) + tree(mid, hi)

    with np.errstate(all="ignore"):
        return tree(0, padded_tiles(tiles))


def tile_tree_stats(partials: np.ndarray, vf_coef: float = VF_COEF, ent_coef: float = ENT_COEF) -> np.ndarray:
    return stats_of_roots(tile_tree(partials), vf_coef, ent_coef)


def left_to_right_stats(partials: np.ndarray) -> np.ndarray:
    """What a fold that adds the tiles in their order, one after the other, would store: not the definition."""
    S = np.zeros(partials.shape[1])
    with np.errstate(all="ignore"):
        for row in np.asarray(partials, dtype=np.float64):
            S = S + row
    return stats_of_roots(S)


def lane_sequential_stats(partials: np.ndarray) -> np.ndarray:
    """What a fold whose 256 lanes each add their ``per`` consecutive tiles one after the other, and then form the tree over
    the lanes, would store: the definition up to two tiles per lane, and not from four on."""
    x = np.asarray(partials, dtype=np.float64)
    tiles, padded = x.shape[0], padded_tiles(x.shape[0])
    per = max(1, padded // 256)
    full = np.zeros((padded,) + x.shape[1:])
    full[:tiles] = x
    lanes = full.reshape(padded // per, per, -1)
    with np.errstate(all="ignore"):
        node = lanes[:, 0]
        for j in range(1, per):
            node = node + lanes[:, j]
    return tile_tree_stats(node)


def draw_partials(rng: np.random.Generator, tiles: int) -> np.ndarray:
    """A synthesised ``partials`` block ``[tiles, 7]``: LIVE an integer in 0..256 with every eighth tile or so empty, BAD a small
    integer, the five sums of either sign with magnitudes 10^U(-8, 8), so that the order of the additions shows in the
    low bits of every root."""
    p = np.empty((tiles, 7))
    p[:, 0] = np.where(rng.random(tiles) < 0.125, 0, rng.integers(0, 257, tiles))
    p[:, 1] = rng.integers(0, 4, tiles)
    p[:, 2:] = rng.choice((-1.0, 1.0), (tiles, 5)) * 10.0 ** rng.uniform(-8.0, 8.0, (tiles, 5))
    return p


def telling_partials(tiles: int, seed: int, tries: int = 5) -> np.ndarray:
    """`draw_partials` at the first of ``tries`` seeds whose data tells the definition's tree from the left-to-right sum and,
    where a lane holds four tiles or more, from the lane-sequential sum, in at least one ``stats`` word each."""
    for k in range(tries):
        p = draw_partials(np.random.default_rng(1000 * seed + k), tiles)
        want = tile_tree_stats(p).tobytes()
        if left_to_right_stats(p).tobytes() != want and (padded_tiles(tiles) < 1024 or lane_sequential_stats(p).tobytes() != want):
            return p
    raise AssertionError(f"{tries} draws of {tiles} tiles prove nothing: every order of the additions gives the tree's bits")
