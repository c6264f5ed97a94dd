"""What tests/test_ppo_loss_host.py (the definition, on the host) and tests/test_ppo_loss.py (the kernels, on the MI355X)
share: seeded minibatches whose rows reach every branch of the loss, and the definition's keywords.  TEST SEAM ONLY."""
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
