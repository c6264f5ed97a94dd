"""What tests/test_policy_head_host.py (the definition, on the host) and tests/test_policy_head.py (the kernels, on the MI355X)
share: seeded parameter rows, hostile rows, and the descriptor's constants.  TEST SEAM ONLY."""
from __future__ import annotations

import math

import numpy as np

from sparc_amd import _abi

LO = (-1.0, 0.0, 0.0, 0.0)          # the action space's bounds: servo, target_voltage, ON_time, OFF_time
HI = (1.0, 200.0, 5.0, 100.0)
LOG_SPAN = tuple(math.log(h - l) for l, h in zip(LO, HI))
MODES = {1: (9,), 2: (5, 13), 9: (1, 3, 5, 7, 9, 11, 13, 15, 17)}
CONSTS = dict(lo=LO, hi=HI, log_span=LOG_SPAN)
# every other mode count: the first M entries of a fixed permutation of 1..19 in which entry j is neither j nor j + 1, so that
# an index handed out as a mode (or a mode read one entry off) shows; MODES[1], MODES[2] and MODES[9] stay what they were
MODE_ORDER = (12, 19, 7, 15, 1, 10, 17, 3, 14, 6, 18, 2, 9, 16, 4, 11, 8, 13, 5)
assert sorted(MODE_ORDER) == list(range(1, 20)) and all(m not in (j, j + 1) for j, m in enumerate(MODE_ORDER))
MODES.update({M: MODE_ORDER[:M] for M in range(1, 20) if M not in MODES})
ALL_M = tuple(range(1, 20))
# the stored pre-squash values of the wide regime beside draws at the parameters: |u| = 20 and 400 (e = exp(-2|u|) is 4e-18
# and underflows to 0, and the action clamps to a bound), +-1e30, +-inf, NaN, and float32 subnormals
HOSTILE_U = (20.0, -20.0, 400.0, -400.0, 1e30, -1e30, np.inf, -np.inf, np.nan, 1e-41, -1e-41, 1.4e-45, -3e-39)


def random_params(rng: np.random.Generator, rows: int, M: int, width: int = 0) -> np.ndarray:
    """float32 ``[rows, 8 + M + width]``: |mean| <= 3, log_std in [-3, 1], logits in [-5, 5]; the ``width`` padding columns NaN."""
    p = np.full((rows, 8 + M + width), np.nan, dtype=np.float32)
    p[:, 0:4] = rng.uniform(-3.0, 3.0, (rows, 4))
    p[:, 4:8] = rng.uniform(-3.0, 1.0, (rows, 4))
    p[:, 8: 8 + M] = rng.uniform(-5.0, 5.0, (rows, M))
    return p


def wide_params(rng: np.random.Generator, rows: int, M: int, width: int = 0) -> np.ndarray:
    """float32 ``[rows, 8 + M + width]`` of the wide regime: |mean| <= 3, log_std in [-6, 2], and per row logits U(-1, 1) x
    10^U(0, 2.9) -- spreads of up to 1588, so that many ``w_j = exp(l_j - m)`` are exactly 0 (`portable_exp` returns 0 below
    -708); the ``width`` padding columns NaN."""
    p = np.full((rows, 8 + M + width), np.nan, dtype=np.float32)
    p[:, 0:4] = rng.uniform(-3.0, 3.0, (rows, 4))
    p[:, 4:8] = rng.uniform(-6.0, 2.0, (rows, 4))
    p[:, 8: 8 + M] = rng.uniform(-1.0, 1.0, (rows, M)) * 10.0 ** rng.uniform(0.0, 2.9, (rows, 1))
    return p


def zero_probability_rows(params: np.ndarray, M: int) -> np.ndarray:
    """The rows of ``params`` in which some logit lies more than 708 below the largest: ``w_j`` is exactly 0 there."""
    l = params[:, 8: 8 + M].astype(np.float64)
    return (l - l.max(1, keepdims=True) < -708.0).any(1)


def wide_stored(rng: np.random.Generator, params: np.ndarray, M: int):
    """`random_stored` with every third row's ``u`` holding one of `HOSTILE_U` in one component (row 0: in all four), and a
    mode index that names every logit in turn."""
    u, k = random_stored(rng, params, M)
    rows = params.shape[0]
    bad = np.array(HOSTILE_U, dtype=np.float32)
    hit = np.arange(0, rows, 3)
    u[hit, rng.integers(0, 4, hit.size)] = bad[np.arange(hit.size) % bad.size]
    u[0] = bad[[8, 6, 9, 2]]
    return u, (np.arange(rows) % M).astype(np.int32) if rows > 1 else k


def random_stored(rng: np.random.Generator, params: np.ndarray, M: int):
    """Stored actions for ``params``: u = mean + sigma * normal rounded to float32, a uniform mode index."""
    rows = params.shape[0]
    mu, ls = params[:, 0:4].astype(np.float64), params[:, 4:8].astype(np.float64)
    u = (mu + np.exp(ls) * rng.normal(size=(rows, 4))).astype(np.float32)
    return u, rng.integers(0, M, rows).astype(np.int32)


def make_hostile(rng: np.random.Generator, params: np.ndarray, M: int) -> np.ndarray:
    """``params`` with NaN, +-inf and +-1e30 scattered into a third of the rows' means, log-stds and logits (one value per
    hit row, some rows hit twice), and two rows hostile in every column."""
    p = params.copy()
    rows, P = p.shape[0], 8 + M
    bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], dtype=np.float32)
    for _ in range(2):
        hit = rng.choice(rows, rows // 3, replace=False)
        p[hit, rng.integers(0, P, hit.size)] = bad[rng.integers(0, bad.size, hit.size)]
    p[0, :P] = np.nan
    p[1, :P] = bad[np.arange(P) % bad.size]
    return p


def desc_consts(d: "_abi.HeadDesc", M: int) -> "_abi.HeadDesc":
    d.lo[:], d.hi[:], d.log_span[:] = LO, HI, LOG_SPAN
    d.modes[:M] = MODES[M]
    d.n_modes = M
    return d
