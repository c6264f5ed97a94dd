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


def random_params(rng: np.random.Generator, rows: int, M: int, width: int = 0) -> np.ndarray:
    """float32 ``[rows, 8 + M + width]``: |mean| <= 3, log_std in [-3, 1], logits in [-5, 5]; the ``width`` padding columns NaN."""
    p = np.full((rows, 8 + M + width), np.nan, dtype=np.float32)
    p[:, 0:4] = rng.uniform(-3.0, 3.0, (rows, 4))
    p[:, 4:8] = rng.uniform(-3.0, 1.0, (rows, 4))
    p[:, 8: 8 + M] = rng.uniform(-5.0, 5.0, (rows, M))
    return p


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
