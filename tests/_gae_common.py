"""What tests/test_rollout_host.py (the definition, on the host) and tests/test_rollout.py (the kernels, on the MI355X)
share: rollouts whose environments are of the kinds a recurrence and a running moment have to survive, and flag bytes other
than 0 and 1.  TEST SEAM ONLY."""
from __future__ import annotations

import numpy as np

# per environment: unit normal; a small spread on a large offset; a constant; values near the bottom and the top of float32's
# range; float32 subnormals; zeros of either sign
GAE_KINDS = ("normal", "offset", "constant", "tiny", "huge", "subnormal", "zeros")
FLAG_BYTES = (0, 1, 2, 0x80, 0xFF)   # `terminated` / `truncated`: non-zero means set, in the kernel and in `torch_gae` alike
PAIRS = ((0.99, 0.95), (1.0, 1.0), (0.0, 0.5), (0.97, 0.0))   # (gamma, lam)


def kinds_of(N: int, kinds=GAE_KINDS):
    """The kind index of every environment in ``reward``, ``value`` and ``last_value``: cycling over the environments at three
    paces, so that the three blocks' kinds are independent of each other (all 7 x 7 pairs of the first two from N = 49)."""
    e, k = np.arange(N), len(kinds)
    return e % k, (e // k) % k, (e // 3) % k


def mixed(rng: np.random.Generator, T: int, which: np.ndarray, kinds=GAE_KINDS) -> np.ndarray:
    """float32 ``[T, N]``, column e of kind ``kinds[which[e]]``."""
    N = which.shape[0]
    make = {
        "normal": lambda: rng.normal(size=(T, N)),
        "offset": lambda: 1e6 + rng.uniform(0.0, 8.0, (T, N)),
        "constant": lambda: np.full((T, N), 293.15),
        "tiny": lambda: 1e-30 * rng.normal(size=(T, N)),
        "huge": lambda: 1e30 * rng.normal(size=(T, N)),
        "subnormal": lambda: 1e-41 * rng.normal(size=(T, N)),
        "zeros": lambda: 0.0 * rng.normal(size=(T, N)),
    }
    planes = np.stack([make[name]() for name in kinds])   # (every kind draws, whatever N is: one stream of numbers per shape)
    return planes[which, :, np.arange(N)].T.astype(np.float32)


def flag_bytes(rng: np.random.Generator, T: int, N: int, p: float) -> np.ndarray:
    """uint8 ``[T, N]``: set with probability ``p``, a set flag being one of the non-zero `FLAG_BYTES`."""
    return np.where(rng.random((T, N)) < p, rng.choice(np.array(FLAG_BYTES[1:], dtype=np.uint8), (T, N)), 0).astype(np.uint8)


def draw_mixed(rng: np.random.Generator, T: int, N: int, p: float = 0.1, kinds=GAE_KINDS):
    """``reward``, ``value`` ``[T, N]`` and ``last_value`` ``[N]`` of the environments' kinds, ``terminated`` / ``truncated``
    of `FLAG_BYTES`."""
    kr, kv, kl = kinds_of(N, kinds)
    return dict(reward=mixed(rng, T, kr, kinds), value=mixed(rng, T, kv, kinds), last_value=mixed(rng, 1, kl, kinds)[0],
                terminated=flag_bytes(rng, T, N, p), truncated=flag_bytes(rng, T, N, p))


def is_subnormal(a: np.ndarray) -> np.ndarray:
    """The float32 entries that are subnormal: an exponent field of 0 and a mantissa that is not."""
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return ((bits & 0x7F800000) == 0) & ((bits & 0x007FFFFF) != 0)
