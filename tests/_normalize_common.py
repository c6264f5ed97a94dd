"""What tests/test_normalize_host.py (the definition, on the host) and tests/test_normalize.py (the kernels, on the MI355X)
share: the column kinds a running moment has to survive, and comparison on every byte.  TEST SEAM ONLY."""
from __future__ import annotations

import numpy as np
import torch

# float32 columns: unit normal; a small spread on a large offset (where E[x^2] - E[x]^2 cancels); a constant; a 0 / 1 flag;
# values near the bottom and the top of float32's range; a spread of 1 on 20 000
COLUMN_KINDS = ("normal", "offset", "constant", "flag", "tiny", "huge", "narrow")


def columns(rng: np.random.Generator, n: int, d: int = len(COLUMN_KINDS)) -> np.ndarray:
    """``[d, n]`` float32, row c of kind ``COLUMN_KINDS[c % 7]``."""
    make = {
        "normal": lambda: rng.normal(size=n),
        "offset": lambda: 1e6 + rng.uniform(0.0, 8.0, n),
        "constant": lambda: np.full(n, 293.15),
        "flag": lambda: rng.integers(0, 2, n).astype(np.float64),
        "tiny": lambda: 1e-30 * rng.normal(size=n),
        "huge": lambda: 1e30 * rng.normal(size=n),
        "narrow": lambda: rng.uniform(20000.0, 20001.0, n),
    }
    return np.stack([make[COLUMN_KINDS[c % len(COLUMN_KINDS)]]().astype(np.float32) for c in range(d)])


def same_bits(a, b) -> bool:
    """Equal in shape, type and every byte (NaN payloads and signed zeros count)."""
    a = a.detach().cpu().contiguous() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    b = b.detach().cpu().contiguous() if torch.is_tensor(b) else torch.from_numpy(np.ascontiguousarray(b))
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)))
