"""What tests/test_wire_profile_host.py (the torch / NumPy path) and tests/test_wire_profile.py (MI355X, the kernel) share:
the definition of a wire profile (include/wedm_hip.h, `wedm_wire_profile`) written out independently of
sparc_amd/profile.py, and the quad-interleaved wire block built from per-environment cells.  TEST SEAM ONLY.

The reference sums with `math.fsum`, which returns the correctly rounded sum of its inputs whatever their order; over the
temperatures of the tests (finite, in [1, 65536), at most 2^11 per mean) the float64 sum is exact in every order (the header's
argument), so the sequential float64 sum of the definition, NumPy's pairwise one and the kernel's tree all equal it."""
from __future__ import annotations

import math

import numpy as np

FIXED = 4   # ZONE_MEAN, WIRE_MEAN, WIRE_MAX, HOT_CELL


def mean32(cells) -> np.float32:
    """``cells``: a list of Python floats holding float32 values."""
    return np.float32(np.float64(math.fsum(cells)) / np.float64(len(cells)))


def bin_edges(n: int, bins: int):
    out = []
    for b in range(bins):
        lo = (b * n) // bins
        out.append((lo, max(lo + 1, ((b + 1) * n) // bins)))
    return out


def reference_column(t: np.ndarray, az_start: int, az_end: int, bins: int) -> np.ndarray:
    """float32 [4 + 2 * bins]: the profile of one wire whose live cells are ``t`` (float32 [n])."""
    n = int(t.size)
    assert t.dtype == np.float32 and n >= 1
    cells = t.tolist()   # float32 values as Python floats: exact
    zone = cells[az_start:az_end] if 0 <= az_start < az_end <= n else cells
    top = max(cells)
    col = [mean32(zone), mean32(cells), top, cells.index(top)]   # list.index: the lowest index
    edges = bin_edges(n, bins)
    assert all(0 <= lo < hi <= n for lo, hi in edges)
    col += [max(cells[lo:hi]) for lo, hi in edges] + [mean32(cells[lo:hi]) for lo, hi in edges]
    return np.asarray(col, dtype=np.float32)


def reference_rows(cells: np.ndarray, n_seg, az_start, az_end, bins: int, env_ids=None) -> np.ndarray:
    """float32 [4 + 2 * bins, count] from ``cells`` float32 [num_envs, n_seg_max] (only ``cells[e, :n_seg[e]]`` is read);
    the geometry is an integer for all or one value per environment."""
    num_envs = cells.shape[0]
    n, zs, ze = (np.broadcast_to(np.asarray(x, dtype=np.int64), (num_envs,)) for x in (n_seg, az_start, az_end))
    ids = range(num_envs) if env_ids is None else [int(e) for e in env_ids]
    cols = [reference_column(np.ascontiguousarray(cells[e, : n[e]]), int(zs[e]), int(ze[e]), bins) for e in ids]
    return np.stack(cols, axis=1) if cols else np.zeros((FIXED + 2 * bins, 0), dtype=np.float32)


def pack(cells: np.ndarray, n_seg, stride: int, dead) -> np.ndarray:
    """The wire block float32 ``[quads][stride][4]`` of ``cells`` [num_envs, n_seg_max]: environment e's cells
    ``[0, n_seg[e])`` where the ABI puts them, and ``dead`` (a poison value) in EVERY other cell -- the cells from an
    environment's own n_seg up to n_seg_max, the last quad's padding, the columns [num_envs, stride)."""
    num_envs, n_max = cells.shape
    n = np.broadcast_to(np.asarray(n_seg, dtype=np.int64), (num_envs,))
    quads = (n_max + 3) // 4
    full = np.full((stride, quads * 4), dead, dtype=np.float32)
    for e in range(num_envs):
        full[e, : n[e]] = cells[e, : n[e]]
    return np.ascontiguousarray(full.reshape(stride, quads, 4).transpose(1, 0, 2))


def unpack(T: np.ndarray, num_envs: int, n_seg_max: int) -> np.ndarray:
    """``cells`` [num_envs, n_seg_max] of a wire block."""
    return np.ascontiguousarray(T.transpose(1, 0, 2).reshape(T.shape[1], -1)[:num_envs, :n_seg_max])


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())
