"""The rows of a rollout dealt into minibatches by a seeded permutation on the device.

Which rows go into which minibatch of an epoch is one call of `wedm_minibatch_index` (include/wedm_hip.h, which holds the
definition): a function of the rollout's ``valid`` block, the number of parts, a seed and the number of the draw alone, in
integers, so that it has the same bits on every device and a checkpoint carries it as three numbers.  The live rows are
spread evenly over the parts (their counts differ by at most one) and come first in every part; the dead ones -- the steps
after a done one -- fill the parts up to the static sizes of ``torch.tensor_split``.  It is a keyed bijection, not a
uniformly random permutation.

`minibatch_index_reference` is that definition on host data in NumPy: the path of CPU devices (the oracle-backend stacks of
the tests) and what the kernels are checked against, byte for byte.  `MinibatchSampler` owns the index and the workspace.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from . import _abi
from .randomize import philox4x32_10

TILE, MAX_ROWS, MAX_PARTS = _abi.MB_TILE, _abi.MB_MAX_ROWS, _abi.MB_MAX_PARTS
COUNT, OFFSETS, SCATTER = _abi.MB_COUNT, _abi.MB_OFFSETS, _abi.MB_SCATTER
ROUNDS = 8
_U32 = np.uint32


def check_shape(rows: int, n_parts: int) -> Tuple[int, int]:
    """``rows`` and ``n_parts`` as ints, or ValueError with the header's conditions."""
    rows, n_parts = int(rows), int(n_parts)
    if not 1 <= rows <= MAX_ROWS:
        raise ValueError(f"minibatch_index: rows must lie in [1, {MAX_ROWS}], got {rows}")
    if not 1 <= n_parts <= min(rows, MAX_PARTS):
        raise ValueError(f"minibatch_index: n_parts must lie in [1, min(rows, {MAX_PARTS})], got {n_parts} for {rows} rows")
    return rows, n_parts


def part_bounds(rows: int, n_parts: int) -> Tuple[np.ndarray, np.ndarray]:
    """(off, cnt), int64 ``[n_parts]``: where part p starts in ``index`` and how many rows it holds -- the offsets and sizes
    of ``torch.tensor_split(index, n_parts)``."""
    p = np.arange(n_parts, dtype=np.int64)
    return p * (rows // n_parts) + np.minimum(p, rows % n_parts), -(-(rows - p) // n_parts)


def keys(seed: int, draw: int) -> np.ndarray:
    """K: uint32 ``[8]``, the two Philox blocks of a draw."""
    seed, draw = int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    blocks = [philox4x32_10((draw & 0xFFFFFFFF, draw >> 32, 0, _abi.MB_STREAM0 + c), key) for c in range(2)]
    return np.array([int(w) for block in blocks for w in block], dtype=_U32)


def _mix(x: np.ndarray) -> np.ndarray:
    x = x ^ (x >> _U32(16))
    x = x * _U32(0x85EBCA6B)
    x = x ^ (x >> _U32(13))
    x = x * _U32(0xC2B2AE35)
    return x ^ (x >> _U32(16))


def bijection(x: np.ndarray, bits: int, K: np.ndarray) -> np.ndarray:
    """E of the header on uint32 values below ``2 ** bits``: eight Feistel rounds over halves of ``bits >> 1`` (low) and the
    remaining (high) bits."""
    hl = bits >> 1
    hh = bits - hl
    mask_lo, mask_hi = _U32((1 << hl) - 1), _U32((1 << hh) - 1)
    x = np.asarray(x, dtype=_U32)
    lo, hi = x & mask_lo, x >> _U32(hl)
    with np.errstate(over="ignore"):
        for i in range(0, ROUNDS, 2):
            hi = hi ^ (_mix(lo ^ K[i]) & mask_hi)
            lo = lo ^ (_mix(hi ^ K[i + 1]) & mask_lo)
    return (hi << _U32(hl)) | lo


def walk(V: int, K: np.ndarray, with_steps: bool = False):
    """PI of the header: the permutation of ``[0, V)`` as a uint32 array (and, with ``with_steps``, the applications of E
    every element took)."""
    bits = int(V - 1).bit_length() if V > 1 else 0
    x = bijection(np.arange(V, dtype=_U32), bits, K)
    steps = np.ones(V, dtype=np.int64)
    out = np.flatnonzero(x >= V)
    while out.size:
        x[out] = bijection(x[out], bits, K)
        steps[out] += 1
        out = out[x[out] >= V]
    return (x, steps) if with_steps else x


def minibatch_index_reference(valid, n_parts: int, seed: int, draw: int, *, rows: Optional[int] = None
                              ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The definition of `wedm_minibatch_index` (include/wedm_hip.h) on host data.  ``valid``: ``[rows]`` (any shape, read
    flat) of uint8 or bool, a row is live iff its entry is not zero; or None with ``rows`` given: every row is live.
    Returns ``index`` (int64 ``[rows]``), ``count`` (int64 ``[2]``: live, dead), ``tile_counts`` and ``tile_base`` (int32
    ``[ceil(rows / 1024)]``)."""
    if valid is None:
        if rows is None:
            raise ValueError("minibatch_index: without a valid block the number of rows is needed")
        live = np.ones(int(rows), dtype=bool)
    else:
        live = np.asarray(valid).reshape(-1) != 0
        if rows is not None and int(rows) != live.shape[0]:
            raise ValueError(f"minibatch_index: valid holds {live.shape[0]} rows, not {rows}")
    R, n = check_shape(live.shape[0], n_parts)
    tiles = -(-R // TILE)
    padded = np.zeros(tiles * TILE, dtype=np.int64)
    padded[:R] = live
    tile_counts = padded.reshape(tiles, TILE).sum(axis=1)
    tile_base = np.cumsum(tile_counts) - tile_counts
    V = int(tile_counts.sum())
    live_below = np.cumsum(live) - live   # k(r) for a live row; r - k is q(r) for a dead one
    pos = np.empty(R, dtype=np.int64)
    pos[live] = walk(V, keys(seed, draw))[live_below[live]]
    pos[~live] = V + (np.arange(R)[~live] - live_below[~live])
    off, _ = part_bounds(R, n)
    index = np.empty(R, dtype=np.int64)
    index[off[pos % n] + pos // n] = np.arange(R, dtype=np.int64)
    return index, np.array([V, R - V], dtype=np.int64), tile_counts.astype(np.int32), tile_base.astype(np.int32)


def device_minibatch_index(desc: "_abi.MbDesc", device) -> None:
    """`wedm_minibatch_index` on ``device`` and torch's current stream, for callers that hold no environment."""
    from . import _lib

    _lib.call_stateless(_lib.load().wedm_minibatch_index, torch.device(device), C.byref(desc))


class MinibatchSampler:
    """``MinibatchSampler(buf, n_parts, seed=0)``: the minibatches of the epochs over a `RolloutBuffer`, one
    `wedm_minibatch_index` per epoch.

    ``index`` (int64 ``[T * N]``), ``count`` (int64 ``[2]``: live rows, dead rows) and the workspace are allocated here, once;
    `draw` allocates nothing and never synchronises with the host.  The permutation of draw number ``d`` is a function of
    the buffer's ``valid`` block, ``n_parts``, ``seed`` and ``d``; `draws` is the number of the next one.  On a CPU device
    every call runs `minibatch_index_reference`."""

    def __init__(self, buf, n_parts: int, seed: int = 0):
        rows = int(buf.num_steps) * int(buf.num_envs)
        if rows > MAX_ROWS:
            raise ValueError(f"MinibatchSampler: a buffer of {rows} rows; the call takes at most {MAX_ROWS}")
        self.buf, self.device, self.rows = buf, buf.device, rows
        self._set(n_parts, seed, 0)
        self._native = None
        if self.device.type == "cuda":
            native = getattr(buf, "_native", None)
            self._native = native.minibatch_index if hasattr(native, "minibatch_index") else \
                (lambda d: device_minibatch_index(d, self.device))
        kw = dict(device=self.device)
        tiles = -(-rows // TILE)
        self.index = torch.zeros(rows, dtype=torch.int64, **kw)
        self.count = torch.zeros(2, dtype=torch.int64, **kw)
        self._tile_counts = torch.zeros(tiles, dtype=torch.int32, **kw)
        self._tile_base = torch.zeros(tiles, dtype=torch.int32, **kw)
        self._valid = buf.computed["valid"]
        assert self._valid.dtype == torch.uint8 and self._valid.is_contiguous() and self._valid.numel() == rows

    def _set(self, n_parts, seed, draws) -> None:
        _, n = check_shape(self.rows, n_parts)
        seed, draws = int(seed), int(draws)
        if not 0 <= seed < 2 ** 64 or not 0 <= draws < 2 ** 64:
            raise ValueError("MinibatchSampler: seed and draws are unsigned 64-bit numbers")
        self.n_parts, self.seed, self.draws = n, seed, draws
        off, cnt = part_bounds(self.rows, n)
        self._bounds = tuple((int(o), int(o + c)) for o, c in zip(off, cnt))
        self._parts = None  # the views of `index`, made by the first draw after a change of n_parts

    # ------------------------------------------------------------------ the call
    def draw(self) -> Tuple[torch.Tensor, ...]:
        """One `wedm_minibatch_index` on torch's current stream over the buffer's own ``valid`` block: the ``n_parts`` int64
        views of `index`, valid until the next `draw`, for ``net(rollout=buf, index=idx)`` and
        ``PPOLoss.backward(..., rollout=buf, index=idx)``.  Needs a finished buffer (`RolloutBuffer.finish` and no `add`
        since)."""
        if not self.buf._finished:
            raise ValueError("MinibatchSampler.draw: the buffer is not finished: call finish() first")
        if self._native is not None:
            self._native(_abi.MbDesc(valid=self._valid.data_ptr(), index=self.index.data_ptr(), count=self.count.data_ptr(),
                                     tile_counts=self._tile_counts.data_ptr(), tile_base=self._tile_base.data_ptr(),
                                     seed=self.seed, draw=self.draws, rows=self.rows, n_parts=self.n_parts, flags=0))
        else:
            index, count, tile_counts, tile_base = self.expected(self._valid.cpu().numpy(), self.draws)
            for mine, host in ((self.index, index), (self.count, count), (self._tile_counts, tile_counts), (self._tile_base, tile_base)):
                mine.copy_(torch.from_numpy(host))
        self.draws += 1
        if self._parts is None:
            self._parts = tuple(self.index[lo:hi] for lo, hi in self._bounds)
        return self._parts

    def expected(self, valid, draw: int):
        """The host values of draw number ``draw`` over ``valid`` (an array or a tensor of ``rows`` entries, or None: every
        row live): what `minibatch_index_reference` returns for this sampler's ``n_parts`` and ``seed``."""
        if torch.is_tensor(valid):
            valid = valid.detach().cpu().numpy()
        return minibatch_index_reference(valid, self.n_parts, self.seed, draw, rows=self.rows)

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self) -> Dict[str, Any]:
        """``seed``, ``n_parts`` and ``draws``: all a permutation depends on besides the buffer's ``valid`` block."""
        return {"seed": self.seed, "n_parts": self.n_parts, "draws": self.draws}

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        """Takes the dict's seed, number of parts and draw number; refuses (and then changes nothing) a number of parts that
        this sampler's buffer cannot be cut into."""
        self._set(sd["n_parts"], sd["seed"], sd["draws"])
