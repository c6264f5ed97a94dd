"""What tests/test_episode_log_host.py (the definition against a plain loop, on the host) and tests/test_episode_log.py (the
kernels against the definition, on the MI355X) share: problems of `wedm_episode_log` laid out in ONE byte arena -- every
block between guard bands, padding columns, bases on and off 16 bytes -- so that "every byte the call may write, and no
other" is one comparison of two buffers.  TEST SEAM ONLY."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from sparc_amd import _abi
from sparc_amd.episode_log import LAST, SUM_F32, SUM_F64, SUM_I32, episode_log_definition

GUARD = 64          # bytes between blocks
FILL = 0xA5
TILE = 256
NAN32 = np.array([0x7FC12345, 0xFFA00001], dtype=np.uint32).view(np.float32)   # NaNs with payloads, one of them signalling
NAN64 = np.array([0x7FF8DEADBEEF0001, 0xFFF4000000000123], dtype=np.uint64).view(np.float64)

# (kind, source dtype, rows): one, four and eight bytes with several rows, the three sums
SPEC = ((LAST, np.uint8, 2), (LAST, np.float32, 3), (LAST, np.float64, 2), (LAST, np.int64, 1),
        (SUM_F32, np.float32, 2), (SUM_F64, np.float64, 1), (SUM_I32, np.int32, 3))
# the limits: 32 planes, 96 rows in all
SPEC_MAX = tuple((k, dt, 3) for k, dt in ((LAST, np.uint8), (LAST, np.int32), (LAST, np.float64), (SUM_F32, np.float32),
                                          (SUM_F64, np.float64), (SUM_I32, np.int32), (LAST, np.float32), (SUM_I32, np.int32))) * 4
assert len(SPEC_MAX) == _abi.ELOG_MAX_PLANES and sum(s[2] for s in SPEC_MAX) == _abi.ELOG_MAX_ROWS
ACC = {SUM_F32: np.float64, SUM_F64: np.float64, SUM_I32: np.int64}


def finishing(rng, N: int, how: str) -> np.ndarray:
    """Who finishes: "none", "first", "last", "few" (about 3 %, at least two where there are two) or "all"."""
    f = np.zeros(N, dtype=bool)
    if how == "first":
        f[0] = True
    elif how == "last":
        f[-1] = True
    elif how == "few":
        f[rng.random(N) < 0.03] = True
        f[rng.integers(0, N, 2)] = True
    elif how == "all":
        f[:] = True
    else:
        assert how == "none"
    return f


def flags_from(rng, fin: np.ndarray, mask: Optional[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    """terminated / truncated bytes (any non-zero byte counts) whose OR over the live environments is ``fin``; environments
    the mask leaves out carry flags of their own, which must reach nothing."""
    N = fin.shape[0]
    which = rng.integers(0, 3, N)
    term = np.where(fin & (which != 1), rng.integers(1, 256, N), 0).astype(np.uint8)
    trunc = np.where(fin & (which != 0), rng.integers(1, 256, N), 0).astype(np.uint8)
    if mask is not None:
        out = mask == 0
        term[out] = rng.integers(0, 2, int(out.sum()))
    return term, trunc


class Problem:
    """One set of blocks for `wedm_episode_log` in one arena.  ``pad``: source columns past ``num_envs``; ``off16``: every
    base one element off a multiple of 16 bytes."""

    def __init__(self, rng, N: int, capacity: int, spec: Sequence = SPEC, pad: int = 0, off16: bool = False,
                 tile_offset: int = 0, n_tiles_total: Optional[int] = None, head0: int = 0, truncated: bool = True,
                 masked: bool = False):
        self.N, self.capacity, self.spec = int(N), int(capacity), tuple(spec)
        self.tiles = -(-self.N // TILE)
        self.tile_offset = int(tile_offset)
        self.ntt = self.tile_offset + self.tiles if n_tiles_total is None else int(n_tiles_total)
        self.layout: Dict[str, Tuple[int, np.dtype, tuple]] = {}
        self._init: Dict[str, np.ndarray] = {}
        self._size = GUARD
        self._off16 = off16
        S = self.N + pad

        def values(dt, shape):
            dt = np.dtype(dt)
            if dt.kind == "f":
                v = (rng.standard_normal(shape) * 100.0).astype(dt)
                nan = NAN32 if dt.itemsize == 4 else NAN64
                flat = v.reshape(-1)
                flat[rng.integers(0, flat.size, max(1, flat.size // 16))] = nan[0]
                flat[rng.integers(0, flat.size, max(1, flat.size // 16))] = nan[1]
                return v
            info = np.iinfo(dt)
            return rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)

        for p, (kind, dt, rows) in enumerate(self.spec):
            src = values(dt, (rows, S))
            if kind != LAST:   # sums stay finite and far from overflow
                src = (rng.integers(-1000, 1000, (rows, S)) if np.dtype(dt).kind == "i" else rng.standard_normal((rows, S)) * 10).astype(dt)
            self._add(f"src{p}", src)
            out_dt = dt if kind == LAST else ACC[kind]
            self._add(f"dst{p}", values(out_dt, (rows, self.capacity)))
            if kind != LAST:
                acc = (rng.integers(-10**12, 10**12, (rows, self.N)) if kind == SUM_I32 else rng.standard_normal((rows, self.N)) * 1e3)
                self._add(f"acc{p}", acc.astype(ACC[kind]))
        self._add("terminated", np.zeros(self.N, dtype=np.uint8))
        self.has_truncated, self.masked = truncated, masked
        if truncated:
            self._add("truncated", np.zeros(self.N, dtype=np.uint8))
        if masked:
            self._add("mask", np.ones(self.N, dtype=np.uint8))
        self._add("env_out", values(np.int64, (self.capacity,)))
        self._add("stamp_out", values(np.int64, (self.capacity,)))
        self._add("head", np.array([head0, -7], dtype=np.int64))
        self._add("tile_counts", rng.integers(0, 3, self.ntt).astype(np.int32))
        self.buf = np.full(self._size, FILL, dtype=np.uint8)
        for name, a in self._init.items():
            self.view(self.buf, name)[...] = a
        del self._init

    def _add(self, name: str, a: np.ndarray) -> None:
        elem = a.dtype.itemsize
        off = -(-self._size // 16) * 16 + (elem if self._off16 else 0)
        self.layout[name] = (off, a.dtype, a.shape)
        self._init[name] = a
        self._size = off + a.nbytes + GUARD

    def view(self, buf: np.ndarray, name: str) -> np.ndarray:
        off, dt, shape = self.layout[name]
        return buf[off: off + int(np.prod(shape)) * dt.itemsize].view(dt).reshape(shape)

    def set_flags(self, buf: np.ndarray, term: np.ndarray, trunc: Optional[np.ndarray], mask: Optional[np.ndarray]) -> None:
        self.view(buf, "terminated")[:] = term
        if self.has_truncated:
            self.view(buf, "truncated")[:] = trunc
        else:
            assert trunc is None
        if self.masked:
            self.view(buf, "mask")[:] = mask
        else:
            assert mask is None

    def define(self, buf: np.ndarray, stamp: int, env_id_offset: int = 0, flags: int = 0, part: Optional[Tuple[int, int]] = None) -> None:
        """`episode_log_definition` on the blocks of ``buf``, in place.  ``part = (first, count)``: the shard of that many
        environments from ``first`` (a multiple of 256) on, at its tile offset."""
        first, count = part or (0, self.N)
        assert first % TILE == 0
        v = lambda name: self.view(buf, name)   # noqa: E731
        planes = [(kind, v(f"src{p}")[:, first:], v(f"dst{p}"), None if kind == LAST else v(f"acc{p}")[:, first: first + count])
                  for p, (kind, _, _) in enumerate(self.spec)]
        # (a shard's accumulators are columns of the batch's: the definition writes through the slices)
        cut = lambda name: v(name)[first: first + count]   # noqa: E731
        episode_log_definition(planes, cut("terminated"), cut("truncated") if self.has_truncated else None,
                               cut("mask") if self.masked else None, v("env_out"), v("stamp_out"), v("head"), v("tile_counts"),
                               num_envs=count, env_id_offset=env_id_offset + first, stamp=stamp,
                               tile_offset=self.tile_offset + first // TILE, n_tiles_total=self.ntt, flags=flags)

    def desc(self, base: int, stamp: int, env_id_offset: int = 0, flags: int = 0,
             part: Optional[Tuple[int, int]] = None) -> "_abi.ElogDesc":
        """The descriptor of the same call on a copy of the arena at address ``base``.  A shard's accumulators are a block of
        their own in the ABI (``[rows][num_envs]``), so a shard is described only for single-row sums or the whole batch:
        the shard tests use `SPEC_SHARD`."""
        first, count = part or (0, self.N)
        at = lambda name: base + self.layout[name][0]   # noqa: E731
        d = _abi.ElogDesc(terminated=at("terminated") + first, truncated=at("truncated") + first if self.has_truncated else None,
                          mask=at("mask") + first if self.masked else None, env_out=at("env_out"), stamp_out=at("stamp_out"),
                          head=at("head"), tile_counts=at("tile_counts"), capacity=self.capacity,
                          env_id_offset=env_id_offset + first, stamp=stamp, n_planes=len(self.spec), num_envs=count,
                          tile_offset=self.tile_offset + first // TILE, n_tiles_total=self.ntt, flags=flags)
        for p, (kind, dt, rows) in enumerate(self.spec):
            q, eb = d.plane[p], np.dtype(dt).itemsize
            q.src, q.dst = at(f"src{p}") + first * eb, at(f"dst{p}")
            q.src_stride, q.n_rows, q.elem_bytes, q.kind = self.layout[f"src{p}"][2][1], rows, eb, kind
            if kind != LAST:
                assert part is None or rows == 1, "a shard's accumulator block is [rows][its own num_envs]"
                q.acc = at(f"acc{p}") + first * 8
        return d


# single-row sums: a shard's accumulators are then a slice of the batch's
SPEC_SHARD = ((LAST, np.uint8, 2), (LAST, np.float32, 3), (LAST, np.float64, 2), (SUM_F32, np.float32, 1),
              (SUM_F64, np.float64, 1), (SUM_I32, np.int32, 1))


def differences(p: Problem, got: np.ndarray, want: np.ndarray) -> List[str]:
    """Where two arenas differ: block names, or "guard" for a byte between blocks."""
    if got.tobytes() == want.tobytes():
        return []
    bad = np.flatnonzero(got != want)
    out = []
    for name, (off, dt, shape) in p.layout.items():
        size = int(np.prod(shape)) * dt.itemsize
        hit = bad[(bad >= off) & (bad < off + size)]
        if hit.size:
            out.append(f"{name}: {hit.size} bytes from element {int(hit[0] - off) // dt.itemsize}")
            bad = bad[(bad < off) | (bad >= off + size)]
    if bad.size:
        out.append(f"guard: {bad.size} bytes from {int(bad[0])}")
    return out


# ------------------------------------------------------------------------------------------------ a shard in a large workspace
SHARD_N = 300                                      # two tiles, the second short
WORKSPACES = (64, 65, 256, 257, 1000, 4096)        # tiles: either side of COMMIT's pass of 64 and of SCATTER's of 256, and the cap
WHERE, DRAWS, CAPS = ("first", "middle", "last"), ("sparse", "full"), ("seven", "total")


def shard_case(ntt: int, where: str, draw: str, cap: str):
    """The inputs of one case of a shard of `SHARD_N` environments inside a workspace of ``ntt`` tiles, from a seed of its own:
    the tile offset; ``tile_counts`` as the other shards left them (0..2 each, or 128..256 with half of them full, which
    brings a call's total to about 0.9 * 256 * ntt); the flags of two calls ("all", then "few", masked); the capacity (7,
    or the larger call's total plus 5); per call (records of the shard that the rule ``k >= n - capacity`` stores, records of
    the shard that finish); and the calls' totals."""
    rng = np.random.default_rng([ntt, WHERE.index(where), DRAWS.index(draw), CAPS.index(cap)])
    offset = {"first": 0, "middle": ntt // 2 - 1, "last": ntt - 2}[where]
    others = (rng.integers(0, 3, ntt) if draw == "sparse" else np.minimum(256, rng.integers(128, 512, ntt))).astype(np.int32)
    calls = []
    for how in ("all", "few"):
        mask = (rng.random(SHARD_N) < 0.8).astype(np.uint8)
        calls.append(flags_from(rng, finishing(rng, SHARD_N, how), mask) + (mask,))
    own = [(mask != 0) & ((term | trunc) != 0) for term, trunc, mask in calls]
    rest = int(others.sum()) - int(others[offset: offset + 2].sum())
    totals = [rest + int(o.sum()) for o in own]
    capacity = 7 if cap == "seven" else max(totals) + 5
    below = int(others[:offset].sum())
    stored = [(int((o & (below + np.cumsum(o) - o >= n - capacity)).sum()), int(o.sum())) for o, n in zip(own, totals)]
    return offset, others, calls, capacity, stored, totals


# ------------------------------------------------------------------------------------------------ whole stacks
def full_stack(device: str, capacity: int, n: int = 70, max_episode_steps: int = 5000, seed: int = 5):
    """An adapter with every optional block -- per-environment parameters, four materials, dynamic geometry, pulse and
    signal statistics (`tests._resume_common.episode_env`), an `EpisodeSampler`, a `Normalizer` -- and an `EpisodeLog` with
    ``params=True``, reset and put into the scenario of `tests._snapshot_common.scenario`: every tenth environment is at
    its target, every tenth breaks its wire, ``max_episode_steps`` truncates the others.  Returns (vec, log, action)."""
    from sparc_amd import EpisodeLog, EpisodeSampler, Normalizer, WireEDMVectorEnv
    from tests import _snapshot_common as snap
    from tests._resume_common import episode_env
    from tests.test_episode_sampler_host import HEIGHT, RANGES

    env = episode_env(device, n)
    sampler = EpisodeSampler(0x5EED_0000 + seed, params=RANGES, materials=True, height=HEIGHT, diameters=True)
    log = EpisodeLog(capacity=capacity, params=True)
    vec = WireEDMVectorEnv(env, episode_sampler=sampler, normalizer=Normalizer(gamma=0.9), max_episode_steps=max_episode_steps,
                           reward="progress", episode_log=log)
    vec.reset(seed=seed)
    action = snap.scenario(env, seed=seed + 70)
    return vec, log, action
