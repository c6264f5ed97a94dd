"""A log of finished episodes kept on the device: an ordered ring and per-episode sums.

How episodes ended -- terminated or truncated, wire broken, target reached, how long they took, how far they cut, how many
sparks and short circuits they saw, which physics they had drawn -- appended by `wedm_episode_log` (include/wedm_hip.h, which
holds the definition) once per control step, in at most three launches without a host synchronisation and without
temporaries.  The records of a step lie in the order of the global environment index, so the log carries the same bytes
at every block size, on one device or several, and after a checkpoint.

`episode_log_definition` is that definition on host data in NumPy: the path of backends without the call (the CPU oracle
backends of the tests) and what the kernels are checked against, byte for byte.  `EpisodeLog` owns the ring, the
accumulators and the cursor; `WireEDMVectorEnv(env, episode_log=EpisodeLog())` is the caller.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi

LAST, SUM_F32, SUM_F64, SUM_I32 = _abi.ELOG_LAST, _abi.ELOG_SUM_F32, _abi.ELOG_SUM_F64, _abi.ELOG_SUM_I32
COUNT, SCATTER, COMMIT = _abi.ELOG_COUNT, _abi.ELOG_SCATTER, _abi.ELOG_COMMIT
TILE = _abi.NORM_TILE
_SUM_SRC = {SUM_F32: np.float32, SUM_F64: np.float64, SUM_I32: np.int32}
_SUM_ACC = {SUM_F32: np.float64, SUM_F64: np.float64, SUM_I32: np.int64}
_RAW = {1: np.uint8, 4: np.uint32, 8: np.uint64}


def _u8(a) -> Optional[np.ndarray]:
    if a is None:
        return None
    a = np.asarray(a)
    assert a.dtype.itemsize == 1
    return a.view(np.uint8).reshape(-1)


def episode_log_definition(planes: Sequence[Tuple[int, np.ndarray, np.ndarray, Optional[np.ndarray]]], terminated, truncated,
                           mask, env_out: np.ndarray, stamp_out: np.ndarray, head: np.ndarray, tile_counts: np.ndarray, *,
                           num_envs: int, env_id_offset: int = 0, stamp: int = 0, tile_offset: int = 0,
                           n_tiles_total: Optional[int] = None, flags: int = 0) -> None:
    """The definition of `wedm_episode_log` on host arrays, IN PLACE: ``planes`` is a sequence of ``(kind, src, dst, acc)``
    with ``src`` ``[rows, stride >= num_envs]``, ``dst`` ``[rows, capacity]`` (a sum: float64 or int64) and ``acc``
    ``[rows, num_envs]`` (a sum) or None; ``terminated`` / ``truncated`` (may be None) / ``mask`` (may be None) hold one byte
    per environment; ``env_out`` / ``stamp_out`` are int64 ``[capacity]``, ``head`` int64 ``[2]``, ``tile_counts`` int32
    ``[n_tiles_total]``.  Written: what the call writes, and nothing else."""
    N = int(num_envs)
    cap = int(env_out.shape[0])
    tiles = -(-N // TILE)
    ntt = tile_offset + tiles if n_tiles_total is None else int(n_tiles_total)
    if N < 1 or cap < 1 or not (tile_offset >= 0 and 1 <= ntt <= _abi.NORM_MAX_TILES and tile_offset + tiles <= ntt):
        raise ValueError("episode log: num_envs, capacity or the tile range is out of range")
    if flags & ~(COUNT | SCATTER | COMMIT):
        raise ValueError("episode log: undefined flag bits")
    if not 1 <= len(planes) <= _abi.ELOG_MAX_PLANES or sum(int(p[1].shape[0]) for p in planes) > _abi.ELOG_MAX_ROWS:
        raise ValueError(f"episode log: 1 to {_abi.ELOG_MAX_PLANES} planes of at most {_abi.ELOG_MAX_ROWS} rows in all")
    every = not flags & (COUNT | SCATTER | COMMIT)
    live = np.ones(N, dtype=bool) if mask is None else _u8(mask)[:N] != 0
    done = _u8(terminated)[:N] != 0
    if truncated is not None:
        done = done | (_u8(truncated)[:N] != 0)
    fin = live & done
    padded = np.zeros(tiles * TILE, dtype=bool)
    padded[:N] = fin
    if every or flags & COUNT:
        tile_counts[tile_offset: tile_offset + tiles] = padded.reshape(tiles, TILE).sum(axis=1)
    if every or flags & SCATTER:
        counts = tile_counts[:ntt].astype(np.int64)
        n = int(counts.sum())
        before = np.concatenate([[0], np.cumsum(counts)])[tile_offset: tile_offset + tiles]   # the tiles below each tile
        in_tile = np.cumsum(padded.reshape(tiles, TILE), axis=1) - padded.reshape(tiles, TILE)
        k = (before[:, None] + in_tile).reshape(-1)[:N]
        write = fin & (k >= n - cap)
        at = np.flatnonzero(write)
        slot = (int(head[0]) + k[at]) % cap
        for kind, src, dst, acc in planes:
            if kind == LAST:
                raw = _RAW[src.dtype.itemsize]
                dst.view(raw)[:, slot] = src.view(raw)[:, :N][:, at]
                continue
            assert src.dtype == _SUM_SRC[kind] and acc.dtype == dst.dtype == _SUM_ACC[kind] and acc.shape[1] == N
            total = acc + src[:, :N].astype(acc.dtype)   # one rounding per addition
            dst[:, slot] = total[:, at]
            acc[:, live] = np.where(fin, np.zeros((), dtype=acc.dtype), total)[:, live]
        env_out[slot] = int(env_id_offset) + at
        stamp_out[slot] = int(stamp)
    if every or flags & COMMIT:
        n = int(tile_counts[:ntt].astype(np.int64).sum())
        head[0] += n
        head[1] = n


def device_episode_log(desc: "_abi.ElogDesc", device) -> None:
    """`wedm_episode_log` on ``device`` and torch's current stream, for callers that hold no environment."""
    import ctypes as C

    from . import _lib

    _lib.call_stateless(_lib.load().wedm_episode_log, torch.device(device), C.byref(desc))


def _np(t: torch.Tensor) -> np.ndarray:
    """A CPU tensor as the NumPy array over the same memory (bool as bytes)."""
    return (t.view(torch.uint8) if t.dtype == torch.bool else t).numpy()


class _Plane:
    """One plane of the call: its column names (one per row), its kind, its source (None: handed in per step), the ring's
    rows and the accumulators."""

    def __init__(self, names, kind, src, dtype, step_key=None):
        self.names, self.kind, self.src, self.dtype, self.step_key = tuple(names), kind, src, dtype, step_key
        self.dst = self.acc = None


_ACC_OF = {SUM_F32: torch.float64, SUM_F64: torch.float64, SUM_I32: torch.int64}


class EpisodeLog:
    """The finished episodes of a `WireEDMVectorEnv`, kept on its device.

    ``capacity``: records the ring holds; a reader that falls further behind loses the oldest (`read` says how many).
    ``params=True``: with an environment built with ``env_params``, every record carries the physics rows its environment
    held (``envp_<row>``).

    Columns are fixed by name; an option adds its columns and moves no other.  Always: ``env`` (global id), ``stamp`` (the
    number of the adapter's ``step()`` call that ended the episode, from 1), ``terminated``, ``truncated``, ``wire_broken``,
    ``target_reached``, ``time_lo`` / ``time_hi`` (and ``time_us`` on read), ``episode``, ``spark_count``,
    ``workpiece_position``, ``wire_position``, ``tmax``, ``episode_count``, and the sums over the episode's control steps
    ``steps`` and ``reward_sum`` (the raw reward, before normalisation).  With a `Normalizer`: ``return``, ``length``.  With
    an `EpisodeSampler`: ``draw``, the environment's draw count -- ``sampler.expected(records["env"], records["draw"] - 1)``
    is the physics every logged episode ran with.  With ``wire_material=[...]``: ``material``.  With ``dynamic_geometry``:
    ``height``, ``diameter_index``.  With ``pulse_stats=True``: the sums ``sparks``, ``shorts``, ``short_steps``; with
    ``signal_stats=True``: ``samples``, ``current``, ``energy``.  With a `ShapedReward`: ``rw_progress`` ... ``rw_tmax_above``,
    the per-episode sum of each weighted reward term in float64 (they add up to ``reward_sum`` to within the float32 rounding
    of each step's reward).

    `read` is the one host synchronisation, taken when the user chooses; nothing else here reads the device."""

    def __init__(self, capacity: int = 65536, params: bool = False):
        if int(capacity) < 1:
            raise ValueError("an EpisodeLog holds at least one record")
        self.capacity, self.params = int(capacity), bool(params)
        self.columns: Optional[tuple] = None
        self.cursor = 0
        self.stamp = 0
        self._pending: Optional[Dict[str, Any]] = None

    # ------------------------------------------------------------------ binding
    def bind(self, vec) -> None:
        """Names the columns from what ``vec`` and its environment have and allocates everything the calls need, once."""
        if self.columns is not None:
            raise ValueError("this EpisodeLog already serves an adapter")
        env = vec.env
        st, N = env.state, int(env.num_envs)
        self.num_envs, self.device = N, torch.device(env.device)
        self._tiles = -(-N // TILE)
        if self._tiles > _abi.NORM_MAX_TILES:
            raise ValueError(f"an EpisodeLog serves at most {_abi.NORM_MAX_TILES * TILE} environments")
        I8, I32, F64 = _abi.I8, _abi.I32, _abi.F64
        row = lambda block, r, n=1: block[int(r): int(r) + n]   # noqa: E731
        one = lambda t: t.reshape(1, -1)                          # noqa: E731
        P: List[_Plane] = [
            _Plane(("terminated",), LAST, None, torch.uint8, "terminated"),
            _Plane(("truncated",), LAST, None, torch.uint8, "truncated"),
            _Plane(("wire_broken", "target_reached"), LAST, row(st.i8, I8.WIRE_BROKEN, 2), torch.int8),
            _Plane(("time_lo",), LAST, row(st.i32, I32.TIME), torch.int32),
            _Plane(("time_hi",), LAST, row(st.i32, I32.TIME_HI), torch.int32),
            _Plane(("episode",), LAST, row(st.i32, I32.EPISODE), torch.int32),
            _Plane(("spark_count",), LAST, row(st.i32, I32.SPARK_COUNT), torch.int32),
            _Plane(("workpiece_position", "wire_position"), LAST, row(st.f64, F64.WORKPIECE_POS, 2), torch.float64),
            _Plane(("tmax",), LAST, row(st.f64, F64.TMAX), torch.float64),
            _Plane(("episode_count",), LAST, one(vec.episode_count), torch.int64),
        ]
        assert int(I8.TARGET_REACHED) == int(I8.WIRE_BROKEN) + 1 and int(F64.WIRE_POS) == int(F64.WORKPIECE_POS) + 1
        norm, sampler = vec.normalizer, vec._episode_sampler
        if norm is not None:
            P.append(_Plane(("return",), LAST, one(norm.rows["last_return"]), torch.float64))
            P.append(_Plane(("length",), LAST, one(norm.rows["last_length"]), torch.int32))
        if sampler is not None:
            P.append(_Plane(("draw",), LAST, one(sampler._count), torch.int32))
        if getattr(env, "_wmat_rows", None) is not None:
            P.append(_Plane(("material",), LAST, one(env._wmat_index), torch.int64))
        dyn = getattr(env, "_dyn", None)
        if dyn is not None:
            P.append(_Plane(("height",), LAST, one(dyn.height), torch.float64))
            P.append(_Plane(("diameter_index",), LAST, one(dyn.dia), torch.int32))
        if self.params and getattr(env, "_envp_rows", None) is not None:
            P.append(_Plane(tuple(f"envp_{f.name.lower()}" for f in _abi.ENVP), LAST, env._envp_rows, torch.float64))
        self._ones = torch.ones((1, N), dtype=torch.int32, device=self.device)
        P.append(_Plane(("steps",), SUM_I32, self._ones, torch.int32))
        P.append(_Plane(("reward_sum",), SUM_F32, None, torch.float32, "reward"))
        if st.pulse is not None:
            P.append(_Plane(("sparks", "shorts", "short_steps"), SUM_I32, row(st.pulse, _abi.PULSE.SPARK_LAST, 3), torch.int32))
        if st.signal is not None:
            P.append(_Plane(("samples", "current", "energy"), SUM_F64, row(st.signal, _abi.SIG.SAMPLES_LAST, 3), torch.float64))
        shaped = getattr(vec, "_shaped", None)
        if shaped is not None:
            P.append(_Plane(tuple(f"rw_{name}" for name in shaped.term_names), SUM_F64, shaped.terms, torch.float64))
        assert len(P) <= _abi.ELOG_MAX_PLANES and sum(len(p.names) for p in P) <= _abi.ELOG_MAX_ROWS
        kw = dict(device=self.device)
        for p in P:
            if p.src is not None:
                assert p.src.dtype == p.dtype and p.src.dim() == 2 and p.src.stride(1) == 1 and p.src.shape[1] >= N, p.names
            p.dst = torch.zeros((len(p.names), self.capacity), dtype=p.dtype if p.kind == LAST else _ACC_OF[p.kind], **kw)
            if p.kind != LAST:
                p.acc = torch.zeros((len(p.names), N), dtype=_ACC_OF[p.kind], **kw)
        self._planes = P
        self.columns = ("env", "stamp") + tuple(n for p in P for n in p.names)
        self.env_id_offset = int(getattr(env, "env_id_offset", 0))
        self._initial_gap = float(env.config.initial_gap)
        self._materials = tuple(m.name for m in getattr(env, "wire_materials", ()) or ())
        self._env_out = torch.zeros(self.capacity, dtype=torch.int64, **kw)
        self._stamp_out = torch.zeros(self.capacity, dtype=torch.int64, **kw)
        self._head = torch.zeros(2, dtype=torch.int64, **kw)
        self._tile_counts = torch.zeros(self._tiles, dtype=torch.int32, **kw)
        backend = getattr(env, "_backend", None)
        self._native = backend if hasattr(backend, "episode_log") else None
        d = self._desc = _abi.ElogDesc(
            env_out=self._env_out.data_ptr(), stamp_out=self._stamp_out.data_ptr(), head=self._head.data_ptr(),
            tile_counts=self._tile_counts.data_ptr(), capacity=self.capacity, env_id_offset=self.env_id_offset,
            n_planes=len(P), num_envs=N, tile_offset=0, n_tiles_total=self._tiles, flags=0)
        for i, p in enumerate(P):
            q = d.plane[i]
            q.dst, q.acc = p.dst.data_ptr(), None if p.acc is None else p.acc.data_ptr()
            q.n_rows, q.elem_bytes, q.kind = len(p.names), p.dst.element_size() if p.kind == LAST else (8 if p.kind == SUM_F64 else 4), p.kind
            q.src = None if p.src is None else p.src.data_ptr()   # (None: the step's own tensor, named per call)
            q.src_stride = int(p.src.stride(0)) if len(p.names) > 1 else N
        self._keep = None
        if self._pending is not None:
            sd, self._pending = self._pending, None
            self.load_state_dict(sd)

    def _bound(self) -> None:
        if self.columns is None:
            raise ValueError("the EpisodeLog serves no adapter yet: pass it to WireEDMVectorEnv(env, episode_log=...)")

    # ------------------------------------------------------------------ the call
    def append(self, reward: torch.Tensor, terminated: torch.Tensor, truncated: torch.Tensor,
               mask: Optional[torch.Tensor] = None) -> None:
        """One call, after a control step: ``reward`` float32 (raw), the step's flags and ``mask`` (the environments that took
        part; None: all), one element per environment, contiguous, on the log's device."""
        self._bound()
        N = self.num_envs
        step = {"reward": reward, "terminated": terminated, "truncated": truncated}
        for key, t in step.items():
            assert t.is_contiguous() and t.numel() == N and t.device == self.device, key
        assert reward.dtype == torch.float32 and terminated.element_size() == 1 and truncated.element_size() == 1
        assert mask is None or (mask.is_contiguous() and mask.numel() == N and mask.element_size() == 1)
        self.stamp += 1
        if self._native is None:
            view = lambda t: _np(t).reshape(1, -1)   # noqa: E731
            planes = [(p.kind, _np(p.src) if p.src is not None else view(step[p.step_key]), _np(p.dst),
                       None if p.acc is None else _np(p.acc)) for p in self._planes]
            episode_log_definition(planes, _np(terminated), _np(truncated), None if mask is None else _np(mask),
                                   _np(self._env_out), _np(self._stamp_out), _np(self._head), _np(self._tile_counts),
                                   num_envs=N, env_id_offset=self.env_id_offset, stamp=self.stamp)
            return
        d = self._desc
        for i, p in enumerate(self._planes):
            if p.src is None:
                d.plane[i].src = step[p.step_key].data_ptr()
        d.terminated, d.truncated = terminated.data_ptr(), truncated.data_ptr()
        d.mask = None if mask is None else mask.data_ptr()
        d.stamp = self.stamp
        self._native.episode_log(d)
        self._keep = (reward, terminated, truncated, mask)  # the launches are asynchronous: their inputs live until the next call

    def reset_sums(self, mask: Optional[torch.Tensor] = None) -> None:
        """Zeroes the accumulators of the environments ``mask`` names (None: all).  An episode cut by a reset did not
        finish: nothing is logged."""
        self._bound()
        for p in self._planes:
            if p.acc is not None:
                if mask is None:
                    p.acc.zero_()
                else:
                    p.acc.masked_fill_(mask.reshape(1, -1), 0)

    def fork(self, src, dst) -> None:
        """Carries the accumulators from environments ``src`` to ``dst`` (`sparc_amd.snapshot.fork_rows`)."""
        from .snapshot import fork_rows

        self._bound()
        for p in self._planes:
            if p.acc is not None:
                for r in range(p.acc.shape[0]):
                    fork_rows(p.acc[r], src, dst)

    # ------------------------------------------------------------------ reading
    def tensors(self) -> Dict[str, torch.Tensor]:
        """The device blocks for consumers that stay on the device: every column's ``[capacity]`` row of the ring (a view)
        and ``head`` (int64 ``[2]``: records appended so far, records of the last step).  Record ``a`` lies at ``a %
        capacity``; valid until the next step."""
        self._bound()
        out = {"env": self._env_out, "stamp": self._stamp_out}
        for p in self._planes:
            for r, name in enumerate(p.names):
                out[name] = p.dst[r]
        out["head"] = self._head
        return out

    def _take(self, move: bool) -> Dict[str, Any]:
        self._bound()
        total = int(self._head[0].item())   # the host synchronisation
        first = max(self.cursor, total - self.capacity)
        lost = first - self.cursor
        idx = torch.arange(first, total, dtype=torch.int64, device=self.device) % self.capacity
        rec: Dict[str, Any] = {name: t.index_select(0, idx).cpu().numpy() for name, t in self.tensors().items() if name != "head"}
        rec["terminated"], rec["truncated"] = rec["terminated"].astype(bool), rec["truncated"].astype(bool)
        rec["wire_broken"], rec["target_reached"] = rec["wire_broken"].astype(bool), rec["target_reached"].astype(bool)
        rec["time_us"] = (rec["time_hi"].astype(np.int64) << 32) | (rec["time_lo"].astype(np.int64) & 0xFFFFFFFF)
        rec["lost"] = lost
        if move:
            self.cursor = total
        return rec

    def read(self) -> Dict[str, Any]:
        """The records appended since the last `read`, oldest first, as NumPy arrays by column name, with ``time_us``
        composed from its two words and ``lost``, the number of records the ring overwrote unread (an int).  Moves the
        cursor.  The one host synchronisation."""
        return self._take(True)

    def peek(self) -> Dict[str, Any]:
        """`read` without moving the cursor."""
        return self._take(False)

    def summary(self, records: Dict[str, Any]) -> Dict[str, Any]:
        """On the host, in NumPy: the number of ``episodes``; the shares ``terminated``, ``truncated``, ``wire_broken``,
        ``target_reached``; ``mean_time_us``; ``mean_progress`` (micrometres cut: ``workpiece_position`` minus the
        configuration's initial gap); ``mean_speed`` (progress per microsecond, over episodes that took time); with a `ShapedReward`
        ``mean_rw_<term>``, the mean of each reward term's per-episode sum; and, where
        there is a ``material`` column, the same ``per_material`` by material name."""
        self._bound()

        def of(sel) -> Dict[str, Any]:
            n = int(sel.sum())
            out: Dict[str, Any] = {"episodes": n}
            mean = lambda x: float(np.mean(x)) if np.size(x) else float("nan")   # noqa: E731
            for key in ("terminated", "truncated", "wire_broken", "target_reached"):
                out[key] = mean(records[key][sel].astype(np.float64))
            t = records["time_us"][sel].astype(np.float64)
            progress = records["workpiece_position"][sel] - self._initial_gap
            out["mean_time_us"], out["mean_progress"] = mean(t), mean(progress)
            out["mean_speed"] = mean(progress[t > 0] / t[t > 0])
            for key in records:
                if key.startswith("rw_"):
                    out[f"mean_{key}"] = mean(records[key][sel])
            return out

        everyone = np.ones(records["env"].shape[0], dtype=bool)
        out = of(everyone)
        if "material" in records:
            out["per_material"] = {name: of(records["material"] == m) for m, name in enumerate(self._materials)}
        return out

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self) -> Dict[str, Any]:
        """The column names, the ring, ``head``, the cursor, the accumulators and the stamp, as CPU tensors and plain values."""
        self._bound()
        host = lambda t: t.detach().cpu().clone()   # noqa: E731
        return {"columns": self.columns, "capacity": self.capacity, "num_envs": self.num_envs, "cursor": self.cursor,
                "stamp": self.stamp, "head": host(self._head), "env": host(self._env_out), "stamp_out": host(self._stamp_out),
                "ring": [host(p.dst) for p in self._planes],
                "sums": [host(p.acc) for p in self._planes if p.acc is not None]}

    def check_state_dict(self, sd: Dict[str, Any]) -> None:
        """Raises ``ValueError`` for a dict of another column set, capacity or batch size; writes nothing."""
        self._bound()
        if tuple(sd["columns"]) != self.columns:
            raise ValueError(f"the state dict logs the columns {tuple(sd['columns'])}, this EpisodeLog {self.columns}")
        if int(sd["capacity"]) != self.capacity:
            raise ValueError(f"the state dict's ring has capacity {sd['capacity']}, this EpisodeLog's {self.capacity}")
        if int(sd["num_envs"]) != self.num_envs:
            raise ValueError(f"the state dict holds {sd['num_envs']} environments, this EpisodeLog {self.num_envs}")

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        """Takes over a `state_dict`.  Before the log serves an adapter the dict is kept and checked when it does; a dict of
        another column set, capacity or batch size is refused before anything is written."""
        if self.columns is None:
            self._pending = sd
            return
        self.check_state_dict(sd)
        sums = [p for p in self._planes if p.acc is not None]
        for p, t in zip(self._planes, sd["ring"]):
            p.dst.copy_(t)
        for p, t in zip(sums, sd["sums"]):
            p.acc.copy_(t)
        self._head.copy_(sd["head"])
        self._env_out.copy_(sd["env"])
        self._stamp_out.copy_(sd["stamp_out"])
        self.cursor, self.stamp = int(sd["cursor"]), int(sd["stamp"])
