"""A sensor model on the device: what a machine measures of the observation, in one call.

The environment's observation is the simulator's own truth: the exact gap, debris density, flow rate and wire temperature,
which no wire-EDM machine reports.  A machine has the feed, voltage, current and pulse classification, through an ADC with
noise, a calibration error and a delay.  `wedm_sensor` (include/wedm_hip.h, which holds the definition with every rounding)
forms, per environment and in one launch, up to 159 measured channels: each a source column of the observation, delayed by a
whole number of control steps, scaled and shifted by a gain and offset error that is drawn once per episode, disturbed by
fresh Gaussian noise, quantised and saturated.  Calibration and delay are a pure function of (seed, global environment id,
episode number, channel), the noise of (seed, global id, call number, channel): Philox4x32-10 of the step kernels on streams
of its own, float64 with nothing fused -- so the measured columns carry the same bits on the MI355X and on the CPU oracle
backends, over 1 or 8 devices, and after a checkpoint.

`sensor_reference` is that definition on host data in NumPy: the path of a CPU device and of backends without the call, and
what the kernel is checked against, byte for byte.  `Channel` describes one output column, `Sensor` holds the table, the
delay ring and the output; ``WireEDMVectorEnv(env, sensor=Sensor(...))`` is the caller.
"""
from __future__ import annotations

import hashlib
import math
from typing import Any, Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _abi
from .policy_head import polar_normal
from .randomize import philox4x32_10

SN = _abi.SN
MAX_DELAY = _abi.SENSOR_MAX_DELAY
STREAM0 = _abi.SENSOR_STREAM0
CALIBRATION_STREAM0 = STREAM0 + 0x100000
#: What a machine's generator and drive report, out of an environment's raw observation columns: the feed, the gap voltage and
#: current, the discharge state, the pulse classification's three counts and the interval's current and energy sums.  Names
#: only -- there are no noise figures here, because nobody has measured a machine's: `Channel`'s defaults are a clean copy.
MEASURABLE_OBS_NAMES = ("wire_velocity", "voltage", "current", "spark_state", "spark_pulses", "short_pulses", "short_steps",
                        "current_sum", "energy_sum")
_NAN32 = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]
_M32 = np.uint64(0xFFFFFFFF)
_2_M32 = 2.3283064365386963e-10  # 2^-32


def _bytes(a: Optional[np.ndarray], n: int) -> Optional[np.ndarray]:
    return None if a is None else np.asarray(a).view(np.uint8).reshape(-1)[:n] != 0


def sensor_reference(planes: Sequence[np.ndarray], chan: np.ndarray, route: np.ndarray, first: Optional[np.ndarray],
                     mask: Optional[np.ndarray], episode: Optional[np.ndarray], out: np.ndarray, ring: Optional[np.ndarray],
                     pos: np.ndarray, age: np.ndarray, *, seed: int, t: int, env_id_offset: int, num_envs: int,
                     ring_len: int, trace: Optional[Dict[str, np.ndarray]] = None) -> None:
    """The definition of `wedm_sensor` on host arrays, IN PLACE.  ``planes``: one or two float32 ``[rows, stride >=
    num_envs]`` source blocks; ``chan`` float64 ``[6, C_out]``, ``route`` int32 ``[2, C_out]``; ``first`` / ``mask`` one byte
    per environment or None, ``episode`` int64 ``[num_envs]`` or None; ``out`` float32 ``[C_out, out_stride]``; ``ring``
    float32 ``[ring_len, C_in, ring_stride]`` (None with ``ring_len == 1``); ``pos`` / ``age`` int32 ``[num_envs]``.  Written:
    columns ``[0, num_envs)`` of ``out``, ``pos``, ``age`` and of the ring slot ``pos``, for the environments of ``mask``, and
    nothing else.  ``trace``: a dict that receives ``delay`` and ``d_eff`` (int64 ``[C_out, num_envs]``), ``gain`` and ``offset``
    (float64, 1 and 0 where a channel has no calibration) and ``noise`` (float64, the standard normal drawn, 0 where none)."""
    N, L = int(num_envs), int(ring_len)
    blocks = [np.asarray(p) for p in planes if p is not None and p.shape[0] > 0]
    if N < 1 or not blocks or any(b.dtype != np.float32 or b.ndim != 2 or b.shape[1] < N for b in blocks):
        raise ValueError("sensor: num_envs must be positive and the planes float32 [rows, stride >= num_envs]")
    src = np.concatenate([b[:, :N] for b in blocks], axis=0)  # [C_in, N], a copy
    C_in, C_out = src.shape[0], int(chan.shape[1])
    top = _abi.NORM_MAX_COLUMNS - 1
    if not (1 <= C_in <= top and 1 <= C_out <= top):
        raise ValueError(f"sensor: {C_in} source columns and {C_out} channels, each must lie in [1, {top}]")
    if not 1 <= L <= MAX_DELAY + 1:
        raise ValueError(f"sensor: ring_len {L} outside [1, {MAX_DELAY + 1}]")
    if L > 1 and ring is None:
        raise ValueError("sensor: ring is None though ring_len > 1")
    if tuple(chan.shape) != (_abi.SENSOR_FIELDS, C_out) or tuple(route.shape) != (_abi.SENSOR_ROUTES, C_out):
        raise ValueError("sensor: chan is [6, C_out] and route [2, C_out]")
    chan, route = np.asarray(chan, dtype=np.float64), np.asarray(route, dtype=np.int32)
    live = np.ones(N, dtype=bool) if mask is None else _bytes(mask, N)
    start = np.ones(N, dtype=bool) if first is None else _bytes(first, N)
    seed = int(seed) & (2 ** 64 - 1)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    t0, t1 = int(t) & 0xFFFFFFFF, (int(t) >> 32) & 0xFFFFFFFF
    gid = (np.uint64(int(env_id_offset) & 0xFFFFFFFF) + np.arange(N, dtype=np.uint64)) & _M32
    k = np.zeros(N, dtype=np.uint64) if episode is None else np.ascontiguousarray(np.asarray(episode)[:N], dtype=np.int64).view(np.uint64)
    k0, k1 = k & _M32, k >> np.uint64(32)
    env = np.arange(N)

    # 1. the episode's clock
    p_old = np.clip(pos[:N].astype(np.int64), 0, L - 1)
    a_old = np.clip(age[:N].astype(np.int64), 0, L - 1)
    new_pos = np.where(start, 0, (p_old + 1) % L)
    new_age = np.where(start, 0, np.minimum(a_old + 1, L - 1))
    pos[:N] = np.where(live, new_pos, pos[:N]).astype(np.int32)
    age[:N] = np.where(live, new_age, age[:N]).astype(np.int32)
    # 2. the newest sample into the ring
    if L > 1:
        at = env[live]
        ring[new_pos[at], :, at] = src[:, at].T
    # 3. the channels
    for c in range(C_out):
        sigma, gs, os_, lsb, lo, hi = (np.float64(v) for v in chan[:, c])
        s = min(max(int(route[_abi.SN_SOURCE, c]), 0), C_in - 1)
        md = min(max(int(route[_abi.SN_MAX_DELAY, c]), 0), L - 1)
        calibrated = bool(gs != 0.0) or bool(os_ != 0.0)
        delay = np.zeros(N, dtype=np.int64)
        ua = ub = np.zeros(N)
        if calibrated or md != 0:
            W = philox4x32_10((k0, k1, gid, (CALIBRATION_STREAM0 + c) & 0xFFFFFFFF), key)
            ua = (W[0].astype(np.float64) + 0.5) * _2_M32
            ub = (W[1].astype(np.float64) + 0.5) * _2_M32
            delay = ((W[2].astype(np.uint64) * np.uint64(md + 1)) >> np.uint64(32)).astype(np.int64)
        d_eff = np.minimum(delay, new_age)
        x = src[s]
        if L > 1:
            x = np.where(d_eff == 0, x, ring[(new_pos + L - d_eff) % L, s, env])
        with np.errstate(all="ignore"):
            y = x.astype(np.float64)
            gain, off, n = np.ones(N), np.zeros(N), np.zeros(N)
            if calibrated:
                gain = 1.0 + gs * (2.0 * ua - 1.0)
                off = os_ * (2.0 * ub - 1.0)
                y = (y * gain) + off
            if sigma != 0.0:
                n = polar_normal(key, t0, t1, gid, (STREAM0 + 64 * c) & 0xFFFFFFFF)
                y = y + sigma * n
            if lsb > 0.0:
                y = lsb * np.rint(y / lsb)
            y = np.where(y < lo, lo, y)
            y = np.where(y > hi, hi, y)
            o = np.where(y != y, _NAN32, y.astype(np.float32))
        out[c, :N] = np.where(live, o, out[c, :N])
        if trace is not None:
            for name, v in (("delay", delay), ("d_eff", d_eff), ("gain", gain), ("offset", off), ("noise", n)):
                trace.setdefault(name, np.zeros((C_out, N), dtype=v.dtype))[c] = v


def device_sensor(desc: "_abi.SensorDesc", device) -> None:
    """`wedm_sensor` on ``device`` and torch's current stream, for callers that hold no environment."""
    import ctypes as C

    from . import _lib

    _lib.call_stateless(_lib.load().wedm_sensor, torch.device(device), C.byref(desc))


def _np(t: Optional[torch.Tensor]) -> Optional[np.ndarray]:
    """A CPU tensor as the NumPy array over the same memory (bool as bytes)."""
    if t is None:
        return None
    return (t.view(torch.uint8) if t.dtype == torch.bool else t).numpy()


class Channel:
    """One measured column: ``Channel(source, name=None, sigma=0.0, gain_spread=0.0, offset_spread=0.0, lsb=0.0, lo=-inf,
    hi=inf, max_delay=0)``.

    ``source``: a name out of the adapter's raw ``obs_names`` (wire-profile columns included).  ``name``: the output column's
    (default: the source's).  ``sigma``: standard deviation of the noise added at every call.  ``gain_spread`` /
    ``offset_spread``: the episode's gain is uniform in ``1 +- gain_spread``, its offset uniform in ``+- offset_spread``.
    ``lsb``: the quantisation step (0: none).  ``lo`` / ``hi``: where the reading saturates.  ``max_delay``: the episode's
    delay is uniform over ``0 .. max_delay`` control steps (at most 7).  The defaults are a clean copy of the source."""

    __slots__ = ("source", "name", "sigma", "gain_spread", "offset_spread", "lsb", "lo", "hi", "max_delay")

    def __init__(self, source: str, name: Optional[str] = None, sigma: float = 0.0, gain_spread: float = 0.0,
                 offset_spread: float = 0.0, lsb: float = 0.0, lo: float = -math.inf, hi: float = math.inf, max_delay: int = 0):
        self.source, self.name = str(source), str(source if name is None else name)
        self.sigma, self.gain_spread, self.offset_spread, self.lsb = float(sigma), float(gain_spread), float(offset_spread), float(lsb)
        self.lo, self.hi = float(lo), float(hi)
        if isinstance(max_delay, bool) or int(max_delay) != max_delay:
            raise ValueError(f"channel {self.name!r}: max_delay must be a whole number of control steps, got {max_delay!r}")
        self.max_delay = int(max_delay)
        for what in ("sigma", "gain_spread", "offset_spread", "lsb"):
            v = getattr(self, what)
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError(f"channel {self.name!r}: {what} must be finite and not negative, got {v}")
        if not self.lo <= self.hi:
            raise ValueError(f"channel {self.name!r}: lo <= hi must hold, got ({self.lo}, {self.hi})")
        if not 0 <= self.max_delay <= MAX_DELAY:
            raise ValueError(f"channel {self.name!r}: max_delay must lie in [0, {MAX_DELAY}], got {self.max_delay}")

    def settings(self) -> Tuple:
        return (self.source, self.name, self.sigma, self.gain_spread, self.offset_spread, self.lsb, self.lo, self.hi, self.max_delay)


class Sensor:
    """``Sensor(channels, privileged=(), seed=0)``: the measurement side of a `WireEDMVectorEnv`.

    The output columns are ``channels`` in order -- the actor's view, ``actor_dim`` of them -- and behind them clean copies
    of the raw columns named in ``privileged`` (``"all"``: every raw column), named ``priv.<name>``: what a critic may see
    beside the measurements in the usual asymmetric setup (``PolicyNet(sensor.actor_dim, head)`` for the actor reads the
    leading columns of the same observation in place, ``PolicyNet(vec, head)`` for the critic all of them).
    `MEASURABLE_OBS_NAMES` lists what a machine can report; the noise figures are the user's to give.

    ``WireEDMVectorEnv(env, sensor=s)`` binds the sensor and calls `apply` once per `reset` and `step`; ``t``, the call number,
    and the per-environment delay ring travel in `state_dict`."""

    def __init__(self, channels: Sequence[Channel], privileged: Union[str, Sequence[str]] = (), seed: int = 0):
        self.channels = tuple(channels)
        if not self.channels or not all(isinstance(c, Channel) for c in self.channels):
            raise ValueError("a Sensor takes a non-empty sequence of Channel objects")
        if isinstance(privileged, str) and privileged != "all":
            raise ValueError('privileged is a sequence of raw column names or "all"')
        self.privileged = privileged if privileged == "all" else tuple(str(p) for p in privileged)
        self.seed, self.t = int(seed) & (2 ** 64 - 1), 0
        self.actor_dim = len(self.channels)
        self.num_envs: Optional[int] = None
        self.obs_names: Optional[Tuple[str, ...]] = None

    # ------------------------------------------------------------------ binding
    def _table(self, raw: Sequence[str]):
        """(output names, every output column as a `Channel`) against the raw column names ``raw``."""
        raw = tuple(raw)
        priv = raw if self.privileged == "all" else self.privileged
        cols = self.channels + tuple(Channel(p, name=f"priv.{p}") for p in priv)
        for c in cols:
            if c.source not in raw:
                raise ValueError(f"channel {c.name!r}: unknown source {c.source!r}; the adapter's raw columns are {list(raw)}")
        names = tuple(c.name for c in cols)
        twice = sorted({n for n in names if names.count(n) > 1})
        if twice:
            raise ValueError(f"the output names {twice} occur more than once: give the channels distinct names")
        if len(cols) > _abi.NORM_MAX_COLUMNS - 1:
            raise ValueError(f"a Sensor puts out at most {_abi.NORM_MAX_COLUMNS - 1} columns, got {len(cols)}")
        return names, cols

    def bind(self, vec) -> None:
        """Checks every channel against ``vec``'s raw columns, uploads the table and allocates ``out``, ``ring``, ``pos`` and
        ``age``, once."""
        if self.num_envs is not None:
            raise ValueError("this Sensor already serves an adapter")
        env = vec.env
        raw = tuple(vec.obs_names)
        names, cols = self._table(raw)
        N, C_in, C_out = int(env.num_envs), len(raw), len(cols)
        self.raw_names, self.obs_names = raw, names
        self.num_envs, self.device = N, torch.device(env.device)
        self.env_id_offset = int(getattr(env, "env_id_offset", 0)) & 0xFFFFFFFF
        self.ring_len = L = 1 + max(c.max_delay for c in cols)
        chan = np.array([[c.sigma, c.gain_spread, c.offset_spread, c.lsb, c.lo, c.hi] for c in cols], dtype=np.float64).T
        route = np.array([[raw.index(c.source), c.max_delay] for c in cols], dtype=np.int32).T
        self._fingerprint = hashlib.sha256(repr((raw, tuple(c.settings() for c in cols))).encode()).hexdigest()[:16]
        kw = dict(device=self.device)
        self._chan = torch.from_numpy(np.ascontiguousarray(chan)).to(self.device)
        self._route = torch.from_numpy(np.ascontiguousarray(route)).to(self.device)
        self.out = torch.zeros((C_out, N), dtype=torch.float32, **kw)
        self.ring = torch.zeros((L, C_in, N), dtype=torch.float32, **kw) if L > 1 else None
        self.pos = torch.zeros(N, dtype=torch.int32, **kw)
        self.age = torch.zeros(N, dtype=torch.int32, **kw)
        backend = getattr(env, "_backend", None)
        self._native = backend if hasattr(backend, "sensor") else None
        self._desc = _abi.SensorDesc(
            chan=self._chan.data_ptr(), route=self._route.data_ptr(), out=self.out.data_ptr(),
            ring=None if self.ring is None else self.ring.data_ptr(), pos=self.pos.data_ptr(), age=self.age.data_ptr(),
            out_stride=N, ring_stride=N, seed=self.seed, env_id_offset=self.env_id_offset, num_envs=N, n_out=C_out, ring_len=L)
        self._keep = None

    def _bound(self) -> None:
        if self.num_envs is None:
            raise ValueError("the Sensor serves no adapter yet: pass it to WireEDMVectorEnv(env, sensor=...)")

    # ------------------------------------------------------------------ the call
    def apply(self, planes: Sequence[torch.Tensor], first: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
              episode: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One `wedm_sensor` call on the source ``planes`` (float32 ``[rows, stride]``, as `wedm_normalize` takes them), then
        ``t += 1``.  ``first``: the environments whose sample is the first of an episode (None: all); ``mask``: those that
        take part (None: all); one byte per environment, contiguous; ``episode``: int64 ``[N]`` episode numbers (None: 0).
        Returns the ``[C_out, N]`` plane, the sensor's own: valid until the next call.  No host synchronisation and no
        allocation."""
        self._bound()
        N = self.num_envs
        planes = [p for p in planes if p is not None]
        if sum(int(p.shape[0]) for p in planes) != len(self.raw_names):
            raise ValueError(f"sensor: the planes hold {sum(int(p.shape[0]) for p in planes)} rows, the Sensor reads {len(self.raw_names)}")
        for b in (first, mask):
            assert b is None or (b.is_contiguous() and b.numel() == N and b.element_size() == 1 and b.device == self.device)
        assert episode is None or (episode.dtype == torch.int64 and episode.is_contiguous() and episode.numel() == N)
        if self._native is None:
            sensor_reference([_np(p) for p in planes], _np(self._chan), _np(self._route), _np(first), _np(mask), _np(episode),
                             _np(self.out), _np(self.ring), _np(self.pos), _np(self.age), seed=self.seed, t=self.t,
                             env_id_offset=self.env_id_offset, num_envs=N, ring_len=self.ring_len)
        else:
            d = self._desc
            for k in range(2):
                p = planes[k] if k < len(planes) else None
                assert p is None or (p.dtype == torch.float32 and p.dim() == 2 and p.stride(1) == 1 and p.device == self.device)
                d.plane[k].rows = None if p is None else p.data_ptr()
                d.plane[k].n_rows = 0 if p is None else int(p.shape[0])
                d.plane[k].stride = 0 if p is None else int(p.stride(0))
            d.first = None if first is None else first.data_ptr()
            d.mask = None if mask is None else mask.data_ptr()
            d.episode = None if episode is None else episode.data_ptr()
            d.seed, d.t = self.seed, self.t
            self._native.sensor(d)
            self._keep = (planes, first, mask, episode)  # the launch is asynchronous: its inputs live until the next call
        self.t = (self.t + 1) & (2 ** 64 - 1)
        return self.out

    # ------------------------------------------------------------------ seed, fork, checkpoints
    def reseed(self, seed: int) -> None:
        """A new seed, and the call number back at 0."""
        self.seed, self.t = int(seed) & (2 ** 64 - 1), 0

    def fork(self, src, dst) -> None:
        """Carries the per-environment columns -- the output, the delay ring, ``pos`` and ``age`` -- from environments ``src``
        to ``dst`` (`sparc_amd.snapshot.fork_rows`).  A destination keeps its own calibration and noise: they are a function
        of its own global id and episode number, as its Philox stream in the physics is."""
        from .snapshot import fork_rows

        self._bound()
        rows = [self.pos, self.age, *self.out]
        if self.ring is not None:
            rows += list(self.ring.view(-1, self.num_envs))
        for row in rows:
            fork_rows(row, src, dst)

    def fingerprint(self) -> str:
        """What names the channel set: the raw columns and every output column's settings."""
        self._bound()
        return self._fingerprint

    def settings(self) -> Dict[str, Any]:
        self._bound()
        return {"fingerprint": self._fingerprint, "obs_names": tuple(self.obs_names), "actor_dim": self.actor_dim}

    def state_dict(self) -> Dict[str, Any]:
        """Seed, call number, the fingerprint of the channel settings, and ``out``, ``ring``, ``pos``, ``age`` as CPU tensors."""
        self._bound()
        host = lambda x: None if x is None else x.detach().cpu().clone()   # noqa: E731
        return {"seed": self.seed, "t": self.t, "fingerprint": self._fingerprint, "num_envs": self.num_envs,
                "out": host(self.out), "ring": host(self.ring), "pos": host(self.pos), "age": host(self.age)}

    def check_state_dict(self, sd: Dict[str, Any]) -> None:
        """Raises ``ValueError`` for a dict of another channel set or batch size; writes nothing."""
        self._bound()
        if sd.get("fingerprint") != self._fingerprint:
            raise ValueError("the checkpoint's Sensor has other channels, settings or raw columns than this one (fingerprint "
                             f"{sd.get('fingerprint')!r} against {self._fingerprint!r})")
        if int(sd["num_envs"]) != self.num_envs:
            raise ValueError(f"the checkpoint's Sensor holds {sd['num_envs']} environments, this one {self.num_envs}")
        for name in ("out", "ring", "pos", "age"):
            mine, theirs = getattr(self, name), sd[name]
            if (mine is None) != (theirs is None) or (mine is not None and (tuple(theirs.shape) != tuple(mine.shape) or theirs.dtype != mine.dtype)):
                raise ValueError(f"the checkpoint's Sensor block {name!r} does not have this one's shape and type")

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        """Takes over a `state_dict`; a dict of another channel set or batch size is refused before a byte changes."""
        self.check_state_dict(sd)
        for name in ("out", "ring", "pos", "age"):
            if getattr(self, name) is not None:
                getattr(self, name).copy_(sd[name])
        self.seed, self.t = int(sd["seed"]) & (2 ** 64 - 1), int(sd["t"])
