"""A shaped reward computed on the device: ten weighted terms of a control step in one call.

Progress alone teaches a policy to feed into short circuits and to cook the wire.  `wedm_reward` (include/wedm_hip.h, which
holds the definition) forms, per environment and in one launch, a weighted sum of the workpiece advance, a cost per step,
wire break and target flags, the interval's spark and short-circuit counts, its discharge energy, how far the gap fell below
a floor and how far the wire's peak temperature rose above a ceiling -- with a fixed order of operations, so that the MI355X
and the CPU oracle backends give the same bits -- and hands out the ten weighted terms beside their sum.

The terms read the ``*_ACC`` rows of the pulse and signal blocks, not the ``*_LAST`` rows that the observation shows: a launch
of one control interval begins with the control sample, which publishes and restarts the accumulators, so when the launch
ends ``*_LAST`` describes the interval before this action and ``*_ACC`` what this action caused.

`reward_definition` is the definition on host data in NumPy: the path of backends without the call (the CPU oracle backends
of the tests) and what the kernel is checked against, byte for byte.  `ShapedReward` holds the weights and the call's own
blocks; ``WireEDMVectorEnv(env, reward=ShapedReward(...))`` is the caller.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi

RW = _abi.RW
TERM_NAMES = ("progress", "step", "wire_break", "target_reached", "sparks", "shorts", "short_steps", "energy", "gap_below",
              "tmax_above")
assert len(TERM_NAMES) == _abi.RW_COUNT
_PULSE_TERMS = (RW.SPARKS, RW.SHORTS, RW.SHORT_STEPS)
_SIGNAL_TERMS = (RW.ENERGY, RW.GAP_BELOW, RW.TMAX_ABOVE)
_NAN64 = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
_NAN32 = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]


def reward_definition(f64: Optional[np.ndarray], i8: Optional[np.ndarray], pulse: Optional[np.ndarray],
                      sig: Optional[np.ndarray], pos_before: Optional[np.ndarray], restart: Optional[np.ndarray],
                      mask: Optional[np.ndarray], reward_out: np.ndarray, terms_out: Optional[np.ndarray], *,
                      weights: Sequence[float], pos_restart: float, gap_floor: float, tmax_ceiling: float, num_envs: int) -> None:
    """The definition of `wedm_reward` on host arrays, IN PLACE: ``f64`` / ``i8`` / ``pulse`` / ``sig`` are the state blocks
    ``[rows, stride >= num_envs]`` (None where no term with a nonzero weight reads them), ``pos_before`` float64
    ``[num_envs]``, ``restart`` / ``mask`` one byte per environment or None, ``reward_out`` float32 ``[num_envs]``,
    ``terms_out`` float64 ``[10, terms_stride >= num_envs]`` or None.  Written: columns ``[0, num_envs)`` of the two outputs,
    and nothing else."""
    N = int(num_envs)
    w = np.asarray(weights, dtype=np.float64)
    if N < 1 or w.shape != (_abi.RW_COUNT,):
        raise ValueError("reward: num_envs must be positive and there are ten weights")
    if not (np.isfinite(w).all() and np.isfinite([pos_restart, gap_floor, tmax_ceiling]).all()):
        raise ValueError("reward: a weight or threshold is not finite")
    on = w != 0.0
    for name, block, terms in (("f64", f64, (RW.PROGRESS,)), ("pos_before", pos_before, (RW.PROGRESS,)),
                               ("i8", i8, (RW.WIRE_BREAK, RW.TARGET)), ("pulse", pulse, _PULSE_TERMS), ("sig", sig, _SIGNAL_TERMS)):
        if block is None and any(on[int(k)] for k in terms):
            raise ValueError(f"reward: {name} is None though a term that reads it has a nonzero weight")
    live = np.ones(N, dtype=bool) if mask is None else np.asarray(mask).view(np.uint8).reshape(-1)[:N] != 0
    one, zero = np.ones(N), np.zeros(N)
    floor, ceiling = np.float64(gap_floor), np.float64(tmax_ceiling)

    def x(k: int) -> np.ndarray:   # (called for terms that are on only: a term that is off reads nothing)
        if k == RW.PROGRESS:
            p0 = pos_before[:N].astype(np.float64)
            if restart is not None:
                p0 = np.where(np.asarray(restart).view(np.uint8).reshape(-1)[:N] != 0, np.float64(pos_restart), p0)
            return f64[int(_abi.F64.WORKPIECE_POS), :N] - p0
        if k == RW.STEP:
            return one
        if k in (RW.WIRE_BREAK, RW.TARGET):
            row = _abi.I8.WIRE_BROKEN if k == RW.WIRE_BREAK else _abi.I8.TARGET_REACHED
            return np.where(i8[int(row), :N] != 0, 1.0, 0.0)
        if k in _PULSE_TERMS:
            row = {RW.SPARKS: _abi.PULSE.SPARK_ACC, RW.SHORTS: _abi.PULSE.SHORT_ACC, RW.SHORT_STEPS: _abi.PULSE.SHORT_STEPS_ACC}[k]
            return pulse[int(row), :N].astype(np.float64)
        if k == RW.ENERGY:
            return sig[int(_abi.SIG.ENERGY_ACC), :N]
        samples = sig[int(_abi.SIG.SAMPLES_ACC), :N]
        with np.errstate(invalid="ignore"):
            if k == RW.GAP_BELOW:
                gap_min = sig[int(_abi.SIG.GAP_MIN_ACC), :N]
                return np.where((samples > 0) & (floor > gap_min), floor - gap_min, 0.0)
            peak = sig[int(_abi.SIG.TMAX_PEAK_ACC), :N]
            return np.where((samples > 0) & (peak > ceiling), peak - ceiling, 0.0)

    r = np.zeros(N)
    with np.errstate(all="ignore"):
        for k in range(_abi.RW_COUNT):
            t = zero
            if on[k]:
                t = w[k] * x(RW(k))   # the product, rounded
                r = r + t             # then the addition
            if terms_out is not None:
                t = np.where(live, t, 0.0)
                terms_out[k, :N] = np.where(np.isnan(t), _NAN64, t)
        r = np.where(live, r, 0.0)
        r32 = r.astype(np.float32)    # the single rounding to float32
    reward_out[:N] = np.where(np.isnan(r), _NAN32, r32)


def device_reward(desc: "_abi.RewardDesc", device) -> None:
    """`wedm_reward` on ``device`` and torch's current stream, for callers that hold no environment."""
    import ctypes as C

    from . import _lib

    _lib.call_stateless(_lib.load().wedm_reward, torch.device(device), C.byref(desc))


def _np(t: Optional[torch.Tensor]) -> Optional[np.ndarray]:
    """A CPU tensor as the NumPy array over the same memory (bool as bytes)."""
    if t is None:
        return None
    return (t.view(torch.uint8) if t.dtype == torch.bool else t).numpy()


class ShapedReward:
    """A reward of weighted terms for `WireEDMVectorEnv`, computed by one `wedm_reward` call per control step.

    Every argument is the weight of one term (0.0: the term is off and nothing of it is read); the reward of a step is the
    sum, in this order, of

    ``progress``        micrometres the workpiece advanced in the step,
    ``step``            1 (a cost per step with a negative weight),
    ``wire_break``      1 where the wire is broken,
    ``target_reached``  1 where the target distance is reached,
    ``sparks`` / ``shorts`` / ``short_steps``   the step's spark pulses, short pulses and short-circuit samples
                        (needs ``pulse_stats=True``),
    ``energy``          the step's sum of voltage times current (needs ``signal_stats=True``),
    ``gap_below=(weight, floor_um)``     how far the step's smallest gap fell below ``floor_um`` (``signal_stats=True``),
    ``tmax_above=(weight, ceiling_K)``   how far the step's peak wire temperature rose above ``ceiling_K``
                        (``signal_stats=True``),

    each times its weight.  Penalties take negative weights.  The counts, sums and extrema are those of the launch itself
    (the accumulator rows), not the published rows the observation carries, which describe the interval before.

    ``term_names`` and ``weights`` name and hold the ten terms in order; ``WireEDMVectorEnv.step`` hands the weighted terms
    out as ``info["reward_terms"]`` (float64 ``[10, N]``, valid until the next step).  The object keeps nothing across
    steps: its weights and thresholds are settings of the adapter's checkpoint."""

    term_names = TERM_NAMES

    def __init__(self, progress: float = 1.0, step: float = 0.0, wire_break: float = 0.0, target_reached: float = 0.0,
                 sparks: float = 0.0, shorts: float = 0.0, short_steps: float = 0.0, energy: float = 0.0,
                 gap_below: Optional[Tuple[float, float]] = None, tmax_above: Optional[Tuple[float, float]] = None):
        gap_w, self.gap_floor = (0.0, 0.0) if gap_below is None else (float(gap_below[0]), float(gap_below[1]))
        tmax_w, self.tmax_ceiling = (0.0, 0.0) if tmax_above is None else (float(tmax_above[0]), float(tmax_above[1]))
        self.weights = tuple(float(v) for v in (progress, step, wire_break, target_reached, sparks, shorts, short_steps, energy,
                                                gap_w, tmax_w))
        if not all(np.isfinite(v) for v in (*self.weights, self.gap_floor, self.tmax_ceiling)):
            raise ValueError("a ShapedReward's weights and thresholds are finite")
        self.num_envs: Optional[int] = None

    def settings(self) -> Dict[str, Any]:
        """What changes the reward, as plain values: the adapter's checkpoint carries and compares them."""
        return {"weights": self.weights, "gap_floor": self.gap_floor, "tmax_ceiling": self.tmax_ceiling}

    # ------------------------------------------------------------------ binding
    def bind(self, vec) -> None:
        """Checks that ``vec``'s environment keeps what the terms read and allocates the call's own blocks, once."""
        if self.num_envs is not None:
            raise ValueError("this ShapedReward already serves an adapter")
        env = vec.env
        st, N = env.state, int(env.num_envs)
        on = [w != 0.0 for w in self.weights]
        names = lambda terms: ", ".join(TERM_NAMES[int(k)] for k in terms if on[int(k)])   # noqa: E731
        if st.pulse is None and names(_PULSE_TERMS):
            raise ValueError(f"the reward terms {names(_PULSE_TERMS)} need an environment built with pulse_stats=True")
        if st.signal is None and names(_SIGNAL_TERMS):
            raise ValueError(f"the reward terms {names(_SIGNAL_TERMS)} need an environment built with signal_stats=True")
        self.num_envs, self.device = N, torch.device(env.device)
        self._state = st
        self._pos_row = st.f64[int(_abi.F64.WORKPIECE_POS), :N]
        self._pos_restart = float(env.config.initial_gap)
        kw = dict(device=self.device)
        self.pos_before = torch.zeros(N, dtype=torch.float64, **kw)
        self.reward = torch.zeros(N, dtype=torch.float32, **kw)
        self.terms = torch.zeros((_abi.RW_COUNT, N), dtype=torch.float64, **kw)
        backend = getattr(env, "_backend", None)
        self._native = backend if hasattr(backend, "reward") else None
        pulse = st.pulse if names(_PULSE_TERMS) else None
        signal = st.signal if names(_SIGNAL_TERMS) else None
        self._blocks = (st.f64, st.i8, pulse, signal)
        d = self._desc = _abi.RewardDesc(
            f64=st.f64.data_ptr(), i8=st.i8.data_ptr(), pulse=None if pulse is None else pulse.data_ptr(),
            sig=None if signal is None else signal.data_ptr(), pos_before=self.pos_before.data_ptr(),
            reward_out=self.reward.data_ptr(), terms_out=self.terms.data_ptr(), stride=int(st.stride), terms_stride=N,
            pos_restart=self._pos_restart, gap_floor=self.gap_floor, tmax_ceiling=self.tmax_ceiling, num_envs=N)
        d.weight[:] = self.weights
        self._keep = None

    # ------------------------------------------------------------------ the two calls of a step
    def before_launch(self) -> None:
        """Keeps the workpiece positions as they lie before the step's launch: one copy, no allocation."""
        self.pos_before.copy_(self._pos_row)

    def after_launch(self, restart: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One `wedm_reward` call on the blocks as the launch left them.  ``restart``: the environments that the launch
        itself restarted (their progress counts from the position a reset leaves); ``mask``: the environments that took
        part (None: all); one byte per environment, contiguous, on the environment's device.  Returns the reward, float32
        ``[N]``, a block of this object's: valid until the next call, as ``terms`` is."""
        N = self.num_envs
        for t in (restart, mask):
            assert t is None or (t.is_contiguous() and t.numel() == N and t.element_size() == 1 and t.device == self.device)
        if self._native is None:
            f64, i8, pulse, signal = self._blocks
            reward_definition(_np(f64), _np(i8), _np(pulse), _np(signal), _np(self.pos_before), _np(restart), _np(mask),
                              _np(self.reward), _np(self.terms), weights=self.weights, pos_restart=self._pos_restart,
                              gap_floor=self.gap_floor, tmax_ceiling=self.tmax_ceiling, num_envs=N)
            return self.reward
        d = self._desc
        d.restart = None if restart is None else restart.data_ptr()
        d.mask = None if mask is None else mask.data_ptr()
        self._native.reward(d)
        self._keep = (restart, mask)  # the launch is asynchronous: its inputs live until the next call
        return self.reward
