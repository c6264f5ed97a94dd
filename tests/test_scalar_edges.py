"""The scalar physics' thresholds at their edge, on every kernel.

The device code is no transcription of the oracle at the scalar decisions: `scalar_prelude` is branch-free, and
`quiet_prelude_t` restates a list of threshold comparisons to decide, per wave, whether the microsecond is a quiet one.
A ``>=`` written as ``>``, or a comparison against a value of one step earlier or later, differs from the oracle only
when an environment sits exactly on the threshold -- where random inputs never land.  The ladders here put environments
there: -2, -1, 0, +1, +2 float64 ulps of a directly assignable row around each threshold.

Shape: 128 segments (every family takes the wire) and 230 environments -- three full blocks of 64 and a partly dead one.
64 consecutive environments share their waves at any lane count per environment, so the rungs are laid out to drive the
wave-uniform fast path both ways: block 0 sits on one side of the threshold, block 1 on the other (each on the rung next
to it), block 2 alternates the sides from environment to environment, block 3 holds the ladder in order.  Launches of 1, 1, 7 and
50 us; every byte of every block is compared with the oracle after every launch.

Every ladder must be observable: its test asserts on the ORACLE's result after the first microsecond that a named row
(the flag, the refreshed cache row, H_BASE, the generator's state ...) equals a plain float64 restatement of the one
reference line, rung by rung (CPU half, unmarked), and that this row differs between rungs on the two sides, the two
adjacent rungs straddling the threshold (the middle rung sits exactly on it wherever the expression allows).  A "guard"
ladder is one whose correct result is the same on every rung while a stated wrong variant (the clamp left out) is not.

Ladders that were dropped, because no observable difference can exist:
- ``ex > 24`` (the quiet path's and the general path's shortcut past the sigmoid) with Philox uniforms: no uniform is
  below 2^-33 and 1 / (1 + e^24) is, so the roll fails on either side;
- ``exponent < -500``: the sigmoid is already exactly 1.0 there (e^-500 is far below half an ulp of 1);
- ``k rho`` against 2.0: both sides of dielectric.py:124-127 evaluate exp(-(k rho)) once k rho >= 0.5 (fast_exp's own
  branch), and -(k rho) == (-k) rho exactly;
- ``max(-0.9, ve)`` apart from the 0.1 h floor: 1 + -0.9 is 0.09999999999999998 < 0.1 in float64, so whenever the clamp
  binds the floor binds too and replaces the clamped value: one ladder (on the unwinding velocity) covers both, a second
  one guards the floor where float32 can see it;
- ``gap <= random_short_min_gap``: within thousands of ulps above min_gap the ramp's factor 1 - (gap - min) / (max - min)
  rounds to 1.0, so both sides give max_probability exactly;
- ``max(0.0, d)`` of the short detection with the default positive hard_short_gap: d <= 0 and a d of a few ulps are both
  hard shorts; it is kept as a guard ladder under a slightly negative hard_short_gap, where leaving the clamp out shorts.
"""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from sparc_amd import (DielectricModuleParameters, EnvironmentConfig, IgnitionModuleParameters, MechanicsModuleParameters,
                       WireEDMEnv, WireModuleParameters, _abi)
from tests._compare import block_diffs
from tests._oracle_backend import OracleBackend, OracleBackendRows

N = 230
SEGMENT_LEN = 0.625
LAUNCHES = (1, 1, 7, 50)
RUNGS = np.arange(-2, 3)
SEED = 909
F, I, B = _abi.F64, _abi.I32, _abi.I8
X0 = 10.0                                     # wire position of every ladder that does not say otherwise
CAVITY_COEFF = math.pi * (0.2 / 2.0) * 20.0   # dielectric.py:62 at the default wire diameter and workpiece height


# ------------------------------------------------------------------ float64 ulps
def _ord(x):
    b = np.asarray(x, dtype=np.float64).view(np.int64)
    return np.where(b < 0, np.int64(-2**63) - b, b)


def ulps(x, k):
    """x moved by k float64 ulps (k an integer array; crosses zero through the denormals)."""
    k = np.asarray(k, dtype=np.int64)
    o = _ord(np.full(k.shape, x, dtype=np.float64)) + k
    return np.where(o < 0, np.int64(-2**63) - o, o).astype(np.int64).view(np.float64)


def flip_center(decide, guess, reach=1 << 14):
    """The float64 nearest `guess` at which the boolean `decide(value)` changes: decide(centre - 1 ulp) != decide(centre)."""
    j = np.arange(-reach, reach + 1)
    d = decide(ulps(guess, j))
    at = np.nonzero(d[1:] != d[:-1])[0]
    assert len(at) == 1, (guess, len(at))
    return float(ulps(guess, j[at[0] + 1 : at[0] + 2])[0])


def layout(decision):
    """Rung per environment from the decision on RUNGS.  Block 0: one side of the threshold, every environment on that
    side's rung next to it (the exact-equality rung where it belongs there); block 1: the same on the other side; block
    2: the two sides' rungs alternating from environment to environment; block 3: the ladder in order.  A wave never
    reaches across a block, so blocks 0 and 1 are waves in which every lane sits on the last rung before the threshold:
    a wave-uniform test written with the neighbouring comparison (`<=` for `<`) takes the whole wave the wrong way."""
    a, b = RUNGS[decision == decision[0]], RUNGS[decision != decision[0]]
    if len(b) == 0:   # a guard ladder: the same decision on every rung
        a, b = RUNGS[:1], RUNGS[-1:]
    near_a = a[np.argmin([np.abs(b - r).min() for r in a])]
    near_b = b[np.argmin([np.abs(a - r).min() for r in b])]
    i = np.arange(64)
    k = np.empty(N, dtype=np.int64)
    k[0:64] = near_a
    k[64:128] = near_b
    k[128:192] = np.where(i % 2 == 0, a[(i // 2) % len(a)], b[(i // 2) % len(b)])
    k[192:N] = RUNGS[np.arange(N - 192) % len(RUNGS)]
    return k


# ------------------------------------------------------------------ ladders
# A ladder is a function k -> dict(rows, decision, expect, row[, wrong][, kw][, servo][, replay]):
#   rows      {(block, row): value or array}: written over the common start state on both sides
#   decision  bool per environment: the reference line's comparison, restated in float64
#   expect    what `row` = (block, row) holds in the ORACLE after the first microsecond, from that restatement
#   wrong     (guard ladders) what it would hold with the clamp left out
#   kw        module parameter overrides {"ignition": {...}, ...}, "control_mode"
def hard_short(k):
    """ignition.py:127 `gap < hard_short_gap`: x = 10, wp = 12 +- k ulp; the subtraction is exact."""
    wp = ulps(12.0, k)
    short = np.maximum(0.0, wp - X0) < 2.0
    return dict(rows={("f64", F.WORKPIECE_POS): wp}, decision=short, expect=short.astype(np.int8), row=("i8", B.IS_SHORT))


HSG_NEG = -1.5 * (ulps(10.0, np.array([1]))[0] - 10.0)   # between the gaps of rungs -1 and -2 of the next ladder


def gap_clamp_zero(k):
    """ignition.py:201 `max(0.0, wp - x)` (guard): under a hard_short_gap between rungs -2 and -1 of d the clamped gap is
    never below it, the unclamped difference is on rung -2."""
    wp = ulps(10.0, k)
    d = wp - X0
    short = np.maximum(0.0, d) < HSG_NEG
    return dict(rows={("f64", F.WORKPIECE_POS): wp}, decision=short, expect=short.astype(np.int8), wrong=(d < HSG_NEG).astype(np.int8),
                guard=True, row=("i8", B.IS_SHORT), kw={"ignition": {"hard_short_gap": float(HSG_NEG)}})


def gap_clamp_milli(k):
    """dielectric.py:88 `max(0.001, wp - x)`: x = 0, wp = 0.001 +- k ulp; the cavity volume follows d only above 0.001."""
    wp = ulps(0.001, k)
    d = wp - 0.0
    gap_um = np.maximum(0.001, d)
    return dict(rows={("f64", F.WORKPIECE_POS): wp, ("f64", F.WIRE_POS): 0.0, ("f64", F.LAST_GAP): 0.001},
                decision=d > 0.001, expect=CAVITY_COEFF * (gap_um * 0.001), row=("f64", F.CAVITY))


def collision(k):
    """wire_edm.py:174 `wire_position > workpiece_position + 100`: wp = 50, x = 150 +- k ulp (the wire is at rest)."""
    x = ulps(150.0, k)
    broken = x > 50.0 + 100
    return dict(rows={("f64", F.WORKPIECE_POS): 50.0, ("f64", F.WIRE_POS): x, ("f64", F.LAST_GAP): 0.001},
                decision=broken, expect=broken.astype(np.int8), row=("i8", B.WIRE_BROKEN))


def target_reached(k):
    """wire_edm.py:177 `workpiece_position >= target_position`: wp = 1000 (no spark), target = 1000 +- k ulp."""
    target = ulps(1000.0, k)
    reached = 1000.0 >= target
    return dict(rows={("f64", F.WORKPIECE_POS): 1000.0, ("f64", F.TARGET_POS): target, ("f64", F.LAST_GAP): 990.0},
                decision=reached, expect=reached.astype(np.int8), row=("i8", B.TARGET_REACHED))


def cache_gap(k):
    """dielectric.py:114 `abs(gap_um - _last_gap_um) > 0.01`: gap 50, ladder on LAST_GAP; a refresh rewrites the row."""
    centre = flip_center(lambda L: np.abs(50.0 - L) > 0.01, 50.0 - 0.01)
    last = ulps(centre, k)
    refresh = np.abs(50.0 - last) > 0.01
    return dict(rows={("f64", F.LAST_GAP): last}, decision=refresh, expect=np.where(refresh, 50.0, last), row=("f64", F.LAST_GAP))


RHO_SMALL = 0.0005 / (CAVITY_COEFF * (50.0 * 0.001))   # debris below the removal gate: the density stays


def cache_density(k):
    """dielectric.py:115 `abs(density - _last_debris_density) > 0.001`: ladder on LAST_DENSITY under a constant density."""
    centre = flip_center(lambda L: np.abs(RHO_SMALL - L) > 0.001, RHO_SMALL - 0.001)
    last = ulps(centre, k)
    refresh = np.abs(RHO_SMALL - last) > 0.001
    return dict(rows={("f64", F.DEBRIS_VOLUME): 0.0005, ("f64", F.DEBRIS_DENSITY): RHO_SMALL, ("f64", F.LAST_DENSITY): last},
                decision=refresh, expect=np.where(refresh, RHO_SMALL, last), row=("f64", F.LAST_DENSITY))


def cache_flow(k):
    """wire.py:279 `abs(flow - _last_flow_condition) > 0.01`: flow 1.0, ladder on WIRE_LAST_FLOW."""
    centre = flip_center(lambda L: np.abs(1.0 - L) > 0.01, 1.0 - 0.01)
    last = ulps(centre, k)
    refresh = np.abs(1.0 - last) > 0.01
    return dict(rows={("f64", F.WIRE_LAST_FLOW): last}, decision=refresh, expect=np.where(refresh, 1.0, last),
                row=("f64", F.WIRE_LAST_FLOW))


RHO_2 = 0.002 / (CAVITY_COEFF * (50.0 * 0.001))


def removal_gate_flow(k):
    """dielectric.py:154 `flow_rate > 0.001`: ladder on FLOW (no cache refresh), 0.002 mm^3 of debris; removal shrinks it."""
    flow = ulps(0.001, k)
    gate = flow > 0.001
    return dict(rows={("f64", F.FLOW): flow, ("f64", F.WIRE_LAST_FLOW): 0.001, ("f64", F.DEBRIS_VOLUME): 0.002,
                      ("f64", F.DEBRIS_DENSITY): RHO_2, ("f64", F.LAST_DENSITY): RHO_2},
                decision=gate, expect=np.where(gate, 0.002 - (0.01 * 100.0 * 1e-6) * flow, 0.002), row=("f64", F.DEBRIS_VOLUME))


def removal_gate_debris(k):
    """dielectric.py:154 `debris_volume > 0.001`: ladder on DEBRIS_VOLUME under flow 1.0."""
    debris = ulps(0.001, k)
    gate = debris > 0.001
    rho = 0.001 / (CAVITY_COEFF * (50.0 * 0.001))
    return dict(rows={("f64", F.DEBRIS_VOLUME): debris, ("f64", F.DEBRIS_DENSITY): rho, ("f64", F.LAST_DENSITY): rho},
                decision=gate, expect=np.where(gate, debris - (0.01 * 100.0 * 1e-6) * 1.0, debris), row=("f64", F.DEBRIS_VOLUME))


FLUSH = {"dielectric": {"debris_removal_efficiency": 1.0, "base_flow_rate": 4000.0}}
RPU_FLUSH = 1.0 * 4000.0 * 1e-6   # dielectric.py:64-66


def removal_clamp(k):
    """dielectric.py:158 `max(0.0, debris_volume - removed)`: debris = removed +- k ulp under flow 1.0 (guard as well)."""
    debris = ulps(RPU_FLUSH * 1.0, k)
    nv = debris - RPU_FLUSH * 1.0
    rho = RPU_FLUSH / (CAVITY_COEFF * (50.0 * 0.001))
    return dict(rows={("f64", F.DEBRIS_VOLUME): debris, ("f64", F.DEBRIS_DENSITY): rho, ("f64", F.LAST_DENSITY): rho},
                decision=nv > 0.0, expect=np.maximum(0.0, nv), wrong=nv, row=("f64", F.DEBRIS_VOLUME), kw=FLUSH)


NO_DEBRIS_SHORT = {"ignition": {"base_critical_density": 2.0, "max_critical_density": 3.0}}   # a full gap does not short


def density_clamp(k):
    """dielectric.py:111 `min(1.0, debris_volume / cavity_volume)`: debris = cavity volume +- k ulp (guard as well)."""
    cavity = CAVITY_COEFF * (50.0 * 0.001)
    debris = ulps(cavity, k)
    q = debris / cavity
    return dict(rows={("f64", F.DEBRIS_VOLUME): debris, ("f64", F.DEBRIS_DENSITY): 1.0, ("f64", F.LAST_DENSITY): 1.0},
                decision=q < 1.0, expect=np.minimum(1.0, q), wrong=q, row=("f64", F.DEBRIS_DENSITY), kw=NO_DEBRIS_SHORT)


def fast_exp_half(k):
    """dielectric.py:36 `x < 0.5` of fast_exp at k = 1: the Pade form 0.6 against exp(-0.5) = 0.6065; the caches are stale,
    so the flow is recomputed.  Ladder on the debris volume around half the cavity volume."""
    cavity = CAVITY_COEFF * (50.0 * 0.001)
    centre = flip_center(lambda v: 1.0 * np.minimum(1.0, v / cavity) < 0.5, 0.5 * cavity)
    debris = ulps(centre, k)
    kd = 1.0 * np.minimum(1.0, debris / cavity)
    pade = kd < 0.5
    return dict(rows={("f64", F.DEBRIS_VOLUME): debris, ("f64", F.DEBRIS_DENSITY): 0.5, ("f64", F.LAST_DENSITY): 0.0},
                decision=pade, expect=pade, observe=lambda row: row < 0.603, row=("f64", F.FLOW), kw=NO_DEBRIS_SHORT)


def _f32_tie_base(lo_factor, hi_factor, near=14000.0):
    """A base convection coefficient near `near` at which float32 tells base * lo_factor from base * hi_factor apart."""
    mid = float(np.float32(near * 0.1)) + 2.0 ** -14      # the midpoint between float32(1400) and its successor
    for j in range(-4000, 4000):
        b = float(ulps(mid / hi_factor, np.array([j]))[0])
        if np.float32(b * lo_factor) != np.float32(b * hi_factor):
            return b
    raise AssertionError("no such base")


BASE_CLAMP = _f32_tie_base(0.1, 1.0 + -float(ulps(0.9, np.array([-1]))[0]))   # floor value against rung -1's base * (1 + ve)
BASE_FLOOR = 14000.000610351564                                              # base * (1 + -0.9) against the floor (fixture F19)


def _convection(k, base):
    unwind = ulps(0.9, k)
    ve = -1.0 * unwind
    clamped = ~(ve > -0.9)
    ve = np.where(ve > -0.9, ve, -0.9)
    hb = base * (1.0 + ve)
    return unwind, clamped, hb, np.maximum(hb, 0.1 * base)


def convection_clamp(k):
    """wire.py:355-361 `max(-0.9, ve)` and `max(h, 0.1 base)`: factor -1, ladder on the unwinding velocity around 0.9; the
    base puts a float32 rounding boundary between the floor and the unclamped rung below it.  WIRE_LAST_FLOW is stale."""
    unwind, clamped, hb, h = _convection(k, BASE_CLAMP)
    return dict(rows={("f64", F.UNWIND_VEL): unwind, ("f64", F.WIRE_LAST_FLOW): 0.5}, decision=clamped,
                expect=h.astype(np.float32).astype(np.float64), row=("f64", F.H_BASE),
                kw={"wire": {"convection_velocity_factor": -1.0, "base_convection_coefficient": BASE_CLAMP}})


def convection_floor(k):
    """The same with the base at which float32 separates base * (1 + -0.9) from 0.1 base: a guard for the floor."""
    unwind, clamped, hb, h = _convection(k, BASE_FLOOR)
    return dict(rows={("f64", F.UNWIND_VEL): unwind, ("f64", F.WIRE_LAST_FLOW): 0.5}, decision=clamped,
                expect=h.astype(np.float32).astype(np.float64), wrong=hb.astype(np.float32).astype(np.float64), guard=True,
                row=("f64", F.H_BASE),
                kw={"wire": {"convection_velocity_factor": -1.0, "base_convection_coefficient": BASE_FLOOR}})


BURNING = {("i8", B.SPARK_STATE): 1, ("f64", F.SPARK_Y): 7.0, ("i32", I.CURRENT_MODE): 5, ("i8", B.MODE_CACHED): 1,
           ("f64", F.VOLTAGE): 24.0, ("f64", F.CURRENT): 60.0, ("f64", F.TARGET_VOLTAGE): 80.0}
RESTING = {("i8", B.SPARK_STATE): -2, ("f64", F.SPARK_Y): 7.0, ("i32", I.CURRENT_MODE): 5, ("i8", B.MODE_CACHED): 1,
           ("f64", F.TARGET_VOLTAGE): 80.0}


def on_time_end(k):
    """ignition.py:274 `duration >= ON_time`: a spark in its second microsecond, ON = 2 +- k ulp."""
    on = ulps(2.0, k)
    end = float(1 + 1) >= on
    return dict(rows={**BURNING, ("i32", I.SPARK_DUR): 1, ("f64", F.ON_TIME): on, ("f64", F.OFF_TIME): 30.0},
                decision=end, expect=np.where(end, -2, 1).astype(np.int8), row=("i8", B.SPARK_STATE))


def rest_end(k):
    """ignition.py:306-308 `duration >= ON_time + OFF_time`: resting, duration 9 + 1, ON 3, OFF = 7 +- k ulp."""
    off = ulps(7.0, k)
    end = float(9 + 1) >= 3.0 + off
    return dict(rows={**RESTING, ("i32", I.SPARK_DUR): 9, ("f64", F.ON_TIME): 3.0, ("f64", F.OFF_TIME): off},
                decision=end, expect=np.where(end, 0, -2).astype(np.int8), row=("i8", B.SPARK_STATE))


def rest_end_rounded_sum(k):
    """The same with a non-integer pair whose sum rounds: ON 0.1, OFF = 9.9 +- k ulp (0.1 + 9.9 == 10.0 in float64)."""
    off = ulps(9.9, k)
    end = float(9 + 1) >= 0.1 + off
    return dict(rows={**RESTING, ("i32", I.SPARK_DUR): 9, ("f64", F.ON_TIME): 0.1, ("f64", F.OFF_TIME): off},
                decision=end, expect=np.where(end, 0, -2).astype(np.int8), row=("i8", B.SPARK_STATE))


def on_time_fallback(k):
    """ignition.py:337 `state.ON_time or default`: ON = 0 +- k denormal steps; only 0.0 itself falls back to the 3 us."""
    on = ulps(0.0, k)
    eff = np.where(on != 0.0, on, 3.0)
    end = float(0 + 1) >= eff
    return dict(rows={**BURNING, ("i32", I.SPARK_DUR): 0, ("f64", F.ON_TIME): on, ("f64", F.OFF_TIME): 30.0},
                decision=end, expect=np.where(end, -2, 1).astype(np.int8), row=("i8", B.SPARK_STATE), middle_only=True)


def off_time_fallback(k):
    """ignition.py:343 `state.OFF_time or default`: OFF = 0 +- k denormal steps under ON 3, duration 4 + 1."""
    off = ulps(0.0, k)
    eff = np.where(off != 0.0, off, 80.0)
    end = float(4 + 1) >= 3.0 + eff
    return dict(rows={**RESTING, ("i32", I.SPARK_DUR): 4, ("f64", F.ON_TIME): 3.0, ("f64", F.OFF_TIME): off},
                decision=end, expect=np.where(end, 0, -2).astype(np.int8), row=("i8", B.SPARK_STATE), middle_only=True)


def voltage_fallback(k):
    """ignition.py:331 `state.target_voltage or default`: idle, target voltage 0 +- k denormal steps; the open voltage shows it."""
    tv = ulps(0.0, k)
    eff = np.where(tv != 0.0, tv, 80.0)
    return dict(rows={("f64", F.WORKPIECE_POS): 1000.0, ("f64", F.LAST_GAP): 990.0, ("f64", F.TARGET_VOLTAGE): tv},
                decision=tv != 0.0, expect=eff, row=("f64", F.VOLTAGE), middle_only=True)


def latch(interval, dt=1):
    def ladder(k):
        tss = interval + k
        ctrl = tss >= interval
        return dict(rows={("i32", I.SINCE_SERVO): tss.astype(np.int32), ("f64", F.WORKPIECE_POS): 1000.0, ("f64", F.LAST_GAP): 990.0},
                    decision=ctrl, expect=np.where(ctrl, 0.125, 0.0), row=("f64", F.TARGET_DELTA), servo=0.125,
                    kw={"config": {"servo_interval": interval} if dt == 1 else {"servo_interval": interval, "dt": dt}})
    ladder.__name__ = f"latch_interval_{interval}" + (f"_dt{dt}" if dt != 1 else "")
    ladder.__doc__ = f"wire_edm.py:117 `time_since_servo >= servo_interval` at interval {interval}: the servo command is latched or not."
    return ladder


# ---- config.dt = 3.  The clocks advance by 3 us per step (wire_edm.py:135-144); the generator's ON and OFF times are compared
# with `spark_status[2]`, which counts STEPS whatever dt is (ignition.py:272-275,304-309).  The ladders below sit on the step
# count's threshold while `time_since_spark_ignition` / `time_since_spark_end` (3 us per step) are already past it: a
# kernel that read ON or OFF against a clock in microseconds decides every rung the other way.  In the launches of 1, 7 and
# 50 steps that follow, `time_since_servo` steps over intervals 1, 4 and 100 without landing on them.
DT3 = {"config": {"dt": 3}}


def on_time_end_dt3(total):
    def ladder(k):
        on = ulps(float(total), k)
        end = float(total - 1 + 1) >= on
        return dict(rows={**BURNING, ("i32", I.SPARK_DUR): total - 1, ("i32", I.SINCE_IGNITION): 3 * (total - 1),
                          ("f64", F.ON_TIME): on, ("f64", F.OFF_TIME): 30.0},
                    decision=end, expect=np.where(end, -2, 1).astype(np.int8), row=("i8", B.SPARK_STATE), kw=DT3)
    ladder.__name__ = f"on_time_end_{total}_dt3"
    ladder.__doc__ = (f"ignition.py:274 `duration >= ON_time` at dt = 3: a spark in step {total} of ON = {total} +- k ulp, "
                      f"time_since_spark_ignition = {3 * (total - 1)} us.")
    return ladder


def rest_end_dt3(total):
    def ladder(k):
        off = ulps(float(total - 3), k)
        end = float(total - 1 + 1) >= 3.0 + off
        return dict(rows={**RESTING, ("i32", I.SPARK_DUR): total - 1, ("i32", I.SINCE_SPARK_END): 3 * (total - 3),
                          ("f64", F.ON_TIME): 3.0, ("f64", F.OFF_TIME): off},
                    decision=end, expect=np.where(end, 0, -2).astype(np.int8), row=("i8", B.SPARK_STATE), kw=DT3)
    ladder.__name__ = f"rest_end_{total}_dt3"
    ladder.__doc__ = (f"ignition.py:306-308 `duration >= ON_time + OFF_time` at dt = 3: resting in step {total} of ON 3 + OFF = "
                      f"{total - 3} +- k ulp, time_since_spark_end = {3 * (total - 3)} us.")
    return ladder


DT3_LADDERS = [latch(1, 3), latch(3, 3), latch(4, 3), latch(100, 3), on_time_end_dt3(2), on_time_end_dt3(3), on_time_end_dt3(4),
               rest_end_dt3(8), rest_end_dt3(9), rest_end_dt3(10)]


# mechanics.py:69-114 at the default parameters, position mode, before the first latch (target_delta = 0)
MECH = dict(omega_n=235.0, zeta=0.38, max_acceleration=3.0e5, max_jerk=1.0e8, max_speed=3.0e4)


# the acceleration ladders: damping = -256 and a limit of 2^18, so that damping * v moves by exactly one ulp per ulp of v
MECH_POW2 = dict(MECH, omega_n=256.0, zeta=0.5, max_acceleration=262144.0)


def mechanics(v, prev, x=X0, MECH=MECH):
    dt = 1 * 1e-6
    damping, stiffness, jerk_dt = -2.0 * MECH["zeta"] * MECH["omega_n"], -MECH["omega_n"] ** 2.0, MECH["max_jerk"] * dt
    a_nom = damping * v + stiffness * (x - (x + 0.0))
    a_lim = np.clip(a_nom, -MECH["max_acceleration"], MECH["max_acceleration"])
    da = a_lim - prev
    da_lim = np.clip(da, -jerk_dt, jerk_dt)
    a = prev + da_lim
    v1 = v + a * dt
    v2 = np.clip(v1, -MECH["max_speed"], MECH["max_speed"])
    return dict(a_nom=a_nom, a=a, da=da, v1=v1, v=v2, a_unlimited=prev + np.clip(a_nom - prev, -jerk_dt, jerk_dt),
                a_unjerked=prev + da)


def _far():
    return {("f64", F.WORKPIECE_POS): 1000.0, ("f64", F.LAST_GAP): 990.0}


def accel_clamp(sign):
    def ladder(k):
        amax = MECH_POW2["max_acceleration"]
        v = ulps(-sign * 1024.0, -sign * k)          # a_nom = -256 v = sign * (2^18 +- k ulp), exactly
        m = mechanics(v, np.full(len(k), sign * amax), MECH=MECH_POW2)
        return dict(rows={**_far(), ("f64", F.WIRE_VEL): v, ("f64", F.PREV_ACCEL): sign * amax}, decision=sign * m["a_nom"] > amax,
                    expect=m["a"], wrong=m["a_unlimited"], row=("f64", F.PREV_ACCEL),
                    kw={"mechanics": {k_: MECH_POW2[k_] for k_ in ("omega_n", "zeta", "max_acceleration")}})
    ladder.__name__ = f"accel_clamp_{'pos' if sign > 0 else 'neg'}"
    ladder.__doc__ = "mechanics.py:86 the acceleration clip: damping -256, limit 2^18, ladder on WIRE_VEL = -+1024 (PREV_ACCEL at the limit: no jerk clip)."
    return ladder


def jerk_clamp(sign):
    def ladder(k):
        jerk_dt = MECH["max_jerk"] * (1 * 1e-6)
        prev = ulps(-sign * jerk_dt, -sign * k)       # da = 0 - prev = sign * (jerk_dt +- k ulp), exactly
        m = mechanics(np.zeros(len(k)), prev)
        return dict(rows={**_far(), ("f64", F.PREV_ACCEL): prev}, decision=sign * m["da"] > jerk_dt,
                    expect=m["a"], wrong=m["a_unjerked"], row=("f64", F.PREV_ACCEL))
    ladder.__name__ = f"jerk_clamp_{'pos' if sign > 0 else 'neg'}"
    ladder.__doc__ = "mechanics.py:92 the jerk clip: the wire at rest, ladder on PREV_ACCEL around -+max_jerk * dt."
    return ladder


def speed_clamp(sign):
    def ladder(k):
        vmax = MECH["max_speed"]
        centre = flip_center(lambda v: sign * mechanics(v, np.zeros(len(v)))["v1"] > vmax, sign * (vmax + 100.0 * 1e-6))
        v = ulps(centre, k)
        m = mechanics(v, np.zeros(len(k)))
        return dict(rows={**_far(), ("f64", F.WIRE_VEL): v}, decision=sign * m["v1"] > vmax, expect=m["v"], wrong=m["v1"],
                    row=("f64", F.WIRE_VEL))
    ladder.__name__ = f"speed_clamp_{'pos' if sign > 0 else 'neg'}"
    ladder.__doc__ = "mechanics.py:105 the speed clip: ladder on WIRE_VEL where v + a dt crosses +-max_speed."
    return ladder


LADDERS = [hard_short, gap_clamp_zero, gap_clamp_milli, collision, target_reached, cache_gap, cache_density, cache_flow,
           removal_gate_flow, removal_gate_debris, removal_clamp, density_clamp, fast_exp_half, convection_clamp, convection_floor,
           on_time_end, rest_end, rest_end_rounded_sum, on_time_fallback, off_time_fallback, voltage_fallback,
           latch(1), latch(2), latch(1000), accel_clamp(+1), accel_clamp(-1), jerk_clamp(+1), jerk_clamp(-1),
           speed_clamp(+1), speed_clamp(-1)]


# ---- the ladders that only injected variates make observable (kernel 1's REPLAY form; OracleBackendRows on the CPU side):
# the roll under test is 1e-300, far below any Philox uniform, so a probability of 1e-217 fires and one of exactly 0 does
# not; the other short roll is 1.0 and the ignition roll 1.0 (neither fires)
RANDOM_SHORT = {"ignition": {"random_short_max_probability": 0.5, "random_short_min_gap": 2.0, "random_short_max_gap": 50.0}}


def sigmoid_cut(k):
    """ignition.py:139 `exponent > 500`: gap 50 (critical density 0.95), ladder on the density around exponent == 500;
    steepness 2000; at 500 and below the roll of 1e-300 is under 1 / (1 + e^500) and a debris short begins."""
    def exponent(rho):
        return -2000.0 * (rho - np.minimum(0.3 + 0.02 * np.maximum(0.0, 60.0 - X0), 0.95))
    centre = flip_center(lambda rho: exponent(rho) > 500, 0.95 - 0.25)
    rho = ulps(centre, k)
    cut = exponent(rho) > 500
    return dict(rows={("f64", F.DEBRIS_DENSITY): rho, ("f64", F.LAST_DENSITY): 0.0}, decision=cut,
                expect=np.where(cut, 0, 50).astype(np.int32), row=("i32", I.DEBRIS_SHORT_REM), replay=(1e-300, 1.0),
                kw={"ignition": {"sigmoid_steepness": 2000.0}})


def random_short_max_gap(k):
    """ignition.py:222 `gap >= random_short_max_gap`: x = 10, wp = 60 +- k ulp; below it the ramp's last value (~1e-17)
    is above the roll of 1e-300 and a random short begins."""
    wp = ulps(60.0, k)
    gap = np.maximum(0.0, wp - X0)
    off = gap >= 50.0
    return dict(rows={("f64", F.WORKPIECE_POS): wp, ("f64", F.LAST_GAP): 50.0}, decision=off,
                expect=np.where(off, 0, 100).astype(np.int32), row=("i32", I.RANDOM_SHORT_REM), replay=(1.0, 1e-300), kw=RANDOM_SHORT)


REPLAY_LADDERS = [sigmoid_cut, random_short_max_gap]


# ------------------------------------------------------------------ running a ladder
def env_kw(spec):
    kw = spec.get("kw", {})
    return dict(config=EnvironmentConfig(target_cutting_distance=5000.0, **kw.get("config", {})),
                ignition_params=IgnitionModuleParameters(**kw.get("ignition", {})),
                wire_params=WireModuleParameters(segment_len=SEGMENT_LEN, **kw.get("wire", {})),
                dielectric_params=DielectricModuleParameters(**kw.get("dielectric", {})),
                mechanics_params=MechanicsModuleParameters(**kw.get("mechanics", {})))


def start(env, spec):
    """The common start state (an idle generator over a clean 50 um gap whose caches are valid), then the ladder's rows."""
    env.reset(seed=SEED)
    rows = {("f64", F.WIRE_POS): X0, ("f64", F.WORKPIECE_POS): 60.0, ("f64", F.TARGET_POS): 5000.0, ("f64", F.LAST_GAP): 50.0,
            ("f64", F.LAST_DENSITY): 0.0, ("f64", F.DEBRIS_VOLUME): 0.0, ("f64", F.DEBRIS_DENSITY): 0.0, ("f64", F.FLOW): 1.0,
            ("f64", F.WIRE_LAST_FLOW): 1.0}
    rows.update(spec["rows"])
    for (block, row), value in rows.items():
        view = getattr(env.state, block)
        value = np.broadcast_to(np.asarray(value), (N,))
        view[int(row), :N] = torch.from_numpy(np.array(value)).to(device=view.device, dtype=view.dtype)
    if spec.get("replay") is not None:
        table = np.empty((sum(LAUNCHES), _abi.REPLAY_SLOTS))
        table[:, 0], table[:, 1] = spec["replay"]   # (debris roll, random-short roll)
        table[:, 2] = 1.0                       # no ignition
        table[:, 3], table[:, 4] = 7.0, 1000.0
        env.bind_rng_replay(table)


def run(env, spec):
    act = env.make_action(spec.get("servo", 0.0), 80.0, 9, 3.0, 30.0)
    blocks = []
    for us in LAUNCHES:
        env.step_many(act, us)
        blocks.append(env.state.clone_blocks())
    return blocks


def oracle_run(ladder):
    spec = ladder(layout(ladder(RUNGS)["decision"]))
    backend = OracleBackendRows if spec.get("replay") is not None else OracleBackend
    env = WireEDMEnv(num_envs=N, device="cpu", backend=backend, **env_kw(spec))
    start(env, spec)
    return spec, run(env, spec)


def observed(spec, blocks):
    block, row = spec["row"]
    got = blocks[block][int(row), :N].numpy()
    return spec["observe"](got) if "observe" in spec else got


def check_observable(ladder, spec, blocks):
    """The oracle's row after the first microsecond equals the restatement on every rung, and the ladder tells the sides
    (or, a guard ladder, the clamp from its absence) apart on adjacent rungs around the threshold."""
    got, want = observed(spec, blocks[0]), np.asarray(spec["expect"])
    # (the restatement is of the one line: an environment whose ignition roll succeeded in this very microsecond -- a
    # handful among 230 at a 50 um gap -- also dug a crater, which moves the workpiece and adds debris)
    calm = blocks[0]["i32"][int(I.SPARK_COUNT), :N].numpy() == 0
    assert calm.sum() >= N // 2 and all(calm[192:][np.arange(N - 192) % len(RUNGS) == r].any() for r in range(len(RUNGS)))
    same = (got == want) | ((got != got) & (want != want)) | ~calm
    assert same.all(), (ladder.__name__, np.nonzero(~same)[0][:8], got[~same][:4], want[~same][:4])
    on_rungs = ladder(RUNGS)
    d, e = on_rungs["decision"], np.asarray(on_rungs["expect"])
    if "wrong" in on_rungs:
        assert (np.asarray(on_rungs["wrong"]) != e).any(), ladder.__name__
    if on_rungs.get("guard"):
        return
    flips = np.nonzero(d[1:] != d[:-1])[0]
    if on_rungs.get("middle_only"):   # `x or default`: only the middle rung, 0.0 itself, falls back
        assert list(d) == [True, True, False, True, True] and e[1] != e[2] != e[3], (ladder.__name__, d, e)
        return
    # two adjacent rungs straddle the threshold (which two is the float64 arithmetic's business: 3 + (7 + 1 ulp) is a tie
    # that rounds to 10), and the named row tells the sides apart: one side holds a value the other never does.  (On an
    # exact-equality rung a clip returns the value it was given, so that rung may agree with its clipped neighbour.)
    assert len(flips) == 1, (ladder.__name__, d)
    assert set(e[d].tolist()) - set(e[~d].tolist()) or set(e[~d].tolist()) - set(e[d].tolist()), (ladder.__name__, e)


@pytest.mark.parametrize("ladder", LADDERS + DT3_LADDERS + REPLAY_LADDERS, ids=lambda f: f.__name__)
def test_oracle_decides_each_rung_like_the_reference_line(ladder):
    spec, blocks = oracle_run(ladder)
    check_observable(ladder, spec, blocks)
    if ladder in DT3_LADDERS:   # the clock of these runs: 3 us per step
        assert blocks[-1]["i32"][int(I.TIME), :N].tolist() == [3 * sum(LAUNCHES)] * N


def test_cavity_coefficient_restatement():
    env = WireEDMEnv(num_envs=N, device="cpu", backend=OracleBackend, **env_kw({}))
    env.reset(seed=SEED)
    env.state.workpiece_position, env.state.wire_position, env.state.target_position = 60.0, 10.0, 5000.0
    env.step_many(env.make_action(0.0, 80.0, 9, 3.0, 30.0), 1)
    calm = env.state.spark_count.numpy() == 0
    assert calm.sum() > N // 2 and (env.state.cavity_volume.numpy()[calm] == CAVITY_COEFF * (50.0 * 0.001)).all()


# ------------------------------------------------------------------------------------------------------------ GPU
KERNELS = [(1, 0), (5, 0), (6, 0), (6, 4), (6, 16), (2, 0), (3, 1), (3, 2), (3, 4), (3, 8), (3, 16), (4, 1), (4, 2), (4, 4),
           (4, 8), (10, 0), (2, 4), (2, 16)]   # tests/test_gpu_parity.py: KERNELS
SERVED = [(9, 4), (9, 8)]
ALL = KERNELS + SERVED + [(7, 1), (7, 2), (8, 0), (0, 0)]   # (0, 0): the automatic plan
# families whose fast path is the instantiation that also carries burning sparks (quiet_prelude_t<true>, a compile-time
# property of the family: kPackedDense in wedm_common.h), and those that run the plain one
DENSE_QUIET = {int(_abi.KERNEL.PACKED), int(_abi.KERNEL.SERVED), int(_abi.KERNEL.REGS), int(_abi.KERNEL.WIDE)}


def gpu_against(ladder, spec, refs, kernels):
    """Every kernel of `kernels` against the oracle's blocks after every launch.  Returns (ran, skipped by name)."""
    from sparc_amd._lib import WedmError

    ran, skipped = [], []
    for variant, lanes in kernels:
        gpu = WireEDMEnv(num_envs=N, device="cuda:0", **env_kw(spec))
        start(gpu, spec)
        gpu.set_kernel(variant, lanes)
        act = gpu.make_action(spec.get("servo", 0.0), 80.0, 9, 3.0, 30.0)
        forms = []
        try:
            for i, us in enumerate(LAUNCHES):
                gpu.step_many(act, us)
                torch.cuda.synchronize()
                name, form = gpu._backend.last_kernel(), gpu._backend.last_form()
                diffs = block_diffs(gpu.state.clone_blocks(), refs[i], N)
                assert not diffs, f"{ladder.__name__} ladder, kernel {name} ({variant},{lanes}), launch {i} ({us} us):\n" + "\n".join(diffs[:10])
                if variant != 0:
                    assert form[0] == variant and (lanes == 0 or form[1] == lanes), (ladder.__name__, variant, lanes, form)
                forms.append(form)
        except WedmError as exc:
            assert "UNSUPPORTED" in str(exc), exc
            skipped.append(f"{ladder.__name__}: kernel ({variant},{lanes}) UNSUPPORTED")
            continue
        ran.append((variant, lanes, tuple(forms)))
        gpu.close()
    return ran, skipped


@pytest.mark.gpu
@pytest.mark.parametrize("ladder", LADDERS + DT3_LADDERS, ids=lambda f: f.__name__)
def test_every_kernel_decides_the_threshold_at_its_edge(ladder):
    spec, refs = oracle_run(ladder)
    check_observable(ladder, spec, refs)
    ran, skipped = gpu_against(ladder, spec, refs, ALL)
    print(f"{ladder.__name__}: {len(ran)} kernels, forms {sorted({f for *_, fs in ran for f in fs})}; skipped: {skipped}")
    assert not skipped, skipped       # every family listed runs the 128-segment uniform batch today
    assert [(v, L) for v, L, _ in ran] == ALL
    families = {f[0] for *_, fs in ran for f in fs}
    assert DENSE_QUIET <= families and {int(_abi.KERNEL.FUSED), int(_abi.KERNEL.GLOBAL)} <= families, families


@pytest.mark.gpu
@pytest.mark.parametrize("ladder", REPLAY_LADDERS, ids=lambda f: f.__name__)
def test_injected_variates_form_decides_the_threshold_at_its_edge(ladder):
    spec, refs = oracle_run(ladder)
    check_observable(ladder, spec, refs)
    ran, skipped = gpu_against(ladder, spec, refs, [(1, 0)])
    assert not skipped and len(ran) == 1
    assert all(f[0] == int(_abi.KERNEL.GLOBAL) and f[2] & int(_abi.FORM.REPLAY) for f in ran[0][2]), ran
