"""The sensor model (sparc_amd/sensor.py) on the host side: the ABI mirror of ``wedm_sensor_desc`` and the
export with its refusals (no device is needed), `sensor_reference` on hand-worked cases, its statistics against bounds derived
from the distributions, `Sensor` through the vector adapter on the CPU oracle backend (which has no ``sensor`` and so runs the
definition), checkpoints of whole stacks cut at every control step, and `PolicyNet` on a store wider than its ``obs_dim``."""
from __future__ import annotations

import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from sparc_amd import (MEASURABLE_OBS_NAMES, Channel, Normalizer, PolicyHead, PolicyNet, Sensor, WireEDMVectorEnv, _abi, _lib,
                       sensor_reference)
from sparc_amd.sensor import CALIBRATION_STREAM0, STREAM0
from tests import _resume_common as rc
from tests import _sensor_common as sc
from tests import _snapshot_common as snap
from tests._sensor_common import SEED, T0, Problem

ROOT = Path(__file__).resolve().parent.parent
SN = _abi.SN
INF = math.inf


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_desc_struct_mirror_matches_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wedm_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(wedm_sensor_desc));', '  printf("planesize %zu\\n", sizeof(wedm_norm_plane));']
    for field, _ in _abi.SensorDesc._fields_:
        lines.append(f'  printf("{field} %zu\\n", offsetof(wedm_sensor_desc, {field}));')
    lines += ['  printf("consts %d %d %d %u abi %d\\n", WEDM_SENSOR_FIELDS, WEDM_SENSOR_ROUTES, WEDM_SENSOR_MAX_DELAY, WEDM_SENSOR_STREAM0, '
              'WEDM_ABI_VERSION);',
              '  printf("fields %d %d %d %d %d %d routes %d %d\\n", WEDM_SN_SIGMA, WEDM_SN_GAIN_SPREAD, WEDM_SN_OFFSET_SPREAD, WEDM_SN_LSB, '
              'WEDM_SN_LO, WEDM_SN_HI, WEDM_SN_SOURCE, WEDM_SN_MAX_DELAY);', "  return 0;", "}"]
    src = tmp_path / "desc.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "desc"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    out = dict(row.split(" ", 1) for row in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("size")) == C.sizeof(_abi.SensorDesc) and int(out.pop("planesize")) == C.sizeof(_abi.NormPlane)
    assert out.pop("consts") == f"{_abi.SENSOR_FIELDS} {_abi.SENSOR_ROUTES} {_abi.SENSOR_MAX_DELAY} {_abi.SENSOR_STREAM0} abi 4"
    assert out.pop("fields") == " ".join(str(int(k)) for k in SN) + f" routes {_abi.SN_SOURCE} {_abi.SN_MAX_DELAY}" == "0 1 2 3 4 5 routes 0 1"
    assert (_abi.SENSOR_MAX_DELAY, _abi.SENSOR_STREAM0) == (7, 0xA0000000)
    assert {k: int(v) for k, v in out.items()} == {f: getattr(_abi.SensorDesc, f).offset for f, _ in _abi.SensorDesc._fields_}


def test_the_call_is_exported_and_the_abi_version_stays():
    assert "wedm_sensor" in _lib.EXPORTS and hasattr(_lib.HipBackend, "sensor")
    L = _lib.load()
    assert L.wedm_sensor is not None and L.wedm_abi_version() == _abi.ABI_VERSION == 4


def test_the_streams_stay_clear_of_each_other_and_of_the_other_calls():
    top = _abi.NORM_MAX_COLUMNS - 1
    noise = range(STREAM0, STREAM0 + 64 * top)
    calib = range(CALIBRATION_STREAM0, CALIBRATION_STREAM0 + top)
    assert noise.stop <= calib.start and calib.stop < _abi.HEAD_STREAM0 and noise.start > 0x80000000 + (1 << 20)
    assert 0xE0000000 not in noise and 0xE0000000 not in calib


def test_bad_arguments_are_refused_before_anything_is_launched():
    """The blocks are host memory in one arena: a call that launched would fail (there is no device, or the device cannot
    read them); every case returns WEDM_ERR_BAD_ARG with its text, and leaves every byte of the arena as it was."""
    L = _lib.load()
    rng = np.random.default_rng(1)
    N = 100
    p = Problem(rng, N, (16, 8), 5, 8, "all", pad=3)
    arena = p.buf.copy()
    base = arena.ctypes.data
    at = lambda name: base + p.layout[name][0]   # noqa: E731

    def desc(**kw):
        d = p.desc(base, T0)
        for key, value in kw.items():
            if key.startswith("plane"):
                setattr(d.plane[int(key[5])], key[7:], value)
            else:
                setattr(d, key, value)
        return d

    def refused(d, what, text):
        assert L.wedm_sensor(C.byref(d), None) == _abi.ERR_BAD_ARG, what
        got = (L.wedm_last_error(None) or b"").decode()
        assert got.startswith("wedm_sensor: ") and text in got, (what, got)
        assert arena.tobytes() == p.buf.tobytes(), what

    assert L.wedm_sensor(None, None) == _abi.ERR_BAD_ARG and L.wedm_last_error(None) == b"wedm_sensor: null descriptor"
    for flags in (1, 2, -1, 1 << 30):
        refused(desc(flags=flags), f"flags {flags}", "undefined flag bits")
    for n in (0, -5):
        refused(desc(num_envs=n), f"num_envs {n}", "num_envs must be positive")
    refused(desc(plane0_n_rows=-1), "a negative n_rows", "negative n_rows")
    refused(desc(plane0_n_rows=0, plane1_n_rows=0), "no source column", "C_in outside [1, 159]")
    refused(desc(plane0_n_rows=100, plane1_n_rows=60), "160 source columns", "C_in outside [1, 159]")
    for n_out in (0, -1, 160):
        refused(desc(n_out=n_out), f"n_out {n_out}", "n_out outside [1, 159]")
    for ring_len in (0, -1, 9):
        refused(desc(ring_len=ring_len), f"ring_len {ring_len}", "ring_len outside [1, 8]")
    refused(desc(ring=None), "ring NULL with ring_len 8", "ring is null though ring_len > 1")
    refused(desc(plane0_stride=N - 1), "plane 0's stride", "plane 0: stride smaller than num_envs")
    refused(desc(plane1_stride=N - 1), "plane 1's stride", "plane 1: stride smaller than num_envs")
    refused(desc(out_stride=N - 1), "out_stride", "out_stride smaller than num_envs")
    refused(desc(ring_stride=N - 1), "ring_stride", "ring_stride smaller than num_envs")
    # a needed block NULL, a block not aligned to its element
    refused(desc(plane0_rows=None), "plane 0 NULL", "plane 0 rows is null or not aligned to its element")
    refused(desc(plane1_rows=None), "plane 1 NULL", "plane 1 rows is null or not aligned to its element")
    for name in ("chan", "route", "out", "pos", "age"):
        refused(desc(**{name: None}), f"{name} NULL", f"{name} is null or not aligned to its element")
    for name, off in (("chan", 4), ("route", 2), ("episode", 4), ("out", 2), ("ring", 1), ("pos", 2), ("age", 3)):
        refused(desc(**{name: at(name) + off}), f"{name} misaligned", f"{name} is null or not aligned to its element")
    refused(desc(plane1_rows=at("plane1") + 2), "plane 1 misaligned", "plane 1 rows is null or not aligned to its element")
    # what is written over an input, first and last byte that the call may touch, and over each other
    S, OS, RS = p.S, p.OS, p.RS
    refused(desc(out=at("plane0") - 4 * (4 * OS + N) + 4), "out's last word on plane 0's first", "out overlaps plane 0 rows")
    refused(desc(out=at("plane1") + 4 * (7 * S + N - 1)), "out's first word on plane 1's last", "out overlaps plane 1 rows")
    refused(desc(out=at("chan") + 8 * 6 * 5 - 4), "out on the table's last word", "out overlaps chan")
    refused(desc(pos=at("route") + 4 * 2 * 5 - 4), "pos on the routes' last word", "pos overlaps route")
    refused(desc(age=(at("first") + N - 1) & ~3), "age on first's last byte", "age overlaps first")
    refused(desc(ring=(at("mask") + N - 1) & ~3), "the ring on the mask's last byte", "ring overlaps mask")
    refused(desc(ring=at("episode") + 8 * N - 4), "the ring's first word on episode's last", "ring overlaps episode")
    refused(desc(ring=at("out") + 4 * (4 * OS + N - 1)), "the ring on out's last word", "ring overlaps out")
    refused(desc(pos=at("ring") + 4 * ((8 * 24 - 1) * RS + N - 1)), "pos on the ring's last word", "pos overlaps ring")
    refused(desc(age=at("pos") + 4 * (N - 1)), "age on pos's last word", "age overlaps pos")
    refused(desc(age=at("out")), "age on out", "age overlaps out")
    # with a ring of one the ring is not looked at: the call passes the checks (and fails only at the launch, or not at all)
    d = desc(ring_len=1, ring=at("mask") + 1, ring_stride=0)
    assert L.wedm_sensor(C.byref(d), None) != _abi.ERR_BAD_ARG or "ring" not in (L.wedm_last_error(None) or b"").decode()


# ------------------------------------------------------------------------------------------------ the definition, by hand
IDENTITY = (0.0, 0.0, 0.0, 0.0, -INF, INF)


def run(src, channels, L=1, first=None, mask=None, episode=None, state=None, t=0, seed=SEED, offset=0, trace=None):
    """One call of the definition on ``src`` (``[C_in, N]``); ``channels``: (settings of six, source, max_delay) each;
    ``state``: (out, ring, pos, age) carried from the call before.  Returns the state."""
    src = np.asarray(src, dtype=np.float32)
    C_in, N = src.shape
    chan = np.array([c[0] for c in channels], dtype=np.float64).T.copy()
    route = np.array([[c[1], c[2]] for c in channels], dtype=np.int32).T.copy()
    if state is None:
        state = (np.full((len(channels), N), 77.0, dtype=np.float32), np.full((L, C_in, N), 55.0, dtype=np.float32) if L > 1 else None,
                 np.full(N, 12345, dtype=np.int32), np.full(N, -99, dtype=np.int32))
    out, ring, pos, age = state
    as_u8 = lambda a: None if a is None else np.asarray(a, dtype=np.uint8)   # noqa: E731
    sensor_reference([src], chan, route, as_u8(first), as_u8(mask), None if episode is None else np.asarray(episode, dtype=np.int64),
                     out, ring, pos, age, seed=seed, t=t, env_id_offset=offset, num_envs=N, ring_len=L, trace=trace)
    return state


def bits(a) -> list:
    return np.asarray(a, dtype=np.float32).view(np.uint32).reshape(-1).tolist()


def test_the_identity_channel_copies_bits_and_a_nan_comes_out_canonical():
    special = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x3F800001, 0x00000000],
                       dtype=np.uint32).view(np.float32)
    nans = np.array([0x7FC12345, 0xFFA00001, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)
    out = run([special, special[::-1]], [(IDENTITY, 1, 0), (IDENTITY, 0, 0)])[0]
    assert bits(out[0]) == bits(special[::-1]) and bits(out[1]) == bits(special)
    out = run([nans], [(IDENTITY, 0, 0)])[0]
    assert bits(out) == [0x7FC00000] * 4
    # and with a ring: the undelayed sample is the source itself
    out, ring, _, _ = run([special], [(IDENTITY, 0, 0)], L=3)
    assert bits(out[0]) == bits(special) and bits(ring[0, 0]) == bits(special) and (ring[1:] == 55.0).all()


def test_lsb_ties_go_to_even_and_lo_hi_saturate_and_a_nan_passes_both():
    x = [0.5, 1.5, 2.5, -0.5, -1.5, 3.49, 0.125, -2.5]
    out = run([x], [((0, 0, 0, 1.0, -INF, INF), 0, 0), ((0, 0, 0, 0.25, -INF, INF), 0, 0), ((0, 0, 0, 0.0, -1.0, 2.0), 0, 0),
                    ((0, 0, 0, 1.0, 1.0, 1.0), 0, 0)])[0]
    assert out[0].tolist() == [0.0, 2.0, 2.0, -0.0, -2.0, 3.0, 0.0, -2.0] and bits(out[0, 3]) == [0x80000000]
    assert out[1].tolist() == [0.5, 1.5, 2.5, -0.5, -1.5, 3.5, 0.0, -2.5]       # 0.125 / 0.25 = 0.5 -> 0 (even)
    assert out[2].tolist() == [0.5, 1.5, 2.0, -0.5, -1.0, 2.0, 0.125, -1.0]
    assert out[3].tolist() == [1.0] * 8
    nan = run([[np.nan, np.inf, -np.inf]], [((0, 0, 0, 0.5, -1.0, 2.0), 0, 0)])[0]
    assert bits(nan[0]) == [0x7FC00000] + bits([2.0, -1.0])
    # a negative lsb is off; lo above hi: lo first, then hi
    assert run([[0.3, 5.0]], [((0, 0, 0, -1.0, 2.0, -2.0), 0, 0)])[0][0].tolist() == [-2.0, -2.0]


def test_a_delay_never_reaches_before_a_first_and_masked_environments_keep_everything():
    """Channel 0 is delayed by exactly d (max_delay chosen, environments picked where the drawn delay equals it); environment
    1 restarts at call 3; environment 2 is masked out at calls 2 and 3."""
    N, L = 4000, 4
    chans = [(IDENTITY, 0, 3), (IDENTITY, 0, 0)]
    state, history = None, []
    for call in range(7):
        src = np.full((1, N), float(call + 1), dtype=np.float32)
        first = np.zeros(N, dtype=np.uint8)
        mask = np.ones(N, dtype=np.uint8)
        if call == 0:
            first[:] = 1
        if call == 3:
            first[1::3] = 9
        if call in (2, 3):
            mask[2::3] = 0
        before = None if state is None else [None if a is None else a.copy() for a in state]
        trace: dict = {}
        state = run(src, chans, L=L, first=first, mask=mask, state=state, t=call, trace=trace)
        out, ring, pos, age = state
        d = trace["delay"][0]
        assert set(d.tolist()) == {0, 1, 2, 3} and (trace["delay"][1] == 0).all()
        live = mask != 0
        # what the episode's clock says: samples since the first, the masked calls not counted
        since = np.full(N, call)
        since[1::3] = call if call < 3 else call - 3
        since[2::3] = call - (call >= 2) - (call >= 3)
        assert (age[live] == np.minimum(since, L - 1)[live]).all()
        want = (call + 1) - np.minimum(d, since)
        # the sources hold the call number, so a reading delayed by d_eff calls is call + 1 - d_eff -- for the environments that
        # took part in every call so far (those that skipped calls read the sample of that many of THEIR calls ago)
        plain = np.ones(N, dtype=bool)
        plain[2::3] = call < 2
        assert (out[0][live & plain] == want[live & plain]).all(), call
        assert (out[1][live] == call + 1).all()
        if before is not None:
            frozen = ~live
            for now, was in zip(state, before):
                if now is not None:
                    assert (now[..., frozen] == was[..., frozen]).all(), "a masked environment keeps output, ring, pos and age"
        history.append(trace["d_eff"][0].copy())
    assert any((h < d).any() for h in history) and any(((h == d) & (d > 0)).any() for h in history)
    # an environment that restarted never reads a sample from before the restart: after call 3 its reading is >= 4
    assert (out[0][1::3] >= 4.0).all()


def test_garbage_state_of_a_first_environment_changes_nothing_and_the_table_is_clamped():
    rng = np.random.default_rng(3)
    src = rng.standard_normal((3, 50)).astype(np.float32)
    chans = [((0.5, 0.1, 0.2, 0.125, -3.0, 3.0), 1, 2), (IDENTITY, 2, 1)]
    clean = run(src, chans, L=3, first=np.ones(50))
    for pos_v, age_v in ((-7, 2 ** 31 - 1), (2 ** 31 - 1, -2 ** 31), (1, 1)):
        state = (np.full((2, 50), 77.0, dtype=np.float32), np.full((3, 3, 50), 55.0, dtype=np.float32),
                 np.full(50, pos_v, dtype=np.int32), np.full(50, age_v, dtype=np.int32))
        got = run(src, chans, L=3, first=np.ones(50), state=state)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, clean))
    # a foreign pos / age of an environment that goes on is clamped into the ring
    state = (np.zeros((2, 50), dtype=np.float32), np.zeros((3, 3, 50), dtype=np.float32), np.full(50, 99, dtype=np.int32),
             np.full(50, -5, dtype=np.int32))
    _, _, pos, age = run(src, chans, L=3, first=np.zeros(50), state=state)
    assert (pos == 0).all() and (age == 1).all()
    # SOURCE and MAX_DELAY outside their ranges are the nearest end of them
    for (s, md), (cs, cmd) in (((-4, -1), (0, 0)), ((1000, 99), (2, 2)), ((-2 ** 31, 2 ** 31 - 1), (0, 2)), ((2 ** 31 - 1, -2 ** 31), (2, 0))):
        states = []
        for source, delay in ((s, md), (cs, cmd)):
            st = None
            for call in range(4):
                st = run(src + call, [((0.0, 0.1, 0.0, 0.0, -INF, INF), source, delay)], L=3, first=[call == 0] * 50, state=st, t=call)
            states.append(st)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(*states)), (s, md)


def test_calibration_is_fixed_for_the_episode_and_noise_is_fresh_for_every_call():
    N = 64
    src = np.full((1, N), 10.0, dtype=np.float32)
    calib = [((0.0, 0.1, 0.5, 0.0, -INF, INF), 0, 0)]
    a = run(src, calib, t=0, episode=np.full(N, 3))[0].copy()
    b = run(src, calib, t=1, episode=np.full(N, 3))[0].copy()
    c = run(src, calib, t=1, episode=np.full(N, 4))[0].copy()
    assert a.tobytes() == b.tobytes() and (a != c).mean() > 0.9 and len(set(a[0].tolist())) > N // 2
    noise = [((0.5, 0.0, 0.0, 0.0, -INF, INF), 0, 0)]
    a = run(src, noise, t=0, episode=np.full(N, 3))[0].copy()
    b = run(src, noise, t=1, episode=np.full(N, 3))[0].copy()
    c = run(src, noise, t=0, episode=np.full(N, 4))[0].copy()
    assert a.tobytes() == c.tobytes() and (a != b).mean() > 0.9
    # the global id, not the place in the batch: environments [32, 64) of a batch at offset 0 are [0, 32) of one at offset 32
    both = [calib[0], noise[0]]
    whole = run(src, both, t=5, episode=np.arange(N))[0]
    part = run(src[:, 32:], both, t=5, episode=np.arange(32, N), offset=32)[0]
    assert whole[:, 32:].tobytes() == part.tobytes()
    wrapped = run(src, both, t=5, offset=2 ** 32 - 3)[0]
    assert wrapped[:, 3:].tobytes() == run(src[:, 3:], both, t=5, offset=0)[0].tobytes()


# ------------------------------------------------------------------------------------------------ statistics
E, T = 512, 256
n = E * T   # 2^17 (environment, step) draws


def _draws(chans, seed, episodes=False):
    """``[T, C, E]`` traces over T calls of E environments (with ``episodes`` every call is a new episode)."""
    src = np.zeros((1, E), dtype=np.float32)
    keep = {"noise": [], "gain": [], "offset": [], "delay": []}
    for t in range(T):
        trace: dict = {}
        run(src, chans, L=8, t=t, seed=seed, episode=np.arange(E) * T + t if episodes else None, trace=trace)
        for k in keep:
            keep[k].append(trace[k])
    return {k: np.stack(v) for k, v in keep.items()}


def test_the_noise_has_the_normal_distributions_mean_and_variance_and_is_uncorrelated():
    """Bounds from the distribution, five standard errors each: the mean of n standard normals has deviation 1 / sqrt(n), their
    sample variance sqrt(2 / n), the sample correlation of two independent sequences 1 / sqrt(n)."""
    sigma = 0.75
    chans = [((sigma, 0, 0, 0, -INF, INF), 0, 0), ((sigma, 0, 0, 0, -INF, INF), 0, 0)]
    src = np.zeros((1, E), dtype=np.float32)
    outs = np.stack([run(src, chans, t=t, seed=11)[0].astype(np.float64).copy() for t in range(T)])   # [T, 2, E]
    x = outs[:, 0].reshape(-1)
    assert x.size == n == 2 ** 17
    assert abs(x.mean()) <= 5 * sigma / math.sqrt(n)
    assert abs(x.var() - sigma ** 2) <= 5 * sigma ** 2 * math.sqrt(2 / n)
    corr = lambda a, b: float(np.corrcoef(a.reshape(-1), b.reshape(-1))[0, 1])   # noqa: E731
    bound = 5 / math.sqrt(n)
    assert abs(corr(outs[:, 0], outs[:, 1])) <= bound, "two channels"
    assert abs(corr(outs[:-1, 0], outs[1:, 0])) <= 5 / math.sqrt(n - E), "consecutive steps"
    assert abs(corr(outs[:, 0, :-1], outs[:, 0, 1:])) <= 5 / math.sqrt(n - T), "neighbouring environments"


def test_gain_offset_and_delay_are_uniform_over_their_ranges():
    gs, os_ = 0.2, 1.5
    tr = _draws([((0, gs, os_, 0, -INF, INF), 0, 7), ((0, 0, 0, 0, -INF, INF), 0, 3)], seed=12, episodes=True)
    gain, off = tr["gain"][:, 0].reshape(-1), tr["offset"][:, 0].reshape(-1)
    assert gain.size == n and (np.abs(gain - 1.0) <= gs).all() and (np.abs(off) <= os_).all()
    # a uniform on [-a, a] has deviation a / sqrt(3)
    assert abs(gain.mean() - 1.0) <= 5 * gs / math.sqrt(3 * n) and abs(off.mean()) <= 5 * os_ / math.sqrt(3 * n)
    assert abs(np.corrcoef(gain, off)[0, 1]) <= 5 / math.sqrt(n)
    for c, md in ((0, 7), (1, 3)):
        d = tr["delay"][:, c].reshape(-1)
        p = 1.0 / (md + 1)
        share = np.bincount(d, minlength=md + 1) / n
        assert share.size == md + 1 and (np.abs(share - p) <= 5 * math.sqrt(p * (1 - p) / n)).all(), (c, share)


# ------------------------------------------------------------------------------------------------ the class and the adapter
def plain_vec(n=6, sensor=None, **kw):
    return WireEDMVectorEnv(snap.make("cpu", n, "pulse", "s13"), max_episode_steps=3000, sensor=sensor, **kw)


def test_names_actor_dim_and_the_measurable_columns():
    assert MEASURABLE_OBS_NAMES == ("wire_velocity", "voltage", "current", "spark_state", "spark_pulses", "short_pulses",
                                    "short_steps", "current_sum", "energy_sum")
    s = Sensor([Channel("voltage", sigma=0.5), Channel("current", name="amps", lsb=0.1)], privileged=("gap", "tmax"))
    vec = plain_vec(sensor=s, wire_profile_bins=2)
    try:
        assert s.actor_dim == vec.actor_obs_dim == 2 and vec.obs_names == ("voltage", "amps", "priv.gap", "priv.tmax")
        assert vec.single_observation_space.shape == (4,) and vec.raw_obs_names[:8] == _abi.OBS_NAMES and len(vec.raw_obs_names) == 19
        obs, info = vec.reset(seed=1)
        assert obs.shape == (6, 4) and info["raw_observation"].shape == (6, 19)
        assert torch.equal(obs[:, 2], info["raw_observation"][:, 0]) and torch.equal(obs[:, 3], info["raw_observation"][:, 7])
        st = vec._settings()
        assert st["obs_names"] == vec.obs_names and st["sensor_actor_dim"] == 2 and st["sensor_fingerprint"] == s.fingerprint()
    finally:
        vec.close()
    everything = Sensor([Channel("voltage")], privileged="all")
    vec = plain_vec(sensor=everything)
    try:
        assert vec.obs_names == ("voltage",) + tuple(f"priv.{n}" for n in vec.raw_obs_names)
    finally:
        vec.close()


def test_constructor_and_bind_refusals():
    for kw, word in ((dict(sigma=-1.0), "sigma"), (dict(sigma=math.nan), "sigma"), (dict(gain_spread=math.inf), "gain_spread"),
                     (dict(offset_spread=-0.1), "offset_spread"), (dict(lsb=-1.0), "lsb"), (dict(lsb=math.inf), "lsb"),
                     (dict(lo=1.0, hi=0.0), "lo <= hi"), (dict(lo=math.nan), "lo <= hi"), (dict(max_delay=8), "max_delay"),
                     (dict(max_delay=-1), "max_delay"), (dict(max_delay=1.5), "max_delay")):
        with pytest.raises(ValueError, match=word):
            Channel("voltage", **kw)
    with pytest.raises(ValueError, match="non-empty"):
        Sensor([])
    with pytest.raises(ValueError, match="privileged"):
        Sensor([Channel("voltage")], privileged="some")
    for sensor, word in ((Sensor([Channel("volts")]), "unknown source 'volts'"), (Sensor([Channel("voltage")], privileged=("nope",)), "unknown source"),
                         (Sensor([Channel("voltage"), Channel("voltage")]), "more than once"),
                         (Sensor([Channel("voltage", name="priv.gap")], privileged=("gap",)), "more than once"),
                         (Sensor([Channel("wire_mean")]), "unknown source")):
        env = snap.make("cpu", 4, "plain", "s13")
        with pytest.raises(ValueError, match=word):
            WireEDMVectorEnv(env, sensor=sensor)
        env.close()
    s = Sensor([Channel("voltage")])
    vec = plain_vec(sensor=s)
    env = snap.make("cpu", 4, "plain", "s13")
    with pytest.raises(ValueError, match="already serves"):
        WireEDMVectorEnv(env, sensor=s)
    env.close()
    vec.close()
    with pytest.raises(ValueError, match="serves no adapter"):
        Sensor([Channel("voltage")]).state_dict()


def _noisy_vec(n=8, seed=5, **kw):
    env = snap.make("cpu", n, "pulse", "s13")
    return WireEDMVectorEnv(env, max_episode_steps=3000, sensor=sc.noisy_sensor(tuple(env.obs_names), seed=seed), **kw)


def _drive(vec, steps, seed=3):
    vec.reset(seed=seed)
    action = snap.scenario(vec.env, seed=seed)
    for _ in range(steps):
        out = vec.step(action)
    return action, out


def test_the_checkpoint_round_trip_and_its_refusals():
    a, b = _noisy_vec(), _noisy_vec(seed=6)
    try:
        action, _ = _drive(a, 4)
        _drive(b, 2, seed=4)
        sd = a.state_dict()
        assert set(sd["sensor"]) == {"seed", "t", "fingerprint", "num_envs", "out", "ring", "pos", "age"} and sd["sensor"]["t"] == 5
        b.load_state_dict(sd)
        rc.assert_equal(sc.sensor_blocks(b.sensor), sc.sensor_blocks(a.sensor), "the sensor after the load")
        for _ in range(3):
            got, want = b.step(action), a.step(action)
            assert got[0].numpy().tobytes() == want[0].numpy().tobytes()
        rc.assert_equal(sc.sensor_blocks(b.sensor), sc.sensor_blocks(a.sensor), "three steps later")
    finally:
        a.close()
        b.close()
    # another channel set, another batch size, a sensor on one side only: refused before a byte changes
    env = snap.make("cpu", 8, "pulse", "s13")
    other = WireEDMVectorEnv(env, max_episode_steps=3000, sensor=Sensor([Channel(n, sigma=0.1 if n == "voltage" else 0.0, max_delay=3 if n == "current" else 0)
                                                                         for n in MEASURABLE_OBS_NAMES if n in env.obs_names], privileged="all"))
    cases = (("other settings", other, "sensor_fingerprint"), ("other batch", _noisy_vec(9), "num_envs"), ("no sensor", plain_vec(8), "obs_names"))
    for name, dst, word in cases:
        _drive(dst, 2)
        before = rc.vec_everything(dst), (None if dst.sensor is None else sc.sensor_blocks(dst.sensor))
        with pytest.raises(ValueError, match=word):
            dst.load_state_dict(sd)
        after = rc.vec_everything(dst), (None if dst.sensor is None else sc.sensor_blocks(dst.sensor))
        rc.assert_equal(after[0], before[0], name)
        if before[1] is not None:
            rc.assert_equal(after[1], before[1], name)
        dst.close()
    # the sensor's own refusal, reached directly
    s = _noisy_vec()
    try:
        bad = dict(s.sensor.state_dict(), fingerprint="0" * 16)
        with pytest.raises(ValueError, match="other channels"):
            s.sensor.load_state_dict(bad)
        with pytest.raises(ValueError, match="a sensor"):
            s.load_state_dict({k: v for k, v in s.state_dict().items() if k != "sensor"})
    finally:
        s.close()


def test_fork_carries_the_columns_and_keeps_the_destinations_calibration():
    vec = _noisy_vec(8)
    try:
        action, _ = _drive(vec, 4)
        before = sc.sensor_blocks(vec.sensor)
        vec.fork([0, 1], [5, 6])
        after = sc.sensor_blocks(vec.sensor)
        for name in ("sensor.out", "sensor.ring", "sensor.pos", "sensor.age"):
            a, b = after[name], before[name]
            assert torch.equal(a[..., 5], b[..., 0]) and torch.equal(a[..., 6], b[..., 1])
            keep = [0, 1, 2, 3, 4, 7]
            assert a[..., keep].numpy().tobytes() == b[..., keep].numpy().tobytes()
        obs = vec.step(action)[0]
        # the same state and history, the environment's own id: the clean copies agree, the calibrated readings do not
        names = vec.obs_names
        assert torch.equal(obs[5, names.index("priv.voltage")], obs[0, names.index("priv.voltage")])
        assert not torch.equal(obs[5, : vec.actor_obs_dim], obs[0, : vec.actor_obs_dim])
    finally:
        vec.close()


def test_a_masked_reset_keeps_the_other_environments_output():
    for norm in (None, Normalizer()):
        vec = _noisy_vec(8, normalizer=norm)
        try:
            _drive(vec, 3)
            before = sc.sensor_blocks(vec.sensor)
            mask = torch.tensor([True, False, False, True, False, False, False, False])
            obs, info = vec.reset(options={"mask": mask})
            after = sc.sensor_blocks(vec.sensor)
            rest = ~mask
            for name in ("sensor.out", "sensor.ring", "sensor.pos", "sensor.age"):
                assert after[name][..., rest].numpy().tobytes() == before[name][..., rest].numpy().tobytes(), name
            assert (after["sensor.age"][mask] == 0).all() and (after["sensor.pos"][mask] == 0).all() and (before["sensor.age"][mask] > 0).all()
            assert obs.shape == (8, len(vec.obs_names)) and info["raw_observation"].shape == (8, len(vec.raw_obs_names))
            if norm is None:
                assert torch.equal(obs, vec.sensor.out.t())
        finally:
            vec.close()


def test_first_is_who_began_an_episode_and_the_episode_number_is_the_adapters():
    """Against the definition driven by hand beside the adapter: ``first`` is ``_need_reset`` as it stood before the launch,
    ``episode`` the adapter's count after its own increment, ``t`` the number of calls."""
    vec = _noisy_vec(8)
    twin = sc.noisy_sensor(vec.raw_obs_names, seed=5)
    names, cols = twin._table(vec.raw_obs_names)
    L = 1 + max(c.max_delay for c in cols)
    chan = np.array([[c.sigma, c.gain_spread, c.offset_spread, c.lsb, c.lo, c.hi] for c in cols]).T.copy()
    route = np.array([[vec.raw_obs_names.index(c.source), c.max_delay] for c in cols], dtype=np.int32).T.copy()
    N = 8
    out, ring = np.zeros((len(cols), N), dtype=np.float32), np.zeros((L, len(vec.raw_obs_names), N), dtype=np.float32)
    pos, age = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    try:
        obs, info = vec.reset(seed=3)
        sensor_reference([info["raw_observation"].t().contiguous().numpy()], chan, route, None, None, vec.episode_count.numpy(), out, ring,
                         pos, age, seed=5, t=0, env_id_offset=vec.env.env_id_offset, num_envs=N, ring_len=L)
        assert obs.numpy().tobytes() == np.ascontiguousarray(out.T).tobytes()
        action = snap.scenario(vec.env, seed=3)
        restarts = 0
        for t in range(1, 7):
            began = vec._need_reset.clone()
            restarts += int(began.sum())
            obs, _, _, _, info = vec.step(action)
            sensor_reference([info["raw_observation"].t().contiguous().numpy()], chan, route, began.view(torch.uint8).numpy(), None,
                             vec.episode_count.numpy(), out, ring, pos, age, seed=5, t=t, env_id_offset=vec.env.env_id_offset,
                             num_envs=N, ring_len=L)
            assert obs.numpy().tobytes() == np.ascontiguousarray(out.T).tobytes(), t
        assert restarts > 0 and vec.sensor.t == 7
    finally:
        vec.close()


@pytest.mark.parametrize("variant", rc.VARIANTS)
def test_a_stack_with_a_sensor_resumes_byte_for_byte_at_every_cut(variant, tmp_path):
    """The stacks of tests/_resume_common.py with noise, calibration, delays of 0, 1 and 3 and ``privileged="all"``."""
    sc.check_resume_at_every_cut(variant, "cpu", tmp_path)


# ------------------------------------------------------------------------------------------------ PolicyNet on a wider store
def test_policy_net_reads_the_leading_columns_of_a_wider_store_in_place():
    env = snap.make("cpu", 6, "plain", "s13")
    head = PolicyHead(env, modes=rc.MODES, bounds=rc.BOUNDS, seed=1)
    D, wide, rows = 5, 13, 40
    rng = np.random.default_rng(8)
    store = torch.from_numpy(rng.standard_normal((rows, wide)).astype(np.float32))
    store[:, D:] = float("nan")   # (what the network must not read)
    narrow = store[:, :D].contiguous()
    gp = torch.from_numpy(rng.standard_normal((rows, head.param_dim)).astype(np.float32))
    gv = torch.from_numpy(rng.standard_normal(rows).astype(np.float32))
    results = []
    for obs in (store, narrow):
        net = PolicyNet(D, head, hidden=(16, 16), seed=3)
        fwd = [t.clone() for t in net.forward(obs)]
        params, value = net(obs)
        outs = [params.clone(), value.clone()]
        torch.autograd.backward((params, value), (gp, gv))
        results.append((*fwd, *outs, net.theta.grad.clone()))
    for a, b in zip(*results):
        assert a.detach().numpy().tobytes() == b.detach().numpy().tobytes() and bool(a.isfinite().all())

    class Roll:   # the one thing the network asks of a rollout
        def __init__(self, obs):
            self.obs = obs

        def flat(self):
            return {"obs": self.obs}

    idx = torch.from_numpy(rng.permutation(rows)[:17].astype(np.int64))
    grads = []
    for obs in (store, narrow):
        net = PolicyNet(D, head, hidden=(16, 16), seed=3)
        params, value = net(rollout=Roll(obs), index=idx)
        keep = (params.clone(), value.clone())
        torch.autograd.backward((params, value), (gp[:17], gv[:17]))
        grads.append((*keep, net.theta.grad.clone()))
    for a, b in zip(*grads):
        assert a.detach().numpy().tobytes() == b.detach().numpy().tobytes()
    with pytest.raises(ValueError, match="obs must be a float32 tensor"):
        PolicyNet(D, head, hidden=(16, 16)).forward(store[:, : D - 1])
    env.close()


def test_a_value_only_backward_reuses_its_cached_zero_gradient():
    env = snap.make("cpu", 6, "plain", "s13")
    head = PolicyHead(env, modes=rc.MODES, bounds=rc.BOUNDS, seed=1)
    net, twin = PolicyNet(7, head, hidden=(16, 16), seed=3), PolicyNet(7, head, hidden=(16, 16), seed=3)
    obs = torch.from_numpy(np.random.default_rng(2).standard_normal((30, 7)).astype(np.float32))
    gv = torch.linspace(-1.0, 1.0, 30)
    seen = []
    for _ in range(3):
        net.theta.grad = None
        _, value = net(obs)
        value.backward(gv)
        seen.append((net._zero_gp.data_ptr(), tuple(net._zero_gp.shape)))
    assert seen == [seen[0]] * 3 and seen[0][1] == (30, head.param_dim) and not bool(net._zero_gp.any())
    params, value = twin(obs)
    torch.autograd.backward((params, value), (torch.zeros_like(params), gv))
    assert net.theta.grad.numpy().tobytes() == twin.theta.grad.numpy().tobytes() and bool((net.theta.grad != 0).any())
    # a smaller call takes a view of the same buffer
    net.theta.grad = None
    net(obs[:11])[1].backward(gv[:11])
    assert net._zero_gp.data_ptr() == seen[0][0]
    env.close()
