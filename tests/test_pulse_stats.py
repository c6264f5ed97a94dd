"""Pulse statistics per control interval (include/wedm_hip.h, enum wedm_pulse_field): the reference driver's "Sparks" and
"Short pulses" (experiments/run_simulation.py:597-636) and the short-circuit steps, counted inside the kernels and
published at every control step.

CPU: the C-ABI mirror, the definition against the reference's own formula on its logger fixtures (F16), the oracle's
refusal.  GPU: the published counts against the fixtures, every kernel with a PULSE form against a per-step trace, resets,
frozen environments, the observation columns, checkpoints and the vector adapter's single launch."""
from __future__ import annotations

import json
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from sparc_amd import _abi, _lib

ROOT = Path(__file__).resolve().parents[1]
F16 = ("f16_logger_philox_env3", "f16_logger_velocity_philox_env1")
THRESHOLD = 0.1  # A (run_simulation.py:607)


# ---------------------------------------------------------------------------- the definition, in Python
def reference_counts(current, short):
    """run_simulation.py:604-627 over one window of logged samples: (sparks, short pulses)."""
    current, short = np.asarray(current), np.asarray(short, dtype=bool)
    short_above = (current > THRESHOLD) & short
    normal_above = (current > THRESHOLD) & ~short
    return int(np.sum(np.diff(short_above.astype(int)) > 0)), int(np.sum(np.diff(normal_above.astype(int)) > 0))


def tally(current, short, ctrl, ran=None, prev_current=0.0, prev_short=False):
    """The kernels' definition, sample by sample: returns the (spark, short, short_steps) counts published at every sample
    where `ctrl` is set, and the accumulators left after the last sample.  The sample before the first one is
    (`prev_current`, `prev_short`): after a reset current 0 and no short.  `ran`: False where the environment did not
    step (frozen: a trace still records its state, but that is no sample)."""
    def kind(i, s):
        return (2 if s else 1) if i > THRESHOLD else 0

    prev = kind(prev_current, prev_short)
    acc = [0, 0, 0]
    published = []
    ran = np.ones(len(current), dtype=bool) if ran is None else np.asarray(ran, dtype=bool)
    for i, s, c, r in zip(np.asarray(current), np.asarray(short, dtype=bool), np.asarray(ctrl, dtype=bool), ran):
        if not r:
            continue
        k = kind(float(i), bool(s))
        if k and k != prev:
            acc[k - 1] += 1
        if s:
            acc[2] += 1
        prev = k
        if c:
            published.append(tuple(acc))
            acc = [0, 0, 0]
    return published, tuple(acc)


def f16_signals(path):
    z = np.load(path, allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    return meta, z["every_step/time"], z["every_step/current"].astype(np.float64), z["every_step/is_short_circuit"]


# ---------------------------------------------------------------------------- CPU
def test_pulse_enum_in_the_header_matches_its_mirror(tmp_path):
    """enum wedm_pulse_field compiled as strict C99, against `_abi.PULSE` / `_abi.PULSE_COUNT`."""
    lines = ['#include <stdio.h>', '#include "wedm_hip.h"', "int main(void) {"]
    for f in _abi.PULSE:
        lines.append(f'  printf("{f.name} %d\\n", (int)WEDM_P_{f.name});')
    lines += ['  printf("COUNT %d\\n", (int)WEDM_PULSE_COUNT);', "  return 0;", "}"]
    src = tmp_path / "pulse.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "pulse"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                   check=True)
    out = dict(row.split() for row in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
               if row)
    assert {k: int(v) for k, v in out.items()} == {**{f.name: f.value for f in _abi.PULSE}, "COUNT": _abi.PULSE_COUNT}
    assert len(_abi.PULSE) == _abi.PULSE_COUNT == 6


def test_bind_pulse_stats_is_exported_and_listed():
    assert "wedm_bind_pulse_stats" in _lib.EXPORTS
    L = _lib.load()
    assert hasattr(L, "wedm_bind_pulse_stats")
    assert L.wedm_bind_pulse_stats(None, None) == _abi.ERR_BAD_ARG


@pytest.mark.parametrize("name", F16)
def test_python_tally_equals_the_reference_formula_on_its_logger_fixtures(golden_dir, name):
    """Per control interval, the definition sample by sample gives what the reference's `np.diff` formula gives over the
    driver's window (`time >= t - 1000`: the previous control step's sample and the interval's 1000), and the sum of
    the published counts is the formula over the whole run (with the reset state in front)."""
    meta, time, current, short = f16_signals(golden_dir / f"{name}.npz")
    assert np.array_equal(time, np.arange(1, len(time) + 1))  # every step of the run, dt = 1 us
    ctrl = (time - 1) % 1000 == 0
    ctrl[0] = False  # the first control step is step 1001 (time_since_servo reaches 1000 after 1000 steps)
    published, rest = tally(current, short, ctrl)
    ctrl_times = time[ctrl]
    assert len(published) == len(ctrl_times) >= 2
    for (sparks, shorts, steps), t in zip(published, ctrl_times):
        w = (time >= t - 1000) & (time <= t)
        if t - 1000 >= 1:
            assert w.sum() == 1001
            ref_short, ref_spark = reference_counts(current[w], short[w])
        else:  # the first interval: the reset state (current 0, no short) is the sample before the window
            ref_short, ref_spark = reference_counts(np.r_[0.0, current[w]], np.r_[False, short[w]])
        assert (sparks, shorts) == (ref_spark, ref_short), t
        assert steps == int(short[(time > t - 1000) & (time <= t)].sum())
    total_short, total_spark = reference_counts(np.r_[0.0, current], np.r_[False, short])
    assert sum(p[0] for p in published) + rest[0] == total_spark
    assert sum(p[1] for p in published) + rest[1] == total_short
    assert total_spark > 5  # the fixture does spark


def test_oracle_backend_refuses_pulse_stats():
    from sparc_amd import WireEDMEnv
    from tests._oracle_backend import OracleBackend

    with pytest.raises(ValueError, match="pulse_stats=True needs a backend"):
        WireEDMEnv(num_envs=4, device="cpu", pulse_stats=True, backend=OracleBackend)


# ---------------------------------------------------------------------------- GPU
def _close_gap(env, wp=25.0, x=10.0, target=5000.0):
    env.state.workpiece_position = wp
    env.state.wire_position = x
    env.state.target_position = target


def _make_env(n, *, pulse, geometry=None, **kw):
    from sparc_amd import EnvironmentConfig, WireEDMEnv, WireModuleParameters

    if geometry == "s128":
        kw.update(wire_params=WireModuleParameters(segment_len=0.625), config=EnvironmentConfig(target_cutting_distance=5000.0))
    elif geometry == "per_env":
        rng = np.random.default_rng(7)
        kw.update(workpiece_height=rng.uniform(10.0, 30.0, n), wire_diameter=rng.choice([0.10, 0.15, 0.20, 0.25, 0.30], n),
                  config=EnvironmentConfig(target_cutting_distance=5000.0))
    else:
        kw.update(config=EnvironmentConfig(target_cutting_distance=5000.0))
    return WireEDMEnv(num_envs=n, device="cuda:0", pulse_stats=pulse, **kw)


STEPS = 2600  # two control intervals and a part of the third


def _run(n, geometry, *, kernel=0, lanes=0, pulse=True, single=0, trace=False):
    """Seeded run with a gap that sparks and shorts: launches of one control interval (fused), or `single` launches of
    one microsecond at the end of the run."""
    env = _make_env(n, pulse=pulse, geometry=geometry)
    env.reset(seed=31)
    # gaps from a hard short (< 1 um) to an idle 15 um, the wire held where it is (servo 0): every kind of pulse
    _close_gap(env, torch.linspace(10.4, 25.0, n, dtype=torch.float64, device="cuda:0"), 10.0)
    env.set_kernel(kernel, lanes)
    tr = env.bind_trace(["current", "is_short_circuit", "control_step", "done"], every=1, capacity=STEPS) if trace else None
    a = env.make_action(0.0, 80.0, 9, 3.0, 30.0)
    fused = STEPS - single
    done = 0
    while done < fused:
        k = min(1000, fused - done)
        env.step_many(a, k)
        done += k
    fused_kernel = env._backend.last_kernel()
    for _ in range(single):
        env.step(a)
    torch.cuda.synchronize()
    return env, tr, fused_kernel


def _expected_from_trace(tr, n):
    d = tr.read_range(0, STEPS)
    cur, sh, ctrl = d["current"].cpu().numpy(), d["is_short_circuit"].cpu().numpy(), d["control_step"].cpu().numpy()
    done = d["done"].cpu().numpy()
    ran = np.ones_like(done)
    ran[1:] = ~done[:-1]  # a sample after one that found the environment terminated is no step it ran (frozen)
    rows = np.zeros((_abi.PULSE_COUNT, n), dtype=np.int32)
    for e in range(n):
        published, rest = tally(cur[:, e], sh[:, e], ctrl[:, e], ran[:, e])
        rows[0:3, e] = rest
        if published:
            rows[3:6, e] = published[-1]
    return rows


_KERNEL_NAMES = {1: "wedm_step_global", 2: "wedm_step_lanes_pk", 7: "wedm_step_regs<", 8: "wedm_step_regs_wide"}
SHAPES = {  # shape -> kernels with a PULSE form that take it (7: <= 128 segments; 8: uniform geometry)
    "s128": (4096, [(1, 0), (2, 0), (7, 0), (7, 1), (8, 0), (0, 0)]),
    "s400": (4096, [(1, 0), (2, 0), (8, 0), (8, 16), (0, 0)]),
    "per_env": (2048, [(1, 0), (2, 0), (2, 8), (0, 0)]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("geometry", list(SHAPES))
def test_every_kernel_counts_what_a_per_step_trace_counts(geometry):
    from tests._compare import assert_blocks_equal

    n, kernels = SHAPES[geometry]
    ref, tr, _ = _run(n, geometry, kernel=1, pulse=False, trace=True)
    want = _expected_from_trace(tr, n)
    assert want[3].sum() > n and want[4].sum() > 0 and want[5].sum() > 0, want[3:].sum(axis=1)
    base = ref.state.clone_blocks()
    for kernel, lanes in kernels:
        env, _, name = _run(n, geometry, kernel=kernel, lanes=lanes)
        assert "[pulse]" in name and (kernel == 0 or name.startswith(_KERNEL_NAMES[kernel])), (kernel, name)
        got = env.state.pulse[:, :n].cpu().numpy()
        assert np.array_equal(got, want), (kernel, lanes, env._backend.last_kernel(), np.argwhere(got != want)[:5])
        blocks = env.state.clone_blocks()
        keys = ("f64", "i32", "i8", "T", "stats", "reward")
        assert_blocks_equal({k: blocks[k] for k in keys}, {k: base[k] for k in keys}, n)  # (NaN == NaN)
        assert torch.equal(blocks["obs"][:8, :n], base["obs"][:, :n]), (kernel, lanes)
        assert torch.equal(blocks["obs"][8:, :n], torch.from_numpy(want[3:6].astype(np.float32))), (kernel, lanes)
        env.close()
    # launches with a trace sample (kernel 1's PULSE + TRACE form), and single microseconds at the end (kernel 1's PULSE form)
    for kw in (dict(trace=True), dict(single=300)):
        env, _, name = _run(n, geometry, **kw)
        assert env._backend.last_kernel().startswith("wedm_step_global[pulse]"), (kw, env._backend.last_kernel())
        assert np.array_equal(env.state.pulse[:, :n].cpu().numpy(), want), kw
        assert_blocks_equal({"T": env.state.clone_blocks()["T"]}, {"T": base["T"]}, n)
        env.close()


@pytest.mark.gpu
def test_forced_kernel_without_pulse_form_is_refused():
    from sparc_amd._lib import WedmError

    env = _make_env(256, pulse=True, geometry="s128")
    env.reset(seed=1)
    for kernel in (3, 4, 5, 6, 9, 10, 11, 12):
        env.set_kernel(kernel, 0)
        with pytest.raises(WedmError, match="WEDM_ERR_UNSUPPORTED"):
            env.step_many(env.make_action(), 10)
    env.set_kernel(0, 0)
    env.step_many(env.make_action(), 10)
    assert "[pulse]" in env._backend.last_kernel()


@pytest.mark.gpu
@pytest.mark.parametrize("name", F16)
def test_published_counts_follow_the_reference_logger_fixtures(golden_dir, name):
    """The F16 runs (the reference's own driver and logger) replayed in fused launches: at every control step the
    published counts equal the reference formula applied to the fixture's signals, as exact integers."""
    from sparc_amd import GapController, WireEDMEnv, WireModuleParameters, run_controlled

    meta, time, current, short = f16_signals(golden_dir / f"{name}.npz")
    e = int(meta["env_id"])
    env = WireEDMEnv(num_envs=e + 3, device="cuda:0", mechanics_control_mode=meta["control_mode"],
                     wire_params=WireModuleParameters(**meta["modules"]["wire"]), pulse_stats=True)
    env.reset(seed=int(meta["seed"]))
    for k, v in meta["state_init"].items():
        setattr(env.state, k, v)
    seen = []

    def on_control_step(env_, done):
        st = env_.get_pulse_statistics()
        seen.append((done, int(st["spark_pulses"][e]), int(st["short_pulses"][e]), int(st["short_steps"][e])))

    run_controlled(env, GapController(), int(meta["n_steps_run"]), on_control_step=on_control_step)
    assert len(seen) >= 2
    for t, sparks, shorts, steps in seen:
        w = (time >= t - 1000) & (time <= t)
        cur, sh = (current[w], short[w]) if t - 1000 >= 1 else (np.r_[0.0, current[w]], np.r_[False, short[w]])
        ref_short, ref_spark = reference_counts(cur, sh)
        assert (sparks, shorts, steps) == (ref_spark, ref_short, int(short[(time > t - 1000) & (time <= t)].sum())), t
    assert sum(s[1] for s in seen) > 5


@pytest.mark.gpu
def test_resets_frozen_environments_observation_and_checkpoint(tmp_path):
    n = 4096
    env, _, _ = _run(n, "s128")
    P = _abi.PULSE
    rows = env.state.pulse[:, :n]
    assert int(rows[P.SPARK_LAST].sum()) > 0 and int(rows[P.SPARK_ACC].sum()) > 0
    # observation columns 8-10 = the published rows; the widened space and names
    obs = env._get_obs()
    assert obs.shape == (n, 11) and env.observation_space.shape == (11,)
    assert env.obs_names[8:] == ("spark_pulses", "short_pulses", "short_steps") and len(_abi.OBS_NAMES) == 8
    assert torch.equal(obs[:, 8:], rows[P.SPARK_LAST:].t().to(torch.float32))
    stats = env.get_pulse_statistics()
    assert torch.equal(stats["short_pulses"], rows[P.SHORT_LAST]) and stats["spark_pulses"].dtype == torch.int32
    # checkpoint round trip reproduces the rows and the continuation
    sd = env.state_dict()
    other = _make_env(n, pulse=True, geometry="s128")
    other.load_state_dict(sd)
    assert torch.equal(other.state.pulse, env.state.pulse)
    for x in (env, other):
        x.step_many(x.make_action(0.0, 80.0, 9, 3.0, 30.0), 1000)
    assert torch.equal(other.state.pulse, env.state.pulse) and torch.equal(other.state.obs, env.state.obs)
    with pytest.raises(ValueError, match="pulse_stats"):
        _make_env(n, pulse=False, geometry="s128").load_state_dict(sd)
    # a masked reset clears exactly the masked environments' rows
    mask = torch.zeros(n, dtype=torch.bool, device="cuda:0")
    mask[::3] = True
    before = env.state.pulse[:, :n].clone()
    env.reset(options={"mask": mask})
    after = env.state.pulse[:, :n]
    assert int(after[:, mask].abs().sum()) == 0 and torch.equal(after[:, ~mask], before[:, ~mask])
    assert int(env._get_obs()[mask][:, 8:].abs().sum()) == 0
    # frozen environments keep their last published counts: terminate some that have counts, step on
    fz = torch.zeros(n, dtype=torch.bool, device="cuda:0")
    fz[1::3] = True
    assert int(env.state.pulse[P.SPARK_LAST, :n][fz].sum()) > 0
    env.state.done = fz
    env.state.is_target_distance_reached = fz
    frozen = env.state.pulse[:, :n][:, fz].clone()
    env.step_many(env.make_action(0.0, 80.0, 9, 3.0, 30.0), 1000)
    torch.cuda.synchronize()
    assert torch.equal(env.state.pulse[:, :n][:, fz], frozen)
    live = ~mask & ~fz  # (the reset ones have not reached their first control step yet: 1000 steps since the reset)
    assert int(env.state.pulse[P.SPARK_LAST, :n][live].sum()) > 0 and not torch.equal(env.state.pulse[:, :n][:, live], before[:, live])


@pytest.mark.gpu
def test_autoreset_clears_the_rows_and_the_vector_env_step_stays_one_launch_without_host_sync():
    from sparc_amd import WireEDMVectorEnv

    n = 4096
    env = _make_env(n, pulse=True, geometry="s128", autoreset=True)
    vec = WireEDMVectorEnv(env, max_episode_steps=3000)
    vec.reset(seed=5)
    _close_gap(env, torch.linspace(10.4, 25.0, n, dtype=torch.float64, device="cuda:0"), 10.0)
    act = env.make_action(0.0, 80.0, 9, 3.0, 30.0)
    vec.step(act)
    vec.step(act)
    torch.cuda.synchronize()
    assert int(env.state.pulse[_abi.PULSE.SPARK_LAST, :n].sum()) > 0
    # the in-launch autoreset: terminated environments start the next launch with cleared rows
    done = torch.zeros(n, dtype=torch.bool, device="cuda:0")
    done[1::2] = True
    env.state.done = done
    env.state.is_target_distance_reached = done
    env.step_many(act, 1)   # one microsecond: the reset environments have no control step in it
    torch.cuda.synchronize()
    rows = env.state.pulse[:, :n]
    assert int(rows[_abi.PULSE.SPARK_LAST:, done].abs().sum()) == 0 and int(env.state.episode[done].min()) >= 1
    assert int(rows[_abi.PULSE.SPARK_LAST, ~done].sum()) > 0
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            obs, reward, term, trunc, info = vec.step(act)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert obs.shape == (n, 11) and "[pulse]" in env._backend.last_kernel()
