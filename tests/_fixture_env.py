"""Compare a batched environment against a reference fixture (tests/golden) environment by
environment.  Shared by the CPU (oracle backend) and GPU tests."""
from __future__ import annotations

import math

import numpy as np

INT_MAP = {
    "time": "time", "time_since_servo": "time_since_servo", "spark_state": "spark_state", "spark_dur": "spark_duration",
    "is_short_circuit": "is_short_circuit", "random_short_remaining": "random_short_remaining",
    "debris_short_remaining": "debris_short_remaining", "time_in_critical_temp": "time_in_critical_temp",
    "is_wire_broken": "is_wire_broken", "is_target_reached": "is_target_distance_reached",
    "ctrl_step": "control_step", "time_since_spark_ignition": "time_since_spark_ignition",
    "time_since_spark_end": "time_since_spark_end", "time_since_open_voltage": "time_since_open_voltage",
}
FLOAT_MAP = {
    "workpiece_position": "workpiece_position", "wire_position": "wire_position", "wire_velocity": "wire_velocity",
    "voltage": "voltage", "current": "current", "spark_y": "spark_location", "debris_volume": "debris_volume",
    "debris_density": "debris_density", "flow_rate": "flow_rate", "cavity_volume": "cavity_volume",
    "last_crater_volume": "last_crater_volume", "prev_accel": "prev_accel", "tmax": "wire_max_temperature",
    "h_base": "h_eff_base", "h_zone": "h_eff_zone", "diel_last_gap": "dielectric_last_gap",
    "diel_last_density": "dielectric_last_density", "wire_last_flow": "wire_last_flow",
}
EXACT_ALWAYS = ("workpiece_position", "wire_position", "wire_velocity", "voltage", "current", "spark_y", "prev_accel")


def check_step(env, fx, env_index, step, *, exact_floats, float_rtol=1e-12, tmax_atol=1e-4):
    """Assert that environment `env_index` equals the fixture at `step` (after that step)."""
    st = env.state
    for name, attr in INT_MAP.items():
        if name == "ctrl_step" and int(fx.int_row("is_wire_broken")[step]):
            continue  # the reference's early return (wire_edm.py:129-130) carries no control_step key
        want = int(fx.int_row(name)[step])
        got = int(getattr(st, attr)[env_index].item())
        assert want == got, f"step {step} env {env_index} {name}: reference {want} got {got}"
    pos = np.searchsorted(fx.float_steps, step)
    if pos < len(fx.float_steps) and fx.float_steps[pos] == step:
        for name, attr in FLOAT_MAP.items():
            want = float(fx.float_row(name)[pos])
            got = float(getattr(st, attr)[env_index].item())
            same = (want == got) or (math.isnan(want) and math.isnan(got))
            if exact_floats or name in EXACT_ALWAYS:
                assert same, f"step {step} env {env_index} {name}: reference {want!r} got {got!r}"
            elif name in ("tmax",):
                assert same or abs(want - got) <= tmax_atol, f"step {step} {name}: {want!r} vs {got!r}"
            else:
                assert same or abs(want - got) <= float_rtol * max(abs(want), abs(got)), \
                    f"step {step} env {env_index} {name}: reference {want!r} got {got!r}"


# ------------------------------------------------------------------ whole-trajectory comparison
# A Philox fixture replayed on the BATCHED environment: the environment whose global id equals the
# fixture's env_id must follow the reference microsecond by microsecond.  The trajectory is read
# from the device trace, so the run itself uses fused launches (one per control interval).
TRACE_INT = {"time": "time", "spark_state": "spark_state", "spark_dur": "spark_duration",
             "is_short_circuit": "is_short_circuit", "random_short_remaining": "random_short_remaining",
             "debris_short_remaining": "debris_short_remaining", "time_in_critical_temp": "time_in_critical_temp",
             "is_wire_broken": "is_wire_broken", "is_target_reached": "is_target_distance_reached",
             "time_since_servo": "time_since_servo"}
TRACE_EXACT = {"workpiece_position": "workpiece_position", "wire_position": "wire_position",
               "wire_velocity": "wire_velocity", "voltage": "voltage", "current": "current", "spark_y": "spark_location",
               "prev_accel": "prev_accel"}
TRACE_CLOSE = {"debris_volume": "debris_volume", "debris_density": "debris_density", "flow_rate": "flow_rate",
               "cavity_volume": "cavity_volume", "last_crater_volume": "last_crater_volume"}


def env_from_fixture(fx, n, *, device, backend=None, **extra):
    """A batched environment configured like the fixture's reference run (constant-action scenarios)."""
    from sparc_amd import (DielectricModuleParameters, EnvironmentConfig, IgnitionModuleParameters,
                           MaterialModuleParameters, MechanicsModuleParameters, WireEDMEnv, WireModuleParameters)

    m = fx.meta
    mods = m["modules"]
    kw = dict(backend=backend) if backend is not None else {}
    kw.update(extra)
    material = m["config"].get("wire_material", "brass")
    if material != "brass":  # register the fixture's custom material the way a user would
        from sparc_amd import WireMaterial, get_material_db

        get_material_db()._wire_materials[material] = WireMaterial(name=material, **m["wire_material_constants"])
    env = WireEDMEnv(num_envs=n, device=device, mechanics_control_mode=m["control_mode"],
                     config=EnvironmentConfig(**m["config"]),
                     ignition_params=IgnitionModuleParameters(**mods["ignition"]),
                     wire_params=WireModuleParameters(**mods["wire"]),
                     material_params=MaterialModuleParameters(**mods["material"]),
                     dielectric_params=DielectricModuleParameters(**mods["dielectric"]),
                     mechanics_params=MechanicsModuleParameters(**mods["mechanics"]), **kw)
    env.reset(seed=int(m["seed"]))
    for k, v in m["state_init"].items():
        setattr(env.state, k, v)
    for k, v in m["module_init"].items():
        assert k == "dielectric.debris_volume"
        env.state.debris_volume = v
    for lo, hi, val in m.get("T_init", []):
        T = env.state.wire_temperature
        T[:, lo:hi] = val
    return env


def compat_env_from_fixture(fx, n, *, device, backend=None, **extra):
    """The reference-compatible modes the F17 / F18 fixtures need: `reset()` re-initialises EDMState only
    (fixtures with a second episode), `step()` goes on after `terminated` (fixtures that were stepped past it)."""
    kw = dict(extra)
    if fx.meta.get("resets"):
        kw["reset_semantics"] = "reference"
    if fx.meta.get("stop_on_terminate") is False:
        kw["freeze_terminated"] = False
    return env_from_fixture(fx, n, device=device, backend=backend, **kw)


def fixture_segments(fx):
    """[(first step, last step + 1, reset before it: (seed, state_init) or None)] of a fixture with second episodes."""
    cuts = sorted((int(at), int(sd), si) for at, sd, si in fx.meta.get("resets", []))
    out, lo, pending = [], 0, None
    for at, sd, si in cuts:
        out.append((lo, at, pending))
        lo, pending = at, (sd, si)
    out.append((lo, fx.n_steps, pending))
    return out


def apply_fixture_reset(env, reset):
    seed, init = reset
    env.reset(seed=seed)  # reset_semantics="reference": EDMState only
    for k, v in init.items():
        setattr(env.state, k, v)


def run_fixture_stepwise(env, fx, *, exact_floats, every=1):
    """One `step()` per microsecond, every recorded quantity of environment `env_id` compared after each step
    (`every`: after every that-many steps), second episodes and steps past `terminated` included."""
    e = int(fx.meta["env_id"])
    assert len(fx.actions) == 1, "constant-action fixtures only"
    servo, tv, on, off, mode = fx.actions[0]
    act = env.make_action(servo, tv, int(mode), on, off)
    checked = 0
    for lo, hi, reset in fixture_segments(fx):
        if reset is not None:
            apply_fixture_reset(env, reset)
        for step in range(lo, hi):
            env.step(act)
            if step % every == 0 or step in (lo, hi - 1):
                check_step(env, fx, e, step, exact_floats=exact_floats)
                if env.freeze_terminated is False:
                    assert int(env.state.done[e]) == int(fx.int_row("terminated")[step]), f"step {step}: terminated"
                checked += 1
    return checked


def fixture_launches(fx, lo, hi, interval):
    """[(row of fx.actions, steps)] covering steps lo ... hi - 1: launches of at most `interval` steps that never span a
    step at which the reference's driver handed `step()` another action (a constant-action fixture: chunks of `interval`)."""
    out, pos = [], lo
    while pos < hi:
        row = int(fx.action_idx[pos])
        end = pos + 1
        while end < hi and end - pos < interval and int(fx.action_idx[end]) == row:
            end += 1
        out.append((row, end - pos))
        pos = end
    return out


def run_fixture_through_trace(env, fx, *, exact_floats, float_rtol=1e-12, T_atol=1e-4, extra=(), run=None):
    """Run the fixture's recorded actions for its whole length in fused launches and compare the
    traced trajectory of environment `env_id` with the reference's recording.  `extra`: further EDMState names to
    trace and return (not compared here).  `run`: a driver `run(env)` that advances the environment by the fixture's
    steps itself (a controller under `run_controlled`) in place of the recorded actions."""
    import torch

    e = int(fx.meta["env_id"])
    names = sorted(set(TRACE_INT.values()) | set(TRACE_EXACT.values()) | set(TRACE_CLOSE.values()) | set(extra))
    keep_stepping = getattr(env, "freeze_terminated", True) is False
    if keep_stepping:
        names = sorted(set(names) | {"done"})
    trace = env.bind_trace(names, every=1, capacity=fx.n_steps, envs=(e, 1))
    # physics steps between two latches: the latch tests `time_since_servo >= servo_interval`, so an interval that is no
    # multiple of dt takes ceil(servo_interval / dt) steps (100 us at dt = 3: 34, not 33)
    interval = -(-env.servo_interval // env.dt)
    for lo, hi, reset in fixture_segments(fx):   # (one segment unless the fixture holds a second episode)
        if reset is not None:
            apply_fixture_reset(env, reset)
        if run is not None:
            assert (lo, hi) == (0, fx.n_steps), "a driver runs a fixture of one episode"
            run(env)
            continue
        acts = {}
        for row, k in fixture_launches(fx, lo, hi, interval):
            if row not in acts:
                servo, tv, on, off, mode = fx.actions[row]
                acts[row] = env.make_action(servo, tv, int(mode), on, off)
            env.step_many(acts[row], k)
    got = {k: v[:, 0].cpu().numpy() for k, v in trace.read().items()}
    if keep_stepping:  # WEDM_B_DONE = `terminated` as the reference's step() returns it, at every microsecond
        assert np.array_equal(got["done"].astype(np.int64), fx.int_row("terminated").astype(np.int64)), "terminated"
    for ref, name in TRACE_INT.items():
        want = fx.int_row(ref)
        assert np.array_equal(got[name].astype(np.int64), want.astype(np.int64)), \
            f"{ref}: first difference at step {int(np.nonzero(got[name].astype(np.int64) != want)[0][0])}"
    fs = fx.float_steps
    for ref, name in TRACE_EXACT.items():
        want, have = fx.float_row(ref), got[name][fs]
        same = (want == have) | (np.isnan(want) & np.isnan(have))
        assert same.all(), f"{ref}: step {int(fs[np.nonzero(~same)[0][0]])}"
    for ref, name in TRACE_CLOSE.items():
        want, have = fx.float_row(ref), got[name][fs]
        if exact_floats:
            assert np.array_equal(want, have), ref
        else:
            assert np.all(np.abs(want - have) <= float_rtol * np.maximum(np.abs(want), np.abs(have))), ref
    T = env.state.wire_temperature[e].cpu().numpy()[: fx.T_snaps.shape[1]]
    if exact_floats:
        assert np.array_equal(T, fx.T_snaps[-1])
    else:
        assert np.abs(T.astype(np.float64) - fx.T_snaps[-1]).max() <= T_atol
    if "crater_stats" in fx.data:
        stats = {k: v[e].item() for k, v in env.get_crater_statistics().items()}
        total, mean, std, vmin, vmax = fx.data["crater_stats"].tolist()
        assert stats["total_craters"] == total
        if total:
            assert (stats["min_volume_um3"], stats["max_volume_um3"]) == (vmin, vmax)
            assert abs(stats["mean_volume_um3"] - mean) <= 1e-12 * mean
    env.unbind_trace()
    return got


# ------------------------------------------------------------------ the reference's own logger (fixture F16)
LOGGER_EXACT = ("time", "voltage", "current", "wire_position", "wire_velocity", "workpiece_position", "target_delta",
                "is_short_circuit")


def run_logger_fixture(path, *, device, backend=None, exact):
    """Fixture F16 = the output of the reference's `SimulationLogger` (utils/logger.py:54-237) fed by its own
    driver loop (experiments/run_simulation.py:241-297) over its own signal list, at the three log
    frequencies.  Runs the build's logger + `run_controlled` + on-device gap controller the same way and
    compares key by key.  `exact`: every float bit for bit (LIBM oracle seam); otherwise positions,
    voltages, currents and commands exact, debris / flow to 1e-12, temperatures to 1e-4 K (GPU)."""
    import json

    from sparc_amd import GapController, SimulationLogger, WireEDMEnv, WireModuleParameters, run_controlled

    z = np.load(path, allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    e, n_steps = int(meta["env_id"]), int(meta["n_steps_run"])
    kw = dict(backend=backend) if backend is not None else {}
    compared = 0
    for freq in ("every_step", "interval", "control_step"):
        signals = meta["every_step_signals"] if freq == "every_step" else meta["signals"]
        env = WireEDMEnv(num_envs=e + 3, device=device, mechanics_control_mode=meta["control_mode"],
                         wire_params=WireModuleParameters(**meta["modules"]["wire"]), **kw)
        env.reset(seed=int(meta["seed"]))
        for k, v in meta["state_init"].items():
            setattr(env.state, k, v)
        lf = {"type": freq, "value": int(meta["interval"])} if freq == "interval" else {"type": freq}
        lg = SimulationLogger({"signals_to_log": signals, "log_frequency": lf, "backend": {"type": "memory"}},
                              env_reference=env)
        lg.attach(env)
        run_controlled(env, GapController(), n_steps, logger=lg)
        data = lg.get_data()
        assert sorted(data) == sorted(signals)
        for sig in signals:
            want, got = z[f"{freq}/{sig}"], data[sig][:, e]
            assert got.shape == want.shape, (freq, sig, got.shape, want.shape)
            if want.dtype.kind in "bi" or exact or sig in LOGGER_EXACT:
                same = (got == want) | ((got != got) & (want != want))
                assert same.all(), f"{freq}/{sig}: first difference at sample {int(np.nonzero(~same.reshape(len(same), -1).all(axis=1))[0][0])}"
            elif sig in ("wire_temperature", "wire_average_temperature"):
                assert np.abs(got.astype(np.float64) - want).max() <= 1e-4, f"{freq}/{sig}"
            else:
                assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(np.abs(got), np.abs(want))), f"{freq}/{sig}"
            compared += 1
        env.close()
    return compared
