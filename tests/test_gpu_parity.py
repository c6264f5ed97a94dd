"""Parity of the HIP path (through the C-ABI) with the CPU oracle, on a real MI355X.

Every comparison is BIT-EXACT over all state blocks (float64 scalars, int32/int8
state, float32 wire temperatures, observations): the kernels evaluate the same IEEE
expression trees as the oracle's PORTABLE math mode, which tests/test_oracle_golden.py
ties to the reference (exact decisions, <=1e-12 relative on float64 state, <=1e-4 K)."""
from __future__ import annotations

import ctypes as C
import json

import os

import numpy as np
import pytest
import torch

from sparc_amd import (EnvironmentConfig, IgnitionModuleParameters, MechanicsModuleParameters, WireEDMEnv,
                       WireModuleParameters)
from tests._compare import assert_blocks_equal, block_diffs
from tests._oracle_backend import OracleBackend

pytestmark = pytest.mark.gpu


def make_pair(n, **kw):
    gpu = WireEDMEnv(num_envs=n, device="cuda:0", **kw)
    cpu = WireEDMEnv(num_envs=n, device="cpu", backend=OracleBackend, **kw)
    return gpu, cpu


def both(envs, fn):
    for e in envs:
        fn(e)


def check(gpu, cpu, n):
    torch.cuda.synchronize()
    assert_blocks_equal(gpu.state.clone_blocks(), cpu.state.clone_blocks(), n)


def close_gap(env, wp=25.0, x=10.0, target=5000.0):
    env.state.workpiece_position = wp
    env.state.wire_position = x
    env.state.target_position = target


def test_native_library_is_the_one_running():
    env = WireEDMEnv(num_envs=64, device="cuda:0")
    assert env._backend.name == "hip"
    env.reset(seed=1)
    env.step(env.make_action())
    assert "wedm_step_stream" in env._backend.last_kernel() or "wedm_step_split" in env._backend.last_kernel()
    env.step_many(env.make_action(), 10)
    assert any(k in env._backend.last_kernel() for k in ("wedm_step_packed", "wedm_step_fused", "wedm_step_regs_wide"))
    env.set_kernel(2)
    env.step_many(env.make_action(), 10)
    assert "wedm_step_lanes" in env._backend.last_kernel()


@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4, 5, 6, 7, 8])
def test_device_math_primitives_match_cpu_bit_for_bit(orc, kind):
    """exp/log/cube are IEEE-basic-op expression trees; sqrt, division and fmod-based
    floor division must be correctly rounded on the device; Philox must match."""
    from sparc_amd import _lib

    L = _lib.load()
    rng = np.random.default_rng(kind)
    n = 1 << 16
    if kind == 0:
        a = rng.uniform(-600, 600, n); b = np.zeros(n)
    elif kind == 1:
        a = np.concatenate([rng.uniform(0, 1, n // 2), 2.0 ** rng.uniform(-104, 0, n // 2)]); b = np.zeros(n)
    elif kind == 2:
        a = rng.uniform(0, 8, n); b = np.zeros(n)
    elif kind == 3:
        a = np.concatenate([rng.uniform(0, 4, n // 2), 10.0 ** rng.uniform(-30, 30, n // 2)]); b = np.zeros(n)
    elif kind == 4:
        a = rng.uniform(0, 40, n); b = rng.choice([0.1, 0.2, 0.25, 0.3, 0.5, 0.625, 1.0], n)
        a[:64] = np.arange(64) * 0.2  # exact-multiple edge cases
        b[:64] = 0.2
    elif kind == 5:
        a = rng.uniform(-1e3, 1e3, n); b = rng.uniform(1e-3, 1e3, n)
    elif kind == 8:
        # the spark's cell: y in [0, h] over segment lengths, plus the cases a rounded division gets wrong (products
        # of an integer and the segment length nudged by one unit in the last place either way), negatives and NaN
        b = rng.choice([0.1, 0.2, 0.25, 0.3, 0.5, 0.625, 1.0, 0.7, 1e-3, 3.3], n)
        a = rng.uniform(0, 60, n)
        m = rng.integers(0, 5000, n // 2).astype(np.float64) * b[: n // 2]
        a[: n // 2] = np.nextafter(m, rng.choice([-np.inf, np.inf, 0.0], n // 2) * np.ones(n // 2))
        a[n // 2: n // 2 + 64] = -rng.uniform(0, 40, 64)
        a[n // 2 + 64] = np.nan
        a[n // 2 + 65] = 0.0
        a[n // 2 + 66] = 1e300
    else:
        a = rng.integers(0, 2**31, n).astype(np.float64); b = rng.integers(0, 2**31, n).astype(np.float64)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    assert L.wedm_debug_math(kind, ta.data_ptr(), tb.data_ptr(), out.data_ptr(), n, None) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    o = orc.lib()
    if kind == 0:
        want = np.array([o.wedm_oracle_exp(x, orc.MATH_PORTABLE) for x in a])
    elif kind == 1:
        want = np.array([o.wedm_oracle_log(x, orc.MATH_PORTABLE) for x in a])
    elif kind == 2:
        want = np.array([o.wedm_oracle_cube(x, orc.MATH_PORTABLE) for x in a])
    elif kind == 3:
        want = np.sqrt(a)
    elif kind == 4:
        want = np.array([o.wedm_oracle_py_floordiv(x, y) for x, y in zip(a, b)])
        assert np.array_equal(want, np.array([x // y for x, y in zip(a.tolist(), b.tolist())]))
    elif kind == 5:
        want = a / b
    elif kind == 8:
        # int(y // seg) by CPython's own float floor division (NaN and 1e300 do not convert: the kernel's int
        # conversion saturates there, and such a y never reaches it: the caller tests y == y and the range)
        ok = np.isfinite(a) & (np.abs(a) < 1e12)
        want = np.array([float(int(x // y)) if k else 0.0 for x, y, k in zip(a.tolist(), b.tolist(), ok)])
        got = np.where(ok, got, 0.0)
    elif kind == 6:
        want = np.array([(lambda u: u[0] + 2.0 * u[1] + 4.0 * u[2] + 8.0 * u[3])(
            orc.step_uniforms(0x9abcdef012345678, int(y), 3, int(x))) for x, y in zip(a[:4096], b[:4096])])
        got = got[:4096]
    else:
        want = np.array([orc.std_normal(0x9abcdef012345678, int(y), 3, int(x))[0] for x, y in zip(a[:4096], b[:4096])])
        got = got[:4096]
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), \
        f"kind {kind}: {np.count_nonzero(got.view(np.uint64) != want.view(np.uint64))} of {len(want)} differ"


KERNELS = [(1, 0), (5, 0), (6, 0), (6, 4), (6, 16), (2, 0), (3, 1), (3, 2), (3, 4), (3, 8), (3, 16), (4, 1), (4, 2), (4, 4), (4, 8),
           (10, 0), (2, 4), (2, 16)]   # (2: the packed any-geometry kernel; 10: its cell-by-cell form)
# the served kernels (wedm_served.h: the scalar physics of a block's environments on a wave of its own, one step ahead)
SERVED = [(9, 4), (9, 8)]
SERVED_ANY = [(11, 4), (11, 8), (11, 16)]   # the served form of the any-geometry kernel


@pytest.mark.parametrize("variant,lanes", KERNELS + SERVED + SERVED_ANY)
def test_default_config_fused_matches_oracle(variant, lanes):
    """BASELINE config 2 shape (S=400): 3 control intervals, every kernel variant."""
    n = 320
    gpu, cpu = make_pair(n)
    gpu.set_kernel(variant, lanes)
    both((gpu, cpu), lambda e: (e.reset(seed=1234), close_gap(e)))
    too_big = (variant == 3 and (-(-gpu.n_segments // lanes) + 1) > 160) or \
              (variant == 4 and (2 * -(-gpu.n_segments // (2 * lanes)) + 2) > 160)
    if too_big:
        from sparc_amd._lib import WedmError

        with pytest.raises(WedmError, match="WEDM_ERR_UNSUPPORTED"):  # chunk does not fit in 160 KB of LDS
            gpu.step_many(gpu.make_action(), 10)
        return
    for env in (gpu, cpu):
        a = env.make_action(0.1, 80.0, 5, 3.0, 80.0)
        for _ in range(3):
            env.step_many(a, 1000)
    check(gpu, cpu, n)
    assert int(gpu.state.spark_count.sum()) > 100


def test_single_microsecond_steps_with_changing_actions():
    """The reference's own call pattern: one step() per microsecond, action latched
    only at control steps (wire_edm.py:117-121)."""
    n = 100  # not a multiple of 64
    gpu, cpu = make_pair(n)
    both((gpu, cpu), lambda e: (e.reset(seed=5), close_gap(e, 22.0, 10.0)))
    rng = np.random.default_rng(0)
    modes = rng.choice([1, 3, 5, 7, 9, 11, 13, 15, 17], size=(3, n)).astype(np.int32)
    servo = rng.uniform(-0.5, 0.5, size=(3, n))
    for step in range(2300):
        k = step // 900
        act = {"servo": servo[k], "generator_control": {
            "target_voltage": np.float32(60 + 20 * k), "current_mode": modes[k],
            "ON_time": np.array([2.5]), "OFF_time": np.array([10.0 + 15 * k])}}
        og, rg, tg, ug, ig = gpu.step(act)
        oc, rc, tc, uc, ic = cpu.step(act)
    check(gpu, cpu, n)
    assert torch.equal(ig["control_step"].cpu(), ic["control_step"])
    assert torch.equal(tg.cpu(), tc)


@pytest.mark.parametrize("variant,lanes", KERNELS + [(7, 0), (12, 0)] + SERVED)
def test_config3_grid_128_segments(variant, lanes):
    """BASELINE config 3: segment_len 0.625 -> 128 segments."""
    n = 1024
    kw = dict(wire_params=WireModuleParameters(segment_len=0.625))
    gpu, cpu = make_pair(n, **kw)
    gpu.set_kernel(variant, lanes)
    assert gpu.n_segments == 128
    both((gpu, cpu), lambda e: (e.reset(seed=99), close_gap(e, 22.0, 10.0)))
    for env in (gpu, cpu):
        a = env.make_action(0.05, 100.0, 9, 2.0, 20.0)
        env.step_many(a, 1)
        env.step_many(a, 2499)
    check(gpu, cpu, n)


@pytest.mark.parametrize("variant,lanes", [(3, 4), (3, 8), (3, 16), (4, 4), (4, 8), (6, 4), (6, 8), (2, 8), (9, 4), (9, 8), (11, 8)])
def test_fused_kernel_with_ragged_chunks_and_heavy_sparking(variant, lanes):
    """361 segments (not divisible by any lane count), thin wire + I17: Joule heating,
    plasma cells at chunk edges, wire breaks and frozen environments inside live waves."""
    n = 200
    kw = dict(config=EnvironmentConfig(workpiece_height=12.3, wire_diameter=0.15, target_cutting_distance=5000.0))
    gpu, cpu = make_pair(n, **kw)
    assert gpu.n_segments == 361
    gpu.set_kernel(variant, lanes)
    both((gpu, cpu), lambda e: (e.reset(seed=17), close_gap(e, 24.0, 10.0)))
    for env in (gpu, cpu):
        a = env.make_action(0.1, 80.0, 17, 3.0, 40.0)
        env.step_many(a, 1)
        env.step_many(a, 1799)
        env.state.wire_unwinding_velocity[::7] = 0.0   # mixed advection inside a wave
        env.step_many(a, 700)
    check(gpu, cpu, n)
    want = {3: f"wedm_step_fused<{lanes}>", 4: f"wedm_step_packed<{lanes}>", 6: f"wedm_step_stream<{lanes}>",
            2: f"wedm_step_lanes_pk<{lanes}>", 9: f"wedm_step_served<{lanes}>", 11: f"wedm_step_lanes_"}[variant]
    assert want in gpu._backend.last_kernel()
    assert bool(gpu.state.is_wire_broken.any()) and not bool(gpu.state.is_wire_broken.all())


@pytest.mark.parametrize("variant,lanes", [(4, 2), (3, 4), (6, 4), (2, 4), (1, 0)])
def test_last_cell_closing_a_full_tile_that_a_partial_tile_follows(variant, lanes):
    """169 segments in chunks of 43 cells: the wire's last cell (168 = 129 + 39) closes the fifth full tile of the last
    chunk, and a sixth tile of three cells past the wire's end follows.  The regular-tile code must keep that cell out
    of the maximum although it is not in the chunk's last tile (it once did not: the value computed from a never-staged
    LDS row broke wires at t = 3 us whenever the previous kernel had left something implausible there; the GPU tests
    poison the LDS for that reason)."""
    n = 160
    kw = dict(config=EnvironmentConfig(workpiece_height=24.5, target_cutting_distance=5000.0),
              wire_params=WireModuleParameters(segment_len=0.5))
    gpu, cpu = make_pair(n, **kw)
    assert gpu.n_segments == 169
    gpu.set_kernel(variant, lanes)
    both((gpu, cpu), lambda e: (e.reset(seed=23), close_gap(e, 24.0, 10.0)))
    for env in (gpu, cpu):
        a = env.make_action(0.1, 80.0, 9, 3.0, 40.0)
        env.step_many(a, 1)
        env.step_many(a, 1500)
    check(gpu, cpu, n)
    assert int(gpu.state.spark_count.sum()) > 100 and not bool(gpu.state.is_wire_broken.any())


def test_per_environment_geometry_config5():
    """BASELINE config 5: per-env workpiece_height / wire_diameter / current_mode."""
    n = 192
    rng = np.random.default_rng(2024)
    h = rng.uniform(10.0, 30.0, n)
    d = rng.choice([0.10, 0.15, 0.20, 0.25, 0.30], n)
    mode = rng.choice([1, 3, 5, 7, 9, 11, 13, 15, 17], n).astype(np.int32)
    kw = dict(workpiece_height=h, wire_diameter=d, config=EnvironmentConfig(target_cutting_distance=5000.0))
    gpu, cpu = make_pair(n, **kw)
    assert gpu.n_segments == cpu.n_segments and 350 <= gpu.n_segments <= 450
    both((gpu, cpu), lambda e: (e.reset(seed=2024), close_gap(e, 24.0, 10.0)))
    for variant, lanes in ((1, 0), (5, 0), (2, 4), (2, 8), (2, 16), (2, 0), (10, 8), (11, 4), (11, 8), (11, 16)):
        gpu.set_kernel(variant, lanes)
        for env in (gpu, cpu):
            a = env.make_action(0.1, 80.0, mode, 3.0, 40.0)
            env.step_many(a, 700)
        check(gpu, cpu, n)
        if variant in (2, 10, 11):
            assert {2: "wedm_step_lanes_pk", 10: "wedm_step_lanes<", 11: "wedm_step_lanes_served"}[variant] in gpu._backend.last_kernel()
    assert int(gpu.state.spark_count.sum()) > 100


SCENARIOS = {
    "hard_short": dict(init=lambda e: close_gap(e, 11.0, 10.0), action=(-0.5, 80.0, 5, 3.0, 80.0), steps=400),
    "debris_short": dict(init=lambda e: (close_gap(e, 20.0, 10.0), setattr(e.state, "debris_volume", 0.0316)),
                         action=(0.0, 80.0, 5, 3.0, 80.0), steps=3000),
    "random_short": dict(kw=dict(ignition_params=IgnitionModuleParameters(random_short_max_probability=0.004)),
                         init=lambda e: close_gap(e, 30.0, 10.0), action=(0.1, 80.0, 5, 3.0, 80.0), steps=3000),
    "collision": dict(init=lambda e: (close_gap(e, 50.0, 149.5), setattr(e.state, "wire_velocity", 20000.0)),
                      action=(1.0, 80.0, 5, 3.0, 80.0), steps=200),
    "target_reached": dict(init=lambda e: close_gap(e, 25.0, 10.0, 25.002), action=(0.1, 80.0, 5, 3.0, 80.0), steps=4000),
    "velocity_mode": dict(kw=dict(mechanics_control_mode="velocity"), init=lambda e: None,
                          action=(200.0, 80.0, 5, 3.0, 80.0), steps=3000),
    "limits": dict(kw=dict(mechanics_params=MechanicsModuleParameters(max_acceleration=2.0e3, max_jerk=5.0e6, max_speed=1.5)),
                   init=lambda e: None, action=(1.0, 80.0, 5, 3.0, 80.0), steps=1500),
    "zero_fallbacks": dict(init=lambda e: close_gap(e), action=(0.1, 0.0, 5, 0.0, 0.0), steps=2600),
    "no_unwinding": dict(init=lambda e: (close_gap(e), setattr(e.state, "wire_unwinding_velocity", 0.0)),
                         action=(0.1, 80.0, 13, 2.0, 30.0), steps=2000),
}


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_edge_scenarios_match_oracle(name):
    """The reference's edge paths, 128 environments each."""
    sc = SCENARIOS[name]
    n = 128
    gpu, cpu = make_pair(n, **sc.get("kw", {}))
    both((gpu, cpu), lambda e: (e.reset(seed=31), sc["init"](e)))
    for env in (gpu, cpu):
        a = env.make_action(*sc["action"])
        done = 0
        while done < sc["steps"]:
            k = min(777, sc["steps"] - done)
            env.step_many(a, k)
            done += k
    check(gpu, cpu, n)
    if name in ("collision", "target_reached"):
        assert bool(gpu.state.done.any())


def test_wire_break_early_return():
    """Tmax > 1500 K: the step returns before mechanics and clocks (wire_edm.py:129-130)."""
    n = 64
    gpu, cpu = make_pair(n)
    for env in (gpu, cpu):
        env.reset(seed=9)
        T = env.state.wire_temperature
        T[: n // 2, 180:186] = 1600.0   # breaks at the first step
        T[n // 2:, 180:181] = 1502.0    # only enters the critical band
        env.step_many(env.make_action(), 50)
    check(gpu, cpu, n)
    assert gpu.state.is_wire_broken[: n // 2].all() and not gpu.state.is_wire_broken[n // 2:].any()
    assert (gpu.state.time[: n // 2] == 0).all() and (gpu.state.time[n // 2:] == 50).all()


def test_partial_reset_and_episode_streams():
    n = 128
    gpu, cpu = make_pair(n)
    mask = np.zeros(n, dtype=bool)
    mask[::3] = True
    for env in (gpu, cpu):
        env.reset(seed=77)
        close_gap(env)
        a = env.make_action()
        env.step_many(a, 1500)
        env.reset(options={"mask": mask})       # new episode, same key -> different stream
        env.state.workpiece_position[torch.as_tensor(mask)] = 25.0
        env.state.wire_position[torch.as_tensor(mask)] = 10.0
        env.step_many(a, 1500)
    check(gpu, cpu, n)
    assert (gpu.state.time[torch.as_tensor(mask).cuda()] == 1500).all()
    assert (gpu.state.episode[torch.as_tensor(mask).cuda()] == 1).all()


def test_invalid_mode_raises_on_host_like_the_reference():
    env = WireEDMEnv(num_envs=64, device="cuda:0")
    env.reset(seed=0)
    with pytest.raises(ValueError, match="not available in crater data"):
        env.step(env.make_action(current_mode=2))


def test_single_spark_known_answer_on_gpu(golden_dir):
    """F2 (experiments/single_spark_animation.py): ignition disabled, spark forced from
    the host before each microsecond; T must equal the reference's recorded field."""
    from tests._golden import Fixture

    fx = Fixture(golden_dir / "f2_single_spark.npz")
    env = WireEDMEnv(num_envs=64, device="cuda:0", disable_ignition=True)
    env.reset(seed=42)
    env.state.workpiece_position = 50.0
    env.state.wire_position = 40.0
    env.state.target_position = 5000.0
    env.state.wire_unwinding_velocity = 0.0
    snaps = dict(zip(fx.T_snap_steps.tolist(), fx.T_snaps))
    act = env.make_action(0.0, 80.0, 13, 2.0, 1000.0)
    for step in range(fx.n_steps):
        st, y, dur, V, I = fx.forced[step]
        env.state.spark_state = int(st)
        env.state.spark_location = float(y)
        env.state.spark_duration = int(dur)
        env.state.voltage = float(V)
        env.state.current = float(I)
        env.step(act)
        if step in snaps:
            T = env.state.wire_temperature[7].cpu().numpy()
            assert np.array_equal(T, snaps[step]), f"step {step}: max |dT| {np.abs(T - snaps[step]).max()}"
    assert float(env.state.wire_position[0]) == float(fx.float_row("wire_position")[-1])


def test_reference_fixtures_with_injected_philox_on_gpu(golden_dir):
    """F3: the REFERENCE consumed this build's Philox variates (tools/gen_golden.py);
    environments 0,1,2,3,777,65535 of a 65 536-wide batch must reproduce its per-step
    discrete state exactly and its floats to the stated tolerance."""
    from tests._golden import Fixture

    ids = [0, 1, 2, 3, 777, 65535]
    fxs = [Fixture(golden_dir / f"f3_philox_env{i}.npz") for i in ids]
    n = 65536
    env = WireEDMEnv(num_envs=n, device="cuda:0")
    env.reset(seed=1234)
    close_gap(env, 25.0, 10.0, 5000.0)
    act = env.make_action(0.1, 80.0, 5, 3.0, 80.0)
    idx = torch.tensor(ids, device="cuda")
    steps = fxs[0].n_steps
    rec_state = torch.empty((steps, len(ids)), dtype=torch.int8, device="cuda")
    rec_i32 = torch.empty((steps, 3, len(ids)), dtype=torch.int32, device="cuda")
    rec_f64 = torch.empty((steps, 6, len(ids)), dtype=torch.float64, device="cuda")
    st = env.state
    for step in range(steps):
        env.step(act)
        rec_state[step] = st.spark_state[idx]
        rec_i32[step, 0] = st.spark_duration[idx]
        rec_i32[step, 1] = st.time[idx]
        rec_i32[step, 2] = st.debris_short_remaining[idx]
        for j, name in enumerate(("workpiece_position", "wire_position", "wire_velocity", "debris_volume",
                                  "flow_rate", "wire_max_temperature")):
            rec_f64[step, j] = getattr(st, name)[idx]
    rs, ri, rf = rec_state.cpu().numpy(), rec_i32.cpu().numpy(), rec_f64.cpu().numpy()
    for c, fx in enumerate(fxs):
        assert np.array_equal(rs[:, c], fx.int_row("spark_state")), f"env {ids[c]} spark_state"
        assert np.array_equal(ri[:, 0, c], fx.int_row("spark_dur"))
        assert np.array_equal(ri[:, 1, c], fx.int_row("time"))
        assert np.array_equal(ri[:, 2, c], fx.int_row("debris_short_remaining"))
        fs = fx.float_steps
        for j, name in enumerate(("workpiece_position", "wire_position", "wire_velocity")):
            assert np.array_equal(rf[fs, j, c], fx.float_row(name)), f"env {ids[c]} {name} not bit-exact"
        np.testing.assert_allclose(rf[fs, 3, c], fx.float_row("debris_volume"), rtol=1e-12, atol=0)
        np.testing.assert_allclose(rf[fs, 4, c], fx.float_row("flow_rate"), rtol=1e-12, atol=0)
        np.testing.assert_allclose(rf[fs, 5, c], fx.float_row("tmax"), rtol=0, atol=1e-4)
        T = env.state.wire_temperature[ids[c]].cpu().numpy()
        assert np.abs(T - fx.T_snaps[-1]).max() <= 1e-4


def test_full_size_fusion_and_sharding_invariance():
    """BASELINE batch (65 536 envs, 128 segments): properties that hold at any size.
      * fusion: step_many(1000) == 1000 x step() bit for bit (LDS kernel vs split global-memory kernel);
      * sharding: the upper half computed alone with env_id_offset reproduces itself."""
    n = 65536
    kw = dict(wire_params=WireModuleParameters(segment_len=0.625))
    a_env = WireEDMEnv(num_envs=n, device="cuda:0", **kw)
    b_env = WireEDMEnv(num_envs=n, device="cuda:0", **kw)
    half = WireEDMEnv(num_envs=n // 2, device="cuda:0", env_id_offset=n // 2, **kw)
    for env in (a_env, b_env, half):
        env.reset(seed=4321)
        close_gap(env, 22.0, 10.0)
    act = a_env.make_action(0.1, 80.0, 5, 3.0, 80.0)
    a_env.step_many(act, 1000)
    a_env.step_many(act, 300)
    assert "wedm_step_regs<2>" in a_env._backend.last_kernel()
    for _ in range(1300):
        b_env.step(act)
    assert "wedm_step_stream<2>" in b_env._backend.last_kernel()
    half.step_many(half.make_action(0.1, 80.0, 5, 3.0, 80.0), 1300)
    torch.cuda.synchronize()
    A, B, H = a_env.state.clone_blocks(), b_env.state.clone_blocks(), half.state.clone_blocks()
    assert_blocks_equal(A, B, n)
    upper = {k: v[:, n // 2: n] for k, v in A.items()}
    assert_blocks_equal(H, upper, n // 2)
    assert int(a_env.state.spark_count.sum()) > 10000


def test_gap_controller_driver_on_gpu_matches_reference_fixture(golden_dir):
    """§8f-3: the reference's run_simulation.py driver with the gap controller evaluated ON the
    GPU (no host round trip for the action), one microsecond per launch, against the reference's
    own recording: discrete state and positions exact, the rest within the stated tolerance."""
    from sparc_amd import GapController
    from tests._fixture_env import check_step
    from tests._golden import Fixture

    fxs = {i: Fixture(golden_dir / f"f7_gap_controller_philox_env{i}.npz") for i in (0, 9)}
    env = WireEDMEnv(num_envs=64, device="cuda:0")
    env.reset(seed=77)
    close_gap(env, 70.0, 10.0, 5000.0)
    ctl = GapController()
    action = ctl(env)
    steps = 5200
    sampled = set(range(0, steps, 37)) | set(range(990, 1010)) | set(range(4990, 5010))
    for step in range(steps):
        env.step(action)
        latch = (step + 1) % 1000 == 1 and step > 0   # calls 1001, 2001, ... (host-side schedule)
        if step in sampled or latch:
            for i, fx in fxs.items():
                check_step(env, fx, i, step, exact_floats=False)
        if latch:
            assert bool(env.state.control_step.all())
            action = ctl(env)


def test_run_controlled_on_gpu_matches_oracle():
    """Fused control-interval launches + on-device controller: GPU == oracle, bit for bit."""
    from sparc_amd import GapController, run_controlled

    n = 256
    gpu, cpu = make_pair(n)
    for env in (gpu, cpu):
        env.reset(seed=123)
        close_gap(env, 40.0, 10.0, 5000.0)
        assert run_controlled(env, GapController(desired_gap=8.0, current_mode=9), 6500) == 6500
    check(gpu, cpu, n)
    assert int(gpu.state.spark_count.sum()) > 100
    assert any(k in gpu._backend.last_kernel() for k in ("wedm_step_packed", "wedm_step_fused", "wedm_step_regs_wide"))


def test_vector_env_autoreset_on_gpu():
    from sparc_amd import WireEDMVectorEnv

    env = WireEDMEnv(num_envs=128, device="cuda:0")
    vec = WireEDMVectorEnv(env)
    vec.reset(seed=3)
    close_gap(env, 25.0, 10.0, 5000.0)
    env.state.target_position[:64] = 25.0005
    act = env.make_action()
    seen = torch.zeros(128, dtype=torch.bool, device="cuda")
    for _ in range(4):
        _, _, term, trunc, _ = vec.step(act)
        seen |= term
    assert seen[:64].all() and not seen[64:].any()
    assert (vec.episode_count[:64] >= 1).all() and (env.state.time[64:] == 4000).all()


@pytest.mark.parametrize("segment_len,n_seg", [(80.0, 1), (40.0, 2), (26.0, 3), (16.0, 5), (8.5, 9), (4.7, 17)])
def test_tiny_wires_all_kernels(segment_len, n_seg):
    """Degenerate grids: 1..17 segments (boundary cell, last cell and zone collapse onto each
    other), odd batch size, every kernel variant that accepts the shape."""
    n = 77
    kw = dict(wire_params=WireModuleParameters(segment_len=segment_len))
    gpu, cpu = make_pair(n, **kw)
    assert gpu.n_segments == n_seg
    both((gpu, cpu), lambda e: (e.reset(seed=8), close_gap(e, 24.0, 10.0)))
    from sparc_amd._lib import WedmError

    ran = 0
    for variant, lanes in KERNELS + [(7, 0), (8, 0)] + SERVED:
        gpu.set_kernel(variant, lanes)
        a_g, a_c = gpu.make_action(0.1, 80.0, 9, 3.0, 30.0), cpu.make_action(0.1, 80.0, 9, 3.0, 30.0)
        try:
            gpu.step_many(a_g, 400)
        except WedmError as exc:
            assert "UNSUPPORTED" in str(exc)
            continue
        cpu.step_many(a_c, 400)
        check(gpu, cpu, n)
        ran += 1
    assert ran >= 3 and int(gpu.state.spark_count.sum()) > 0


# ------------------------------------------------------------------ device trace
TRACE_SIGNALS = ["voltage", "current", "wire_position", "workpiece_position", "debris_density", "flow_rate",
                 "wire_max_temperature", "time", "spark_duration", "spark_count", "spark_state", "is_short_circuit",
                 "done", "control_step"]


def assert_rings_equal(tg, tc, rows=None):
    torch.cuda.synchronize()
    assert tg.count == tc.count
    for b in ("f64", "i32", "i8"):
        if tg._buf[b] is None:
            assert tc._buf[b] is None
            continue
        G, Cc = tg._buf[b].cpu(), tc._buf[b]
        same = (G == Cc) | ((G != G) & (Cc != Cc)) if b == "f64" else (G == Cc)
        assert bool(same.all()), f"trace block {b}: {int((~same).sum())} of {same.numel()} differ"
    if tg._T is not None:
        G, Cc = tg._T.cpu(), tc._T
        if rows is not None:   # per-environment wires: rows past the environment's own n_seg are not written
            keep = torch.arange(G.shape[1])[None, :, None] < rows[None, None, :]
            G, Cc = torch.where(keep, G, 0), torch.where(keep, Cc, 0)
        assert torch.equal(G, Cc), f"trace T: {int((G != Cc).sum())} of {G.numel()} differ"


@pytest.mark.parametrize("variant,lanes", KERNELS + [(8, 0), (7, 0), (7, 1)])
def test_device_trace_ring_matches_oracle(variant, lanes):
    """The ring the kernels fill inside fused launches == the ring the oracle seam fills by
    sampling after single microseconds: every slot, every traced row, wire temperature included."""
    n = 200
    # (the register kernel holds wires of at most 128 segments: its TRACE instantiation, one and two lanes per environment)
    gpu, cpu = make_pair(n, **(dict(wire_params=WireModuleParameters(segment_len=0.625)) if variant == 7 else {}))
    gpu.set_kernel(variant, lanes)
    both((gpu, cpu), lambda e: (e.reset(seed=321), close_gap(e)))
    if (variant == 3 and (-(-gpu.n_segments // lanes) + 1) > 160) or \
       (variant == 4 and (2 * -(-gpu.n_segments // (2 * lanes)) + 2) > 160):
        pytest.skip("chunk does not fit in LDS (covered by test_default_config_fused_matches_oracle)")
    gpu.state.target_position[20] = 25.0005   # one traced environment terminates early
    cpu.state.target_position[20] = 25.0005
    traces = [e.bind_trace(TRACE_SIGNALS, every=3, capacity=300, envs=(13, 150), wire_temperature=True)
              for e in (gpu, cpu)]
    for env in (gpu, cpu):
        a = env.make_action(0.1, 80.0, 5, 3.0, 80.0)
        for k in (700, 1, 2, 650):          # 1353 us -> 451 samples through a 300-slot ring
            env.step_many(a, k)
    assert traces[0].count == 451
    assert_rings_equal(*traces)
    check(gpu, cpu, n)
    got = traces[0].read()
    assert bool(got["done"][-1, 7]) and int((got["spark_state"] == 1).sum()) > 0
    assert got["wire_temperature"].shape == (300, 150, gpu.n_segments)
    if variant == 7:
        assert "wedm_step_regs<" in gpu._backend.last_kernel()
    # no trace bound -> the instantiation without the trace point runs, results unchanged
    for env in (gpu, cpu):
        env.unbind_trace()
        env.step_many(env.make_action(0.1, 80.0, 5, 3.0, 80.0), 300)
    check(gpu, cpu, n)


def test_device_trace_config3_every_microsecond_all_envs():
    n = 1024
    kw = dict(wire_params=WireModuleParameters(segment_len=0.625))
    gpu, cpu = make_pair(n, **kw)
    gpu.set_kernel(4, 2)   # the kernel the 65 536-environment headline workload runs
    both((gpu, cpu), lambda e: (e.reset(seed=9), close_gap(e)))
    traces = [e.bind_trace(["voltage", "spark_state", "time"], every=1, capacity=1001) for e in (gpu, cpu)]
    for env in (gpu, cpu):
        a = env.make_action(0.1, 80.0, 9, 3.0, 30.0)
        env.step_many(a, 1000)
        env.step_many(a, 500)
    assert "wedm_step_packed" in gpu._backend.last_kernel()
    assert_rings_equal(*traces)
    check(gpu, cpu, n)
    v = traces[0].read(last=1001)["voltage"]
    assert v.shape == (1001, n) and float(v.min()) == 0.0 and float(v.max()) == 80.0


def test_device_trace_per_environment_geometry():
    n = 96
    rng = np.random.default_rng(7)
    h = rng.uniform(10.0, 30.0, n)
    d = rng.choice([0.10, 0.20, 0.30], n)
    kw = dict(workpiece_height=h, wire_diameter=d, config=EnvironmentConfig(target_cutting_distance=5000.0))
    gpu, cpu = make_pair(n, **kw)
    both((gpu, cpu), lambda e: (e.reset(seed=4), close_gap(e, 24.0, 10.0)))
    n_seg = gpu._geom_i32[0, :n].cpu()   # WEDM_GI_N_SEG
    for variant in (2, 1, 5):
        gpu.set_kernel(variant, 0)
        traces = [e.bind_trace(["voltage", "time", "spark_state"], every=10, capacity=64, envs=(5, 80),
                               wire_temperature=True) for e in (gpu, cpu)]
        for env in (gpu, cpu):
            env.step_many(env.make_action(0.1, 80.0, 7, 3.0, 40.0), 400)
        assert_rings_equal(*traces, rows=n_seg[5:85])
        check(gpu, cpu, n)


def test_single_microsecond_launches_feed_the_trace():
    n = 64
    gpu, cpu = make_pair(n)
    both((gpu, cpu), lambda e: (e.reset(seed=2), close_gap(e)))
    traces = [e.bind_trace(["voltage", "time"], every=2, capacity=16, wire_temperature=True) for e in (gpu, cpu)]
    for env in (gpu, cpu):
        a = env.make_action()
        for _ in range(41):
            env.step(a)
    assert "wedm_step_stream" in gpu._backend.last_kernel() and traces[0].count == 20
    assert_rings_equal(*traces)
    check(gpu, cpu, n)


def test_bind_trace_rejects_bad_descriptors():
    from sparc_amd import _abi
    from sparc_amd._lib import WedmError

    env = WireEDMEnv(num_envs=64, device="cuda:0")
    buf = torch.zeros(1024, dtype=torch.float64, device="cuda:0")
    ok = dict(f64=buf.data_ptr(), i32=None, i8=None, T=None, f64_mask=1, i32_mask=0, i8_mask=0, env_lo=0, env_count=8,
              every=1, capacity=4, reserved0=0)
    for bad in (dict(f64_mask=1 << 26), dict(f64_mask=1 << 25), dict(f64=None), dict(i32_mask=1), dict(every=0), dict(capacity=0),
                dict(env_lo=60, env_count=8), dict(env_count=0), dict(f64=None, f64_mask=0)):
        with pytest.raises(WedmError, match="WEDM_ERR_BAD_ARG"):
            env._backend.bind_trace(_abi.TraceDesc(**{**ok, **bad}))
    env._backend.bind_trace(_abi.TraceDesc(**ok))
    env.step_many(env.make_action(), 3)
    assert env._backend.trace_samples() == 3
    env._backend.bind_trace(None)
    assert env._backend.trace_samples() == 0


def test_voltage_controller_on_gpu_matches_oracle():
    """§8f-3: PI voltage controller averaging the kernel-side 1 ms voltage ring, fused control
    intervals: GPU == oracle bit for bit (state, integrators, averaged voltage)."""
    from sparc_amd import SimulationLogger, VoltageController, run_controlled

    n = 256
    gpu, cpu = make_pair(n)
    ctls, logs = [], []
    for env in (gpu, cpu):
        env.reset(seed=31)
        close_gap(env, 22.0, 10.0, 5000.0)
        trace = env.bind_trace(["voltage", "time", "wire_position"], every=1, capacity=1101)
        ctl = VoltageController(30.0).bind(env, trace)
        lg = SimulationLogger({"signals_to_log": ["time", "voltage", "wire_position"], "log_frequency": {"type": "every_step"}})
        lg.attach(env, trace=trace)
        assert run_controlled(env, ctl, 5400, logger=lg) == 5400
        ctls.append(ctl)
        logs.append(lg.get_data())
    check(gpu, cpu, n)
    assert torch.equal(ctls[0].integral_error.cpu(), ctls[1].integral_error)
    assert torch.equal(ctls[0].average_voltage().cpu(), ctls[1].average_voltage())
    for k in ("time", "voltage", "wire_position"):
        assert logs[0][k].shape == (5400, n) and np.array_equal(logs[0][k], logs[1][k]), k
    assert int(gpu.state.spark_count.sum()) > 1000


def test_voltage_controller_driver_on_gpu_matches_reference_fixture(golden_dir):
    """The reference's run_simulation.py loop with ITS voltage controller (fixture) against the
    GPU: one microsecond per launch, the voltage ring filled by the kernel, commands computed on
    the device.  Discrete state, positions, voltages and servo commands exact."""
    from sparc_amd import VoltageController
    from tests._fixture_env import check_step
    from tests._golden import Fixture

    fx = Fixture(golden_dir / "f9_voltage_controller_philox_env2.npz")
    env = WireEDMEnv(num_envs=64, device="cuda:0")
    env.reset(seed=79)
    close_gap(env, 70.0, 10.0, 5000.0)
    ctl = VoltageController(30.0)
    action = ctl(env)
    steps = 4300
    sampled = set(range(0, steps, 41)) | set(range(990, 1010)) | set(range(3990, 4010))
    for step in range(steps):
        env.step(action)
        latch = (step + 1) % 1000 == 1 and step > 0
        if step in sampled or latch:
            check_step(env, fx, 2, step, exact_floats=False)
        if latch:
            action = ctl(env)
            assert float(action.servo[2]) == fx.actions[fx.action_idx[step + 1], 0], step


def test_crater_statistics_on_gpu_match_reference_fixture(golden_dir):
    """§8f-4: the running crater statistics kept by the kernels against the reference's
    `get_crater_statistics()` (fixture F10, 140 craters), fused launches, three kernel variants."""
    from tests._golden import Fixture

    fx = Fixture(golden_dir / "f10_crater_statistics_philox_env1.npz")
    total, mean, std, vmin, vmax = fx.data["crater_stats"].tolist()
    for variant, lanes in ((0, 0), (3, 16), (1, 0), (5, 0)):
        env = WireEDMEnv(num_envs=64, device="cuda:0", crater_log_capacity=160)
        env.set_kernel(variant, lanes)
        env.reset(seed=81)
        close_gap(env, 22.0, 10.0, 5000.0)
        act = env.make_action(0.05, 80.0, 13, 2.0, 20.0)
        for _ in range(12):
            env.step_many(act, 1000)
        got = {k: v[1].item() for k, v in env.get_crater_statistics().items()}
        assert got["total_craters"] == total, (variant, got)
        assert got["min_volume_um3"] == vmin and got["max_volume_um3"] == vmax
        assert abs(got["mean_volume_um3"] - mean) <= 1e-12 * mean and abs(got["std_volume_um3"] - std) <= 1e-12 * std
        assert float(env.state.workpiece_position[1]) == float(fx.float_row("workpiece_position")[-1])
        # the whole `crater_volumes_um3` list of the reference (material.py:133), from the kernel-side crater log
        vols = env.get_crater_volumes(1).cpu().numpy()
        assert vols.shape == fx.data["crater_volumes_um3"].shape
        np.testing.assert_allclose(vols, fx.data["crater_volumes_um3"], rtol=1e-14, atol=0)


def test_checkpoint_resume_on_gpu(tmp_path):
    n = 512
    a = WireEDMEnv(num_envs=n, device="cuda:0")
    a.reset(seed=12)
    close_gap(a)
    act = a.make_action(0.1, 80.0, 9, 3.0, 40.0)
    a.step_many(act, 1300)
    a.save_checkpoint(tmp_path / "ck.pt")
    a.step_many(act, 1200)
    b = WireEDMEnv(num_envs=n, device="cuda:0")
    b.load_checkpoint(tmp_path / "ck.pt")
    b.step_many(b.make_action(0.1, 80.0, 9, 3.0, 40.0), 1200)
    torch.cuda.synchronize()
    assert_blocks_equal(a.state.clone_blocks(), b.state.clone_blocks(), n)


def test_full_headline_batch_matches_oracle_bit_for_bit():
    """The bench workload itself (BASELINE configs[2]: 65 536 environments x 128 segments, the
    kernel the bench runs) against the CPU oracle on every byte of state, 2 control intervals."""
    n = 65536
    kw = dict(wire_params=WireModuleParameters(segment_len=0.625))
    gpu, cpu = make_pair(n, **kw)
    both((gpu, cpu), lambda e: e.reset(seed=1234))
    for env in (gpu, cpu):
        act = env.make_action(0.1, 80.0, 5, 3.0, 80.0)
        env.step_many(act, 1000)
        env.step_many(act, 1000)
    assert "wedm_step_regs<2>" in gpu._backend.last_kernel()
    check(gpu, cpu, n)
    assert int(gpu.state.spark_count.sum()) > 50000
    # the LDS kernel that ran this workload before the register kernel existed, same bytes
    gpu.set_kernel(4, 2)
    for env in (gpu, cpu):
        env.step_many(env.make_action(0.1, 80.0, 5, 3.0, 80.0), 1000)
    assert "wedm_step_packed<2>" in gpu._backend.last_kernel()
    check(gpu, cpu, n)


@pytest.mark.parametrize("k", range(8))
def test_randomized_parameter_reference_fixtures_on_gpu(golden_dir, k):
    """F11 on the GPU: eight reference runs with randomized parameters in every module; the
    per-microsecond trajectory comes back through the in-kernel trace of fused launches.
    Discrete state, clocks, positions, voltage / current exact; debris / flow <= 1e-12; T <= 1e-4 K."""
    from tests._fixture_env import env_from_fixture, run_fixture_through_trace
    from tests._golden import Fixture

    fx = Fixture(golden_dir / f"f11_random_params_{k}.npz")
    env = env_from_fixture(fx, 64, device="cuda:0")
    got = run_fixture_through_trace(env, fx, exact_floats=False)
    assert (got["spark_state"] == 1).sum() > 30
    assert "wedm_step_" in env._backend.last_kernel()


def _untaken_decisions():
    from tests.test_oracle_golden import UNTAKEN_DECISIONS

    # a mode below the table stays with the oracle: the batch ABI keeps the negative values of the mode row for
    # "None" (peak_current in wedm_device.h), and the action space is Box(1, 19) here as in the reference
    return [name for name in UNTAKEN_DECISIONS if "below_table" not in name]


@pytest.mark.parametrize("name", _untaken_decisions())
def test_untaken_decision_reference_fixtures_on_gpu(golden_dir, name):
    """F19 on the GPU: the reference runs recorded for the decisions of the scalar physics that no other recording takes
    (both speed clamps, a crater draw <= 0, debris flushed to 0, density saturated at 1, the sigmoid's cuts at +-500,
    k rho >= 2, the convection floor, a mode above the table).  Same comparison and tolerances as F11, and the witness
    of tests/test_oracle_golden.py repeated on the traced GPU trajectory: the kernels took the decision too."""
    from tests._fixture_env import FLOAT_MAP, INT_MAP, env_from_fixture, run_fixture_through_trace
    from tests._golden import Fixture
    from tests.test_oracle_golden import untaken_decision_witness

    fx = Fixture(golden_dir / f"{name}.npz")
    raised = fx.meta["raised"] is not None
    env = env_from_fixture(fx, 64, device="cuda:0", **(dict(strict_actions=False) if raised else {}))
    extra = ("h_eff_base", "dielectric_last_gap", "dielectric_last_density")
    got = run_fixture_through_trace(env, fx, exact_floats=False, extra=extra)
    assert "wedm_step_" in env._backend.last_kernel()
    assert len(got["spark_state"]) == fx.n_steps

    def row(field):
        return got[FLOAT_MAP[field] if field in FLOAT_MAP else INT_MAP[field]]

    untaken_decision_witness(name, fx, row)
    e = int(fx.meta["env_id"])
    assert not bool(env.state.error[e])
    if raised:   # the step at which the reference raised ValueError: the sticky ERROR row, at the fresh spark
        servo, tv, on, off, mode = fx.actions[0]
        env.step_many(env.make_action(servo, tv, int(mode), on, off), 1)
        assert bool(env.state.error[e]) and int(env.state.spark_state[e]) == 1 and int(env.state.spark_duration[e]) == 0
        assert float(env.state.current[e]) == 215.0


@pytest.mark.parametrize("case", range(int(os.environ.get("WEDM_FUZZ_CASES", "64"))))
def test_randomized_configurations_all_kernels_bit_exact(case):
    """Fuzz: random parameters in every module, random batch size / control mode / action / kernel
    variant (and per-environment geometry in a third of the cases): GPU == oracle on every byte.
    (64 cases in the default run; `WEDM_FUZZ_CASES=400` widens the hunt: 400 cases passed on the final builds of rounds 2 and 3.)"""
    _fuzz_case(case, False)


@pytest.mark.parametrize("case", range(int(os.environ.get("WEDM_FUZZ_F64_CASES", "40"))))
def test_randomized_configurations_float64_typing_bit_exact(case):
    """The same fuzz with the stencil in Numba's typing (`stencil_dtype="float64"`) over the kernels that carry it: the register
    kernels, the tile walk, the packed and the cell-by-cell any-geometry kernels, the stream kernel (single microseconds) and the
    global-memory kernel."""
    _fuzz_case(case, True)


def _fuzz_case(case, f64):
    from sparc_amd import DielectricModuleParameters, MaterialModuleParameters
    from sparc_amd._lib import WedmError

    rng = np.random.default_rng(9000 + case)
    u = rng.uniform
    n = int(rng.choice([65, 128, 200, 333]))
    per_env = case % 3 == 2
    kw = dict(
        mechanics_control_mode="velocity" if case % 4 == 1 else "position",
        config=EnvironmentConfig(workpiece_height=float(u(8, 32)), wire_diameter=float(rng.choice([0.1, 0.2, 0.3])),
                                 servo_interval=int(rng.choice([200, 500, 1000])), initial_gap=float(u(15, 40)),
                                 target_cutting_distance=5000.0),
        ignition_params=IgnitionModuleParameters(
            base_critical_density=float(u(0.05, 0.4)), gap_coefficient=float(u(0.005, 0.03)),
            sigmoid_steepness=float(rng.choice([50.0, 500.0])), hard_short_gap=float(u(1, 4)),
            debris_short_duration=int(rng.integers(10, 80)), random_short_duration=int(rng.integers(20, 120)),
            random_short_max_probability=float(rng.choice([0.0, 0.003, 0.01])), spark_voltage_factor=float(u(0.2, 0.5)),
            ignition_c_coeff=float(14.05 * u(0.9, 1.3))),
        wire_params=WireModuleParameters(segment_len=float(rng.choice([0.2, 0.25, 0.5, 0.625])),
                                         buffer_len_bottom=float(u(10, 40)), buffer_len_top=float(u(10, 40)),
                                         base_convection_coefficient=float(u(8000, 20000)),
                                         plasma_efficiency=float(u(0.05, 0.3)), critical_temp_threshold=float(u(0.7, 0.95))),
        material_params=MaterialModuleParameters(base_overcut=float(u(0.08, 0.2))),
        dielectric_params=DielectricModuleParameters(base_flow_rate=float(u(50, 200)), debris_obstruction_coeff=float(u(0.5, 3)),
                                                     reference_gap=float(u(15, 40)), dielectric_temperature=float(u(285, 300))),
        mechanics_params=MechanicsModuleParameters(omega_n=float(u(150, 400)), zeta=float(u(0.2, 0.9)),
                                                   max_speed=float(3e4 * u(0.3, 1.5))),
    )
    if per_env:
        kw["workpiece_height"] = rng.uniform(8, 32, n)
        kw["wire_diameter"] = rng.choice([0.1, 0.15, 0.25], n)
    if case >= 10 and case % 2:   # the cases with terminations: reset inside the launch + kernel-side reward + crater log
        kw.update(autoreset=True, reward="progress", crater_log_capacity=8)
    # the reference-compatible modes in a part of the cases: the reference's own reset (module state carries over, also
    # through the in-launch autoreset) and / or stepping on after `terminated`, with a masked reset between the kernels
    compat = case % 5 in (3, 4)
    if compat:
        kw.update(reset_semantics="reference", freeze_terminated=(case % 5 == 3))
    if f64:
        kw["stencil_dtype"] = "float64"
    gpu, cpu = make_pair(n, **kw)
    seed = int(rng.integers(1, 1 << 40))
    gaps, debris = rng.uniform(6, 30, n), rng.uniform(0, 0.01, n)
    extreme = case >= 10   # hard shorts, debris shorts, collisions, terminations, hot modes
    if extreme:
        gaps = np.where(rng.random(n) < 0.5, rng.uniform(0.5, 5, n), rng.uniform(5, 15, n))
        debris = np.where(rng.random(n) < 0.3, rng.uniform(0, 0.2, n), debris)
    for env in (gpu, cpu):
        env.reset(seed=seed)
        env.state.wire_position = 10.0
        env.state.workpiece_position = torch.as_tensor(10.0 + gaps)
        env.state.target_position = torch.as_tensor(np.where(np.arange(n) % 7 == 3, 10.0 + gaps + 0.01, 5000.0)) if extreme else 5000.0
        env.state.debris_volume = torch.as_tensor(debris) if (case % 2 or extreme) else 0.0
    variants = [(0, 0), (1, 0), (5, 0), (2, 4), (2, 8), (10, 4), (2, 2), (2, 16), (11, 4), (11, 8), (11, 16)] if per_env else KERNELS + [(0, 0), (7, 0), (8, 0)]
    if f64:   # (kernel 6: launches of one microsecond only -- any other draw of k is refused and skipped)
        variants = [(0, 0), (1, 0), (2, 4), (2, 8), (10, 4), (2, 2), (2, 16)] if per_env else \
            [(0, 0), (1, 0), (3, 0), (3, 8), (7, 0), (7, 1), (8, 0), (8, 16), (2, 4), (10, 4), (6, 0), (6, 4)]
    servo = rng.uniform(50, 300, n) if kw["mechanics_control_mode"] == "velocity" else rng.uniform(-0.05, 0.3, n)
    if extreme:
        servo = servo * rng.choice([1.0, 1.0, 20.0, -3.0], n)
    modes = rng.choice([15, 17] if extreme else [1, 3, 5, 7, 9, 11, 13, 15, 17], n).astype(np.int32)
    ran = 0
    drawn = [variants[i] for i in rng.permutation(len(variants))[:4]]
    if not per_env and not f64:   # every uniform-geometry case also runs a served kernel, last (the draws of the earlier rounds stay as they were)
        drawn.append(SERVED[case % 2])
    for variant, lanes in drawn:
        gpu.set_kernel(variant, lanes)
        k = int(rng.choice([1, 7, 400, 1300]))
        if f64 and variant == 6:
            k = 1
        if ran == 0:
            volt, on, off = float(u(60, 120)), float(rng.choice([1.5, 2.0, 3.0])), float(u(10, 60))
            acts = [env.make_action(servo, volt, modes, on, off) for env in (gpu, cpu)]
        try:
            gpu.step_many(acts[0], k)
        except WedmError as exc:
            assert "UNSUPPORTED" in str(exc)
            continue
        cpu.step_many(acts[1], k)
        torch.cuda.synchronize()
        diffs = block_diffs(gpu.state.clone_blocks(), cpu.state.clone_blocks(), n)
        assert not diffs, f"case {case}: kernel {gpu._backend.last_kernel()} after {k} us (n={n}, S={gpu.n_segments}):\n" + \
            "\n".join(diffs[:12])
        assert not f64 or "[f64 stencil]" in gpu._backend.last_kernel()
        if gpu.state.crater_log is not None:
            G, Cc = gpu.state.crater_log[:, :n].cpu(), cpu.state.crater_log[:, :n]
            cnt = gpu.state.spark_count.cpu()[None, :]   # slots written so far (a ring: all of them once the count passes the capacity)
            filled = torch.arange(G.shape[0])[:, None] < cnt
            assert torch.equal(torch.where(filled, G, 0), torch.where(filled, Cc, 0)), f"case {case}: crater log differs"
        ran += 1
        if compat:   # a second episode for a third of the environments: EDMState only, what the modules hold lives on
            for env in (gpu, cpu):
                env.reset(seed=seed + ran, options={"mask": np.arange(n) % 3 == ran % 3})
                wp = env.state.workpiece_position.cpu().numpy()
                env.state.wire_position = torch.as_tensor(np.where(np.arange(n) % 3 == ran % 3, wp - gaps, env.state.wire_position.cpu().numpy()))
    assert ran >= (2 if case < 20 else 1)   # (a widened hunt may draw three kernels that do not fit the geometry)


@pytest.mark.parametrize("variant,lanes", [(1, 0), (2, 4), (3, 8), (4, 4), (5, 0), (6, 8), (7, 0), (9, 8)])
def test_clock_high_word_across_the_32_bit_wrap_matches_oracle(variant, lanes):
    """`state.time` past 2**31 and 2**32 us: the kernels carry the low word (also the Philox counter word) through the
    launch and bump row TIME_HI when it wrapped inside it; every kernel == the oracle on every byte, in fused and in
    single-microsecond launches, with autoreset (a re-initialised environment starts again at 0 / 0)."""
    _clock_wrap(variant, lanes, 1, [2**31 - 300, 2**32 - 300, 2**32 - 1, 5 * 2**32 - 40])


# starts from which the clock's low word steps OVER 2**31 and 2**32 (never landing on them): in the first launch of one
# step, inside the fused launch of 298 steps and in the last launch
CLOCK_STARTS = {3: [2**31 - 301, 2**32 - 899, 2**32 - 1, 2**32 - 2, 2**32 - 3002, 5 * 2**32 - 40],
                7: [2**31 - 300, 2**32 - 1000, 2**32 - 1, 2**32 - 6, 2**32 - 4000, 5 * 2**32 - 40]}


@pytest.mark.parametrize("dt", [3, 7])
@pytest.mark.parametrize("variant,lanes", [(1, 0), (2, 4), (3, 8), (4, 4), (5, 0), (6, 8), (7, 0), (9, 8)])
def test_clock_high_word_across_the_32_bit_wrap_at_other_physics_steps(variant, lanes, dt):
    """The same with config.dt = 3 and 7: the low word passes 2**32 without ever being 0 (2**32 - 1 -> 2**32 + 2), so a
    wrap test on `time == 0`, or one that assumes a step of 1 us, misses it."""
    for s in CLOCK_STARTS[dt]:
        for edge in (2**31, 2**32, 5 * 2**32):
            assert (edge - s) % dt != 0 or edge < s or edge - s > 1502 * dt, (s, edge)
        assert any(s < edge <= s + 1502 * dt for edge in (2**31, 2**32, 5 * 2**32)), s
    _clock_wrap(variant, lanes, dt, CLOCK_STARTS[dt])


def _clock_wrap(variant, lanes, dt, starts):
    n = 192
    kw = dict(autoreset=True, config=EnvironmentConfig(target_cutting_distance=5000.0) if dt == 1 else
              EnvironmentConfig(target_cutting_distance=5000.0, dt=dt))
    if variant == 7:   # (the register kernel holds wires of at most 128 segments)
        kw["wire_params"] = WireModuleParameters(segment_len=0.625)
    gpu, cpu = make_pair(n, **kw)
    start = torch.tensor(starts * (n // len(starts)))
    for env in (gpu, cpu):
        env.reset(seed=5)
        close_gap(env, 22.0, 10.0)
        env.state.target_position = torch.where(torch.arange(n) % 5 == 1, 22.000001, 5000.0)   # the first crater terminates these: re-initialised by the next launch
        env.state.time = start
        env.state.time_since_open_voltage = start
    gpu.set_kernel(variant, lanes)
    for env in (gpu, cpu):
        a = env.make_action(0.1, 80.0, 9, 3.0, 30.0)
        for k in (1, 1, 298, 1, 1, 1200):
            env.step_many(a, k)
    check(gpu, cpu, n)
    t = gpu.state.time.cpu()
    alive = gpu.state.episode.cpu() == 0
    assert alive.sum() > n // 2 and (~alive).sum() > 0
    assert torch.equal(t[alive], (start + 1502 * dt)[alive]) and int(t[~alive].max()) < 1502 * dt
    assert (gpu.state.time_high32.cpu()[alive] == ((start + 1502 * dt) >> 32)[alive]).all()


def test_float64_stencil_on_the_tile_walk_over_wire_lengths_and_lane_counts():
    """`stencil_dtype="float64"` on kernel 3 (the fused tile walk with per-cell coefficients): wire lengths across the
    tile residues x every lane count, sparks, current and a frozen (broken) environment in the batch == the oracle's
    STENCIL_F64, every byte."""
    from sparc_amd._lib import WedmError

    n_envs, ran = 96, 0
    for n_seg in (9, 16, 17, 31, 33, 57, 64, 65, 100, 127, 128, 129, 163):
        gpu, cpu = make_pair(n_envs, stencil_dtype="float64", wire_params=WireModuleParameters(segment_len=80.0 / (n_seg + 0.5)),
                             config=EnvironmentConfig(target_cutting_distance=5000.0))

        def scenario(env):
            env.reset(seed=500 + n_seg)
            close_gap(env, 21.0, 10.0)
            hot = env.state.wire_temperature
            hot[5, n_seg // 2] = 1600.0
            hot[70, n_seg - 1] = 900.0
            hot[71, 1] = 900.0
            return env.make_action(0.1, 80.0, 17, 3.0, 20.0)

        act = scenario(cpu)
        cpu.step_many(act, 300)
        want = cpu.state.clone_blocks()
        for lanes in (1, 2, 4, 8, 16):
            act = scenario(gpu)
            gpu.set_kernel(3, lanes)
            try:
                gpu.step_many(act, 300)
            except WedmError as exc:
                assert "UNSUPPORTED" in str(exc)
                continue
            torch.cuda.synchronize()
            assert "wedm_step_fused" in gpu._backend.last_kernel() and "[f64 stencil]" in gpu._backend.last_kernel()
            diffs = block_diffs(gpu.state.clone_blocks(), want, n_envs)
            assert not diffs, f"n_seg {n_seg}, kernel {gpu._backend.last_kernel()}:\n" + "\n".join(diffs[:10])
            ran += 1
        gpu.close()
    assert ran >= 60


@pytest.mark.parametrize("variant", [7, 8])
def test_float64_stencil_on_the_register_kernels_over_wire_lengths_and_lane_counts(variant):
    """`stencil_dtype="float64"` on kernels 7 and 8 (the register walks, interior cells by `cell_f64`, odd cells by the
    predicated float64-typed formula): wire lengths across the tile residues x the lane counts, sparks, current and a frozen
    (broken) environment in the batch, fused launches and single microseconds, with and without a trace sample in the launch
    == the oracle's STENCIL_F64, every byte."""
    from sparc_amd._lib import WedmError

    n_envs, ran = 96, 0
    sizes = (9, 16, 17, 31, 33, 57, 64, 65, 100, 127, 128) if variant == 7 else (9, 17, 33, 64, 100, 128, 129, 200, 256, 257, 400, 450, 512)
    name = "wedm_step_regs<{}>[f64 stencil]" if variant == 7 else "wedm_step_regs_wide<{}>[f64 stencil]"
    for n_seg in sizes:
        gpu, cpu = make_pair(n_envs, stencil_dtype="float64", wire_params=WireModuleParameters(segment_len=80.0 / (n_seg + 0.5)),
                             config=EnvironmentConfig(target_cutting_distance=5000.0))

        def scenario(env):
            env.reset(seed=500 + n_seg)
            close_gap(env, 21.0, 10.0)
            hot = env.state.wire_temperature
            hot[5, n_seg // 2] = 1600.0
            hot[70, n_seg - 1] = 900.0
            hot[71, 1] = 900.0
            return env.make_action(0.1, 80.0, 17, 3.0, 20.0)

        act = scenario(cpu)
        cpu.step_many(act, 300)
        for _ in range(3):
            cpu.step(act)
        cpu.step_many(act, 200)
        want = cpu.state.clone_blocks()
        for lanes in ((1, 2) if variant == 7 else (4, 8, 16)):
            for traced in (False, True):
                act = scenario(gpu)
                gpu.set_kernel(variant, lanes)
                if traced:
                    gpu.bind_trace(["voltage"], every=7, capacity=128)
                try:
                    gpu.step_many(act, 300)
                except WedmError as exc:   # (32 cells per lane do not cover this wire)
                    assert variant == 8 and "UNSUPPORTED" in str(exc) and 32 * lanes < n_seg
                    if traced:
                        gpu.unbind_trace()
                    continue
                assert name.format(lanes) in gpu._backend.last_kernel(), gpu._backend.last_kernel()
                gpu.set_kernel(0, 0)   # (single microseconds: whatever the plan takes for this typing)
                for _ in range(3):
                    gpu.step(act)
                gpu.set_kernel(variant, lanes)
                gpu.step_many(act, 200)
                torch.cuda.synchronize()
                diffs = block_diffs(gpu.state.clone_blocks(), want, n_envs)
                assert not diffs, f"n_seg {n_seg}, lanes {lanes}, traced {traced}:\n" + "\n".join(diffs[:10])
                if traced:
                    gpu.unbind_trace()
                ran += 1
        gpu.close()
    assert ran >= (44 if variant == 7 else 50)


def test_float64_stencil_on_the_stream_kernel_single_microseconds():
    """`stencil_dtype="float64"` on kernel 6 (launches of one microsecond: the register walk of the single-microsecond
    instantiation in Numba's typing; waves with a frozen environment on its per-cell code): wire lengths x lane counts, sparks,
    current, a broken wire and hot cells == the oracle's STENCIL_F64, every byte; fused launches in between run the plan's kernel."""
    from sparc_amd._lib import WedmError

    n_envs, ran = 96, 0
    for n_seg in (16, 33, 64, 100, 128, 200, 400):
        gpu, cpu = make_pair(n_envs, stencil_dtype="float64", wire_params=WireModuleParameters(segment_len=80.0 / (n_seg + 0.5)),
                             config=EnvironmentConfig(target_cutting_distance=5000.0))

        def scenario(env):
            env.reset(seed=700 + n_seg)
            close_gap(env, 21.0, 10.0)
            hot = env.state.wire_temperature
            hot[5, n_seg // 2] = 1600.0
            hot[70, n_seg - 1] = 900.0
            hot[71, 1] = 900.0
            return env.make_action(0.1, 80.0, 17, 3.0, 20.0)

        act = scenario(cpu)
        for k in (200, 1, 1, 1, 100, 1, 1):
            cpu.step_many(act, k)
        want = cpu.state.clone_blocks()
        for lanes in (1, 2, 4, 8, 16):
            act = scenario(gpu)
            try:
                for k in (200, 1, 1, 1, 100, 1, 1):
                    gpu.set_kernel(6 if k == 1 else 0, lanes if k == 1 else 0)
                    gpu.step_many(act, k)
                    if k == 1:
                        assert f"wedm_step_stream<{lanes}>[f64 stencil]" in gpu._backend.last_kernel(), gpu._backend.last_kernel()
            except WedmError as exc:   # (a chunk of more than 64 cells for this lane count)
                assert "UNSUPPORTED" in str(exc)
                continue
            torch.cuda.synchronize()
            diffs = block_diffs(gpu.state.clone_blocks(), want, n_envs)
            assert not diffs, f"n_seg {n_seg}, lanes {lanes}:\n" + "\n".join(diffs[:10])
            ran += 1
        gpu.close()
    assert ran >= 20


@pytest.mark.parametrize("n_seg", [400, 450, 129])
def test_float64_stencil_on_the_wide_register_kernel_at_two_blocks_per_cu(n_seg):
    """A batch of more than one wave per SIMD in the float64 typing runs the wide register kernel's 256-register instantiation
    (two blocks per CU; chosen by the plan for wires of more than 128 segments): a ragged batch, sparks, hot cells, a traced
    launch == the oracle's STENCIL_F64, every byte."""
    n = 4128 + 5
    gpu, cpu = make_pair(n, stencil_dtype="float64", wire_params=WireModuleParameters(segment_len=80.0 / (n_seg + 0.5)),
                         config=EnvironmentConfig(target_cutting_distance=5000.0))

    def scenario(env):
        env.reset(seed=900 + n_seg)
        close_gap(env, 21.0, 10.0)
        hot = env.state.wire_temperature
        hot[5, n_seg // 2] = 1600.0
        hot[4100, n_seg - 1] = 900.0
        hot[71, 1] = 900.0
        return env.make_action(0.1, 80.0, 17, 3.0, 20.0)

    act = scenario(cpu)
    cpu.step_many(act, 150)
    cpu.step_many(act, 50)
    want = cpu.state.clone_blocks()
    for traced in (False, True):
        act = scenario(gpu)
        if traced:
            gpu.bind_trace(["voltage"], every=7, capacity=64, envs=(0, 64))
        gpu.step_many(act, 150)   # the automatic plan
        assert "wedm_step_regs_wide<" in gpu._backend.last_kernel() and "[f64 stencil]" in gpu._backend.last_kernel(), gpu._backend.last_kernel()
        gpu.step_many(act, 50)
        torch.cuda.synchronize()
        diffs = block_diffs(gpu.state.clone_blocks(), want, n)
        assert not diffs, f"n_seg {n_seg}, traced {traced}:\n" + "\n".join(diffs[:10])
        if traced:
            gpu.unbind_trace()
    assert int(gpu.state.spark_count.sum()) > 100
    gpu.close()


@pytest.mark.parametrize("variant", [3, 4])
def test_handle_without_autoreset_moves_to_the_frozen_lane_tile_code_by_itself(variant):
    """A handle without autoreset runs the kernel instantiation without the frozen-lane tile code until one of its launches
    finds a terminated environment and says so through the host-visible word (no synchronisation; the handle follows a
    launch or two later); a reset of every environment takes it back.  Results == the oracle throughout."""
    n = 256
    gpu, cpu = make_pair(n, wire_params=WireModuleParameters(segment_len=0.625))
    gpu.set_kernel(variant, 2)
    for env in (gpu, cpu):
        env.reset(seed=21)
        close_gap(env, 22.0, 10.0)
        env.state.target_position = torch.where(torch.arange(n) % 3 == 0, 22.000001, 5000.0)
    names = []
    for _ in range(5):
        for env in (gpu, cpu):
            env.step_many(env.make_action(0.1, 80.0, 9, 3.0, 30.0), 400)
        torch.cuda.synchronize()
        names.append(gpu._backend.last_kernel())
    check(gpu, cpu, n)
    assert int(gpu.state.done.sum()) > n // 4
    assert "[frozen lanes ok]" not in names[0] and "[frozen lanes ok]" in names[-1], names
    for env in (gpu, cpu):
        env.reset(seed=22)
        env.step_many(env.make_action(), 50)
    assert "[frozen lanes ok]" not in gpu._backend.last_kernel()
    check(gpu, cpu, n)


SWEEP_N = list(range(9, 171))


@pytest.mark.parametrize("n_lo", SWEEP_N[::18])
def test_tile_geometry_sweep_every_wire_length_every_lane_count(n_lo):
    """Every wire length from 9 to 170 segments x every lane count x the tile-table kernels (fused, packed, stream; the
    register kernel up to 128 segments) against the oracle, on poisoned LDS.  The one real bug of round 2 lived exactly in `n_seg mod (8 L)` (a last cell
    closing a tile that a partial tile of cells past the wire's end follows): this walks through all of those residues --
    chunk lengths, tails of 1..7 cells, chunks wholly past the end, zone / contact boundaries at every tile offset -- with
    sparks (plasma patch), current (Joule tiles) and a wire break in the batch."""
    from sparc_amd._lib import WedmError

    n_envs, ran, refused = 96, 0, 0
    for n_seg in SWEEP_N[SWEEP_N.index(n_lo): SWEEP_N.index(n_lo) + 18]:
        kw = dict(wire_params=WireModuleParameters(segment_len=80.0 / (n_seg + 0.5)),
                  config=EnvironmentConfig(target_cutting_distance=5000.0))
        gpu, cpu = make_pair(n_envs, **kw)
        assert gpu.n_segments == n_seg

        def scenario(env):
            env.reset(seed=1000 + n_seg)
            close_gap(env, 21.0, 10.0)
            hot = env.state.wire_temperature
            hot[5, n_seg // 2] = 1600.0       # environment 5 breaks its wire at the first step: a frozen lane in its wave
            hot[70, n_seg - 1] = 900.0        # (in a wave without a frozen lane:) a hot last cell (Neumann end) ...
            hot[71, 1] = 900.0                # ... and a hot first interior cell
            return env.make_action(0.1, 80.0, 17, 3.0, 20.0)

        act = scenario(cpu)
        cpu.step_many(act, 290)
        for _ in range(10):
            cpu.step(act)
        want = cpu.state.clone_blocks()
        assert int(cpu.state.spark_count.sum()) > n_envs and bool(cpu.state.is_wire_broken[5])
        for variant in (3, 4, 6, 7):
            for lanes in (1, 2, 4, 8, 16):
                if (variant == 4 and lanes == 16) or (variant == 7 and lanes > 2):   # (the register kernel: one or two lanes per environment)
                    continue
                act = scenario(gpu)
                gpu.set_kernel(variant, lanes)
                try:
                    gpu.step_many(act, 290)
                    for _ in range(10):
                        gpu.step(act)
                except WedmError as exc:
                    assert "UNSUPPORTED" in str(exc)
                    refused += 1
                    continue
                torch.cuda.synchronize()
                diffs = block_diffs(gpu.state.clone_blocks(), want, n_envs)
                assert not diffs, f"n_seg {n_seg}, kernel {gpu._backend.last_kernel()}:\n" + "\n".join(diffs[:10])
                ran += 1
        gpu.close()
    assert ran >= 18 * 11 and refused <= 18 * 5, (ran, refused)   # (one lane per environment: wires over ~104 / 128 / ~159 cells do not fit)


@pytest.mark.parametrize("segment_len,expect", [(0.05, "wedm_step_fused<16>"), (0.02, "wedm_step_global")])
def test_very_long_wires_fall_back_to_a_kernel_that_fits(segment_len, expect):
    """1 600 segments (a chunk fits in LDS only at 16 lanes per environment) and 4 000 segments (no
    LDS kernel fits: multi-microsecond launches run the global-memory kernel); single steps take
    the split kernel.  All against the oracle."""
    n = 70
    kw = dict(wire_params=WireModuleParameters(segment_len=segment_len))
    gpu, cpu = make_pair(n, **kw)
    assert gpu.n_segments == round(80.0 / segment_len)
    both((gpu, cpu), lambda e: (e.reset(seed=6), close_gap(e)))
    for env in (gpu, cpu):
        act = env.make_action(0.1, 80.0, 9, 3.0, 30.0)
        env.step_many(act, 150)
    assert expect in gpu._backend.last_kernel()
    check(gpu, cpu, n)
    for env in (gpu, cpu):
        act = env.make_action(0.1, 80.0, 9, 3.0, 30.0)
        for _ in range(3):
            env.step(act)
    assert "wedm_step_split" in gpu._backend.last_kernel()
    check(gpu, cpu, n)
    assert int(gpu.state.spark_count.sum()) > 0


def test_single_environment_batch_follows_the_reference(golden_dir):
    """num_envs = 1 (the reference's own shape): fixture F3 env 0, whole trajectory through the
    device trace, fused launches."""
    from tests._fixture_env import env_from_fixture, run_fixture_through_trace
    from tests._golden import Fixture

    fx = Fixture(golden_dir / "f3_philox_env0.npz")
    env = env_from_fixture(fx, 1, device="cuda:0")
    got = run_fixture_through_trace(env, fx, exact_floats=False)
    assert (got["spark_state"] == 1).sum() > 10


@pytest.mark.parametrize("name", ["f17_second_episode_philox_env2", "f17_reset_during_short_philox_env4",
                                  "f17_stale_current_cache_philox_env5", "f18_past_target_philox_env1",
                                  "f18_past_wire_break_philox_env3", "f18_past_collision_philox_env6"])
def test_reference_compatible_reset_and_stepping_past_termination_on_gpu(golden_dir, name):
    """F17 / F18 (the reference's second episode on one environment object; `step()` after `terminated`) on the GPU:
    fused launches read back through the device trace -- discrete state, clocks, positions, voltage / current and the
    `terminated` flag exact at every microsecond, debris / flow <= 1e-12, temperatures <= 1e-4 K."""
    from tests._fixture_env import compat_env_from_fixture, run_fixture_through_trace
    from tests._golden import Fixture

    fx = Fixture(golden_dir / f"{name}.npz")
    env = compat_env_from_fixture(fx, 64, device="cuda:0")
    got = run_fixture_through_trace(env, fx, exact_floats=False)
    assert "wedm_step_" in env._backend.last_kernel()
    if name.startswith("f18"):
        first = int(np.argmax(fx.int_row("terminated") != 0))
        assert got["done"][first:].all() and not got["done"][:first].any() and fx.n_steps - first >= 500


@pytest.mark.parametrize("variant,lanes", KERNELS + [(0, 0)])
def test_compat_modes_every_kernel_matches_oracle(variant, lanes):
    """`reset_semantics="reference"` + `freeze_terminated=False` (+ in-launch autoreset with the reference's reset) on every
    kernel against the oracle batch, every byte: wire breaks by temperature and by collision, reached targets, stale current
    caches, running short timers, all stepped on past `terminated` and through several second episodes."""
    n = 160
    kw = dict(reset_semantics="reference", freeze_terminated=False, autoreset=variant in (0, 3, 4),
              ignition_params=IgnitionModuleParameters(default_current_mode="I13"),
              config=EnvironmentConfig(target_cutting_distance=5000.0))
    gpu, cpu = make_pair(n, **kw)
    gpu.set_kernel(variant, lanes)
    if (variant == 3 and (-(-gpu.n_segments // lanes) + 1) > 160) or (variant == 4 and (2 * -(-gpu.n_segments // (2 * lanes)) + 2) > 160):
        pytest.skip("chunk does not fit in 160 KB of LDS")
    idx = torch.arange(n)
    for env in (gpu, cpu):
        env.reset(seed=11)
        close_gap(env, 21.0, 10.0)
        env.state.workpiece_position = torch.where(idx % 9 == 2, 11.2, 21.0)          # hard shorts: timers running at the resets
        env.state.target_position = torch.where(idx % 4 == 1, 21.0005, 5000.0)        # reached after the first craters
        env.state.wire_position = torch.where(idx % 11 == 5, 125.0, 10.0)             # collision: wire > workpiece + 100
        hot = env.state.wire_temperature
        hot[7::13, 200:204] = 1600.0                                                  # breaks at the first step
        a = env.make_action(0.1, 80.0, 9, 3.0, 30.0)
        for k in ((1, 1, 1200, 1, 700) if variant in (5, 6) else (1, 1200, 1, 1, 700)):
            env.step_many(a, k)
        env.reset(seed=12, options={"mask": idx % 3 == 0})                             # a second episode for a third of them
        env.state.wire_position = torch.where(idx % 3 == 0, 35.0, env.state.wire_position.cpu())   # (15 um gap: sparks before the latch)
        for k in (1, 900, 1, 600):
            env.step_many(a, k)
    check(gpu, cpu, n)
    st = gpu.state
    assert bool(st.ignition_mode_cached.any()) and int(st.spark_count.sum()) > n
    if not kw["autoreset"]:   # (with in-launch autoreset the terminated ones have long been re-initialised)
        assert bool(st.is_wire_broken.any()) and bool(st.is_target_distance_reached.any())


def test_two_microsecond_physics_step_fixture_on_gpu(golden_dir):
    from tests._fixture_env import env_from_fixture, run_fixture_through_trace
    from tests._golden import Fixture

    fx = Fixture(golden_dir / "f13_dt2_philox_env4.npz")
    env = env_from_fixture(fx, 64, device="cuda:0")
    got = run_fixture_through_trace(env, fx, exact_floats=False)
    assert got["time"][:3].tolist() == [2, 4, 6]


@pytest.mark.parametrize("name", ["f20_dt3_gap_controller_philox_env5", "f20_dt7_schedule_velocity_philox_env6",
                                  "f20_dt3_voltage_controller_philox_env3"])
def test_off_grid_fixtures_on_gpu(golden_dir, name):
    """F20: dt = 3 / servo_interval = 100 and dt = 7 / servo_interval = 50 (latches at time_since_servo = 102 and 56), the
    recorded action rows handed to launches of at most one control interval."""
    from tests._fixture_env import env_from_fixture, run_fixture_through_trace
    from tests._golden import Fixture

    fx = Fixture(golden_dir / f"{name}.npz")
    env = env_from_fixture(fx, 64, device="cuda:0")
    got = run_fixture_through_trace(env, fx, exact_floats=False)
    steps = -(-env.servo_interval // env.dt)
    assert got["time"][:3].tolist() == [env.dt, 2 * env.dt, 3 * env.dt] and got["time_since_servo"].max() == steps * env.dt
    assert (got["spark_state"] == 1).sum() >= 15


def test_custom_wire_material_fixture_on_gpu(golden_dir):
    from tests._fixture_env import env_from_fixture, run_fixture_through_trace
    from tests._golden import Fixture

    fx = Fixture(golden_dir / "f14_copper_wire_philox_env6.npz")
    env = env_from_fixture(fx, 64, device="cuda:0")
    got = run_fixture_through_trace(env, fx, exact_floats=False)
    assert (got["spark_state"] == 1).sum() > 50


def test_default_modes_before_the_first_latch_fixture_on_gpu(golden_dir):
    from tests._fixture_env import env_from_fixture, run_fixture_through_trace
    from tests._golden import Fixture

    fx = Fixture(golden_dir / "f15_default_mode_philox_env7.npz")
    env = env_from_fixture(fx, 64, device="cuda:0")
    got = run_fixture_through_trace(env, fx, exact_floats=False)
    assert (got["spark_state"][:1000] == 1).sum() > 5


# ------------------------------------------------------------------ BASELINE configs[3] / configs[4] as the bench shards them
def test_config4_shard_of_rank_7_matches_oracle():
    """BASELINE configs[3] (262 144 environments over 8 GPUs) as rank 7 of 8 sees it: 32 768 environments x
    400 segments, env_id_offset = 7 * 32 768, the automatically selected kernel, two control intervals and a
    few single microseconds, against the CPU oracle on every byte."""
    n, rank = 32768, 7
    gpu, cpu = make_pair(n, env_id_offset=rank * n)
    both((gpu, cpu), lambda e: (e.reset(seed=1234), close_gap(e, 25.0, 10.0)))
    for env in (gpu, cpu):
        act = env.make_action(0.1, 80.0, 5, 3.0, 80.0)
        env.step_many(act, 1000)
        env.step_many(act, 1000)
    assert "wedm_step_served<8>" in gpu._backend.last_kernel(), gpu._backend.last_kernel()
    check(gpu, cpu, n)
    for env in (gpu, cpu):
        act = env.make_action(0.1, 80.0, 5, 3.0, 80.0)
        for _ in range(3):
            env.step(act)
    assert "wedm_step_split" in gpu._backend.last_kernel()
    check(gpu, cpu, n)
    assert int(gpu.state.spark_count.sum()) > 100000
    # the offset really is in the random streams: rank 0's first environments follow other trajectories
    other = WireEDMEnv(num_envs=256, device="cuda:0")
    other.reset(seed=1234)
    close_gap(other, 25.0, 10.0)
    other.step_many(other.make_action(0.1, 80.0, 5, 3.0, 80.0), 2003)
    assert not torch.equal(other.state.spark_count, gpu.state.spark_count[:256])


def test_config5_shard_of_rank_5_matches_oracle():
    """BASELINE configs[4] (131 072 environments, per-environment workpiece height / wire diameter / current
    mode from numpy.default_rng(2024)) as rank 5 of 8 sees it: its 16 384-environment slice of
    the global draws, env_id_offset = 5 * 16 384, the automatically selected kernel, two control intervals
    and a few single microseconds, against the CPU oracle on every byte."""
    import bench

    n, rank, world = 16384, 5, 8
    h, d, mode = bench.config5_draws(world * n, rank * n, (rank + 1) * n)
    kw = dict(workpiece_height=h, wire_diameter=d, env_id_offset=rank * n,
              config=EnvironmentConfig(target_cutting_distance=5000.0))
    gpu, cpu = make_pair(n, **kw)
    assert gpu.n_segments == cpu.n_segments and 440 <= gpu.n_segments <= 450
    both((gpu, cpu), lambda e: (e.reset(seed=1234), close_gap(e, 25.0, 10.0)))
    for env in (gpu, cpu):
        act = env.make_action(0.1, 80.0, mode, 3.0, 80.0)
        env.step_many(act, 1000)
        env.step_many(act, 1000)
    assert "wedm_step_lanes_" in gpu._backend.last_kernel(), gpu._backend.last_kernel()   # (the served or the packed form)
    check(gpu, cpu, n)
    for env in (gpu, cpu):
        act = env.make_action(0.1, 80.0, mode, 3.0, 80.0)
        for _ in range(3):
            env.step(act)
    check(gpu, cpu, n)
    assert int(gpu.state.spark_count.sum()) > 50000 and len(set(gpu._geom_i32[0, :n].cpu().tolist())) > 50


def _shards_in_turn_equal_one_batch(n_shard, world, make_env, action_of, T_rows_of=None):
    """BASELINE configs[3] / configs[4] at their OWN size on one GPU: the whole batch stepped as ONE environment object
    against its `world` shards stepped one after the other, each with `env_id_offset = r * n_shard` exactly as
    `bench.py --gpus 8` cuts them.  Every byte of every state block must agree (1 000 us fused + 3 single microseconds):
    results do not depend on how the batch is sharded, nor on the kernel / lane count the launch plan picks for a size."""
    n_all = n_shard * world
    full = make_env(n_all, 0, 0, n_all)
    full.reset(seed=1234)
    close_gap(full, 25.0, 10.0)
    act = action_of(full, 0, n_all)
    full.step_many(act, 1000)
    kernels = {full._backend.last_kernel()}
    for _ in range(3):
        full.step(act)
    torch.cuda.synchronize()
    want = full.state.clone_blocks()
    sparks = int(full.state.spark_count.sum())
    n_seg_full = full.n_segments
    full.close()
    del full
    for r in range(world):
        lo, hi = r * n_shard, (r + 1) * n_shard
        env = make_env(n_shard, r * n_shard, lo, hi)
        env.reset(seed=1234)
        close_gap(env, 25.0, 10.0)
        act = action_of(env, lo, hi)
        env.step_many(act, 1000)
        kernels.add(env._backend.last_kernel())
        for _ in range(3):
            env.step(act)
        torch.cuda.synchronize()
        got = env.state.clone_blocks()
        assert env.n_segments <= n_seg_full
        assert_blocks_equal(got, {k: v[:, lo:hi] for k, v in want.items()}, n_shard,
                            T_rows=(T_rows_of(env) if T_rows_of else None))
        env.close()
    return sparks, kernels


@pytest.mark.parametrize("stencil_dtype", ["float32", "float64"])
def test_config4_at_full_size_all_eight_shards_in_turn_equal_one_batch(stencil_dtype):
    """BASELINE configs[3]: 262 144 environments x 400 segments as ONE batch == its 8 shards of 32 768, in both typings of the
    stencil (float64: the wide register kernel at two blocks per CU)."""
    sparks, kernels = _shards_in_turn_equal_one_batch(
        32768, 8, lambda n, off, lo, hi: WireEDMEnv(num_envs=n, device="cuda:0", env_id_offset=off, stencil_dtype=stencil_dtype),
        lambda env, lo, hi: env.make_action(0.1, 80.0, 5, 3.0, 80.0))
    assert sparks > 400000, sparks
    assert any("<<<" in k for k in kernels)
    assert stencil_dtype == "float32" or all("[f64 stencil]" in k for k in kernels), kernels


@pytest.mark.parametrize("stencil_dtype", ["float32", "float64"])
def test_config5_at_full_size_all_eight_shards_in_turn_equal_one_batch(stencil_dtype):
    """BASELINE configs[4]: 131 072 environments with per-environment workpiece height / wire diameter / current mode
    (bench.config5_draws: numpy.default_rng(2024)) as ONE batch == its 8 shards of 16 384, in both typings of the
    stencil.  The full batch and the shards run different lane counts of the per-environment-geometry kernel (the plan follows
    the batch size)."""
    import bench

    world, n = 8, 16384
    H, D, M = bench.config5_draws(world * n, 0, world * n)

    def make_env(num, off, lo, hi):
        return WireEDMEnv(num_envs=num, device="cuda:0", env_id_offset=off, workpiece_height=H[lo:hi], wire_diameter=D[lo:hi],
                          stencil_dtype=stencil_dtype, config=EnvironmentConfig(target_cutting_distance=5000.0))

    sparks, kernels = _shards_in_turn_equal_one_batch(
        n, world, make_env, lambda env, lo, hi: env.make_action(0.1, 80.0, M[lo:hi], 3.0, 80.0),
        T_rows_of=lambda env: env.n_segments)
    assert sparks > 200000, sparks
    assert len(kernels) >= 2, kernels  # (wedm_step_lanes_pk<4> for the whole batch, <8> for a shard)


# ------------------------------------------------------------------ auto-reset / reward / voltage sum inside the launch
@pytest.mark.parametrize("variant,lanes", [(0, 0), (2, 4), (3, 8), (4, 4), (1, 0), (5, 0), (6, 8), (9, 8), (9, 4), (11, 8)])
def test_in_kernel_autoreset_and_reward_match_oracle_and_host_path(variant, lanes):
    """wedm_params.autoreset + reward_mode: environments that reach their cutting target are
    re-initialised by the NEXT launch itself (Philox episode + 1, fresh module state, spool-temperature wire,
    statistics cleared) and the launch writes the progress reward.  Three runs must agree on every byte, every
    control interval: the GPU with the in-kernel reset, the CPU oracle with the same mode, and the GPU driven
    the round-1 way (masked wedm_reset from the host + torch reward).  More than 30 % of the environments
    terminate inside a single launch."""
    from sparc_amd import WireEDMVectorEnv
    from tests.test_next_rows import run_autoreset_pair, terminating_pair

    n = 96
    a, b = terminating_pair(n, None, device="cuda:0")
    a.set_kernel(variant, lanes), b.set_kernel(variant, lanes)
    c_env, _ = terminating_pair(n, OracleBackend)
    vc = WireEDMVectorEnv(c_env)
    act_c = c_env.make_action(0.05, 80.0, 13, 2.0, 20.0)
    va, vb = WireEDMVectorEnv(a), WireEDMVectorEnv(b, reward="progress")
    act_a, act_b = a.make_action(0.05, 80.0, 13, 2.0, 20.0), b.make_action(0.05, 80.0, 13, 2.0, 20.0)
    most = 0.0
    for k in range(5):
        oa, ra, ta, ua, ia = va.step(act_a)
        ob, rb, tb, ub, ib = vb.step(act_b)
        oc, rc, tc, uc, ic = vc.step(act_c)
        torch.cuda.synchronize()
        assert torch.equal(ta, tb) and torch.equal(ta.cpu(), tc), k
        assert torch.equal(ra, rb) and torch.equal(ra.cpu(), rc), k
        A, B, Cc = a.state.clone_blocks(), b.state.clone_blocks(), c_env.state.clone_blocks()
        assert_blocks_equal(A, Cc, n)                                  # GPU == oracle, reward row included
        assert_blocks_equal(A, B, n, skip_rows=("reward",))            # in-kernel reset == host-driven reset
        most = max(most, float(ta.float().mean()))
    assert most >= 0.3 and int(a.state.episode.max()) >= 1
    assert va._in_kernel_reset and not vb._in_kernel_reset


def test_vector_env_step_is_one_launch_without_host_sync():
    """`WireEDMVectorEnv.step` on an autoreset environment: no `.item()` / device-to-host read.  Checked by
    running it under torch's sync debug mode, which raises on any synchronising call."""
    from sparc_amd import WireEDMVectorEnv

    env = WireEDMEnv(num_envs=4096, device="cuda:0", autoreset=True, reward="progress")
    vec = WireEDMVectorEnv(env, max_episode_steps=3000)
    vec.reset(seed=5)
    close_gap(env, 25.0, 10.0, 25.004)
    act = env.make_action(0.05, 80.0, 13, 2.0, 20.0)
    vec.step(act)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(4):
            obs, reward, term, trunc, info = vec.step(act)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert "wedm_step_" in env._backend.last_kernel()
    assert bool(term.any() | (env.state.episode > 0).any()) and reward.dtype == torch.float32
    assert info["time"].dtype == torch.int64 and torch.equal(info["time"], env.state.time)  # the exact clock, not a placeholder
    # ... and with what a policy really hands over (wire_edm.py:116-121,162-170): a FRESH dict of device tensors per control
    # step -- the servo command a torch function of the observation, the generator settings drawn on the device.  The
    # current modes are validated on the device (sticky ERROR row, `check_errors()`), not read back.
    valid = torch.tensor([1, 3, 5, 7, 9, 11, 13, 15, 17], dtype=torch.int32, device="cuda:0")
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(4):
            gap = obs[:, 0]
            action = {"servo": torch.clamp(0.02 * (gap - 12.0), -1.0, 1.0),
                      "generator_control": {"target_voltage": torch.full((4096,), 80.0, device="cuda:0"),
                                            "current_mode": valid[torch.randint(0, 9, (4096,), device="cuda:0", generator=gen)],
                                            "ON_time": torch.full((4096, 1), 2.0, device="cuda:0"),
                                            "OFF_time": torch.full((4096,), 20.0, device="cuda:0")}}
            obs, reward, term, trunc, info = vec.step(action)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    env.check_errors()                                                    # every mode was a valid one
    assert int(env.state.current_mode.unique().numel()) > 1             # the drawn modes were latched
    # an invalid mode in a device tensor: no exception at step() (nothing is read back), the sticky flag and a deferred raise
    bad = valid[torch.zeros(4096, dtype=torch.int64, device="cuda:0")].clone()
    bad[77] = 4
    action["generator_control"]["current_mode"] = bad
    vec.step(action)
    assert bool(env.state.error[77]) and int(env.state.error.sum()) == 1
    with pytest.raises(ValueError, match="environment 77"):
        env.check_errors()
    with pytest.raises(ValueError, match="I4 is not available"):      # host-side values still raise at once
        env.step_many(env.make_action(0.0, 80.0, 4, 2.0, 20.0), 1)


@pytest.mark.parametrize("name", ["f16_logger_philox_env3", "f16_logger_velocity_philox_env1"])
def test_reference_logger_fixture_on_gpu(golden_dir, name):
    """F16 on the GPU: the output of the reference's own `SimulationLogger` over its own driver loop and signal
    list (every_step / interval / control_step) against the build's logger fed by the in-kernel trace of fused
    launches.  Clocks, positions, voltages, currents, commands and flags exact; debris / flow (and
    `dielectric_flow_rate` with the reference's 1e-9 scaling) to 1e-12; temperatures to 1e-4 K."""
    from tests._fixture_env import run_logger_fixture

    assert run_logger_fixture(golden_dir / f"{name}.npz", device="cuda:0", exact=False) == 38


@pytest.mark.parametrize("name,n", [("f9_voltage_controller_dt2_philox_env4", 64), ("f9_voltage_controller_servo500_philox_env6", 64)])
def test_voltage_controller_sum_rows_on_gpu_follow_reference_fixtures(golden_dir, name, n):
    """The PI voltage controller fed by the kernel-side running voltage sum (rows VOLT_ACC / VOLT_SUM) in fused
    launches against the reference's own controller (fixtures F9b: 2-us physics step, 500-us servo interval):
    every float32 servo command the reference computed, exactly."""
    from sparc_amd import VoltageController
    from tests._fixture_env import env_from_fixture
    from tests._golden import Fixture

    fx = Fixture(golden_dir / (name + ".npz"))
    env_id = int(fx.meta["env_id"])
    env = env_from_fixture(fx, n, device="cuda:0")
    ctl = VoltageController(30.0)
    action = ctl(env)
    assert float(action.servo[env_id]) == fx.actions[fx.action_idx[0], 0]
    steps = -(-env.servo_interval // env.dt)
    done, k, checked = 0, steps + 1, 0
    while done + k <= fx.n_steps:
        env.step_many(action, k)       # one fused launch up to and including the next latch
        done += k
        action = ctl(env)
        if done < fx.n_steps:
            assert float(action.servo[env_id]) == fx.actions[fx.action_idx[done], 0], done
            checked += 1
        k = steps
    assert checked >= 4
    assert float(env.state.wire_position[env_id]) == float(fx.float_row("wire_position")[np.searchsorted(fx.float_steps, done - 1)]) \
        or (done - 1) not in fx.float_steps.tolist()


def test_environment_on_a_non_current_device_is_refused_by_the_abi_and_guarded_by_the_host():
    """a handle belongs to the device that was current at wedm_create.  With one GPU the guard can only
    be exercised through the C-ABI's own check: the status of a launch with the right device current is OK."""
    env = WireEDMEnv(num_envs=64, device="cuda:0")
    env.reset(seed=1)
    env.step(env.make_action())
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs to make another device current")
    other = WireEDMEnv(num_envs=64, device="cuda:1")   # current device stays cuda:0
    cpu = WireEDMEnv(num_envs=64, device="cpu", backend=OracleBackend)
    for e in (other, cpu):   # the second device's results against the oracle, every byte, both launch cadences
        e.reset(seed=1)
        close_gap(e, 22.0, 10.0)
        a = e.make_action(0.1, 80.0, 9, 3.0, 30.0)
        e.step_many(a, 1500)
        for _ in range(3):
            e.step(a)
    torch.cuda.synchronize("cuda:1")
    assert torch.cuda.current_device() == 0
    assert_blocks_equal(other.state.clone_blocks(), cpu.state.clone_blocks(), 64)
    assert int(other.state.time[0]) == 1503 and int(other.state.spark_count.sum()) > 0


# ------------------------------------------------------------------ the stencil as Numba types it (wedm_params.stencil_mode 1)
@pytest.mark.parametrize("shape", ["default400", "config3", "per_env"])
def test_float64_stencil_mode_matches_oracle_bit_for_bit(shape):
    """`stencil_dtype="float64"`: wire.py:58-123 with Numba's typing (float64 expressions, rounded at each float32
    store) on the device == the oracle's STENCIL_F64 restatement, every byte, fused and single-microsecond launches."""
    n = 160
    kw = dict(stencil_dtype="float64")
    if shape == "config3":
        kw["wire_params"] = WireModuleParameters(segment_len=0.625)
    if shape == "per_env":
        rng = np.random.default_rng(3)
        kw.update(workpiece_height=rng.uniform(10.0, 30.0, n), wire_diameter=rng.choice([0.1, 0.2, 0.3], n),
                  config=EnvironmentConfig(target_cutting_distance=5000.0))
    gpu, cpu = make_pair(n, **kw)
    both((gpu, cpu), lambda e: (e.reset(seed=77), close_gap(e, 24.0, 10.0)))
    # (kernel 3, the tile walk: uniform geometry; kernel 7, the register walk: at most 128 segments)
    # (kernel 2: the packed any-geometry walk with float64-typed cells; kernel 10: its cell-by-cell form)
    variants = ((0, 0), (2, 0), (2, 4), (2, 16), (10, 0), (1, 0)) if shape == "per_env" else ((0, 0), (3, 0), (2, 0), (10, 0), (1, 0))
    if shape == "config3":
        variants += ((7, 1), (7, 2), (8, 4))
    if shape == "default400":
        variants += ((8, 16),)
    for variant, lanes in variants:
        gpu.set_kernel(variant, lanes)
        for env in (gpu, cpu):
            a = env.make_action(0.1, 80.0, 17, 3.0, 40.0)
            env.step_many(a, 900)
            for _ in range(3):
                env.step(a)
        assert "[f64 stencil]" in gpu._backend.last_kernel()
        check(gpu, cpu, n)
    assert int(gpu.state.spark_count.sum()) > 100
    # a launch with trace samples (the TRACE instantiation of whatever the plan takes for this shape and typing)
    gpu.set_kernel(0, 0)
    gpu.bind_trace(["voltage"], every=7, capacity=64, wire_temperature=True)
    for env in (gpu, cpu):
        env.step_many(env.make_action(0.1, 80.0, 17, 3.0, 40.0), 300)
    assert "[f64 stencil]" in gpu._backend.last_kernel()
    check(gpu, cpu, n)
    gpu.unbind_trace()
    # and it really is another arithmetic: the float32 typing differs in the last bits of T
    f32 = WireEDMEnv(num_envs=n, device="cuda:0", **{k: v for k, v in kw.items() if k != "stencil_dtype"})
    f32.reset(seed=77)
    close_gap(f32, 24.0, 10.0)
    f32.step_many(f32.make_action(0.1, 80.0, 17, 3.0, 40.0), 903 * len(variants) + 300)
    d = (f32.state.T[:, :n] - gpu.state.T[:, :n]).abs().max().item()
    assert 0.0 < d < 1e-3
    from sparc_amd._lib import WedmError

    gpu.set_kernel(4, 0)   # no packed form of that typing
    with pytest.raises(WedmError, match="UNSUPPORTED"):
        gpu.step_many(gpu.make_action(), 10)


@pytest.mark.parametrize("env_id", [0, 777])
def test_float64_stencil_mode_stays_within_the_stated_tolerance_of_the_reference(golden_dir, env_id):
    """The reference as users run it (real Numba: float64 intermediates) differs from the reference as it runs
    without Numba (float32 promotion, what the fixtures recorded) by at most 1.3e-4 K over these horizons
    (SURVEY.md §8c); on the GPU: fixture F3 replayed with the float64 stencil — discrete state and positions
    exact, temperatures within 1.3e-4 K."""
    from tests._fixture_env import env_from_fixture, run_fixture_through_trace
    from tests._golden import Fixture

    fx = Fixture(golden_dir / f"f3_philox_env{env_id}.npz")
    env = env_from_fixture(fx, env_id + 64, device="cuda:0", stencil_dtype="float64")
    got = run_fixture_through_trace(env, fx, exact_floats=False, T_atol=1.3e-4)
    assert (got["spark_state"] == 1).sum() > 10 and "[f64 stencil]" in env._backend.last_kernel()


def test_native_seed_reference_run_followed_on_the_gpu(golden_dir):
    """Fixture F1 = BASELINE configs[0], the reference's OWN NumPy PCG64 stream (reset(seed=0), 10 000 us,
    SURVEY.md §8c known answers).  The device consumes the reference's recorded draws through the variate-injection
    mode (wedm_bind_rng_replay) and must follow the reference step by step: discrete state, clocks, positions,
    voltage / current exact, debris / flow to 1e-12, temperatures to 1e-4 K, read back through the in-kernel trace."""
    from tests._fixture_env import env_from_fixture, run_fixture_through_trace
    from tests._golden import Fixture, replay_table

    fx = Fixture(golden_dir / "f1_config1_native.npz")
    env = env_from_fixture(fx, 64, device="cuda:0")
    env.bind_rng_replay(replay_table(fx))
    fx.meta["env_id"] = 5                       # any environment: all consume the same variates
    got = run_fixture_through_trace(env, fx, exact_floats=False)
    assert "[injected variates]" in env._backend.last_kernel()
    assert (got["spark_state"] == 1).sum() == 36 and (got["spark_state"] == -2).sum() == 960
    st = env.state
    assert float(st.workpiece_position[5]) == float(fx.float_row("workpiece_position")[-1])
    assert float(st.wire_position[5]) == float(fx.float_row("wire_position")[-1]) and int(st.spark_count[5]) == 12
    assert not bool(st.error.any())
    env.bind_rng_replay(None)
    env.step_many(env.make_action(), 10)
    assert any(k in env._backend.last_kernel() for k in ("wedm_step_packed", "wedm_step_fused", "wedm_step_regs_wide"))


def test_densely_sparking_batch_on_the_packed_kernel_matches_oracle():
    """The packed kernel's wave-uniform fast path also carries burning / ending sparks (quiet_prelude_t<true>): a densely
    sparking 128-segment batch with mixed current modes and ON times against the oracle, every byte."""
    n = 2048
    kw = dict(wire_params=WireModuleParameters(segment_len=0.625))
    gpu, cpu = make_pair(n, **kw)
    both((gpu, cpu), lambda e: (e.reset(seed=606), close_gap(e, 18.0, 10.0)))
    rng = np.random.default_rng(1)
    modes = rng.choice([5, 9, 13, 17], n).astype(np.int32)
    on = rng.choice([1.0, 2.0, 3.5, 5.0], n)
    gpu.set_kernel(4, 2)
    for env in (gpu, cpu):
        a = env.make_action(0.05, 80.0, modes, on, 15.0)
        for k in (1000, 1000, 777):
            env.step_many(a, k)
    assert "wedm_step_packed<2>" in gpu._backend.last_kernel(), gpu._backend.last_kernel()
    check(gpu, cpu, n)
    assert int(gpu.state.spark_count.sum()) / n / 2.777 > 5.0          # densely sparking indeed


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("mode", ["default", "autoreset", "reference"])
def test_register_kernel_one_environment_per_lane_matches_oracle(mode, lanes):
    """Kernel 7 (the whole wire of an environment in the registers of its one or two lanes, no LDS) at the headline grid (128 segments)
    against the oracle batch, every byte: sparks in every tile of the workpiece zone (plasma cell recomputed inside its
    tile), current through the contact tile, wire breaks by temperature (frozen lanes inside live waves) and by
    collision, reached targets; launches of 1, 2, 1000 and 1300 us; in-launch autoreset with the progress reward; the
    reference's reset semantics with stepping past `terminated`; a batch that does not fill its last wave."""
    n = 333
    kw = dict(wire_params=WireModuleParameters(segment_len=0.625), config=EnvironmentConfig(target_cutting_distance=5000.0))
    if mode == "autoreset":
        kw.update(autoreset=True, reward="progress", crater_log_capacity=8)
    if mode == "reference":
        kw.update(reset_semantics="reference", freeze_terminated=False, ignition_params=IgnitionModuleParameters(default_current_mode="I13"))
    gpu, cpu = make_pair(n, **kw)
    assert gpu.n_segments == 128
    gpu.set_kernel(7, lanes)
    idx = torch.arange(n)
    for env in (gpu, cpu):
        env.reset(seed=77)
        close_gap(env, 21.0, 10.0)
        env.state.workpiece_position = torch.where(idx % 9 == 2, 11.2, 21.0)          # hard shorts
        env.state.target_position = torch.where(idx % 4 == 1, 21.0005, 5000.0)        # reached after the first craters
        env.state.wire_position = torch.where(idx % 11 == 5, 125.0, 10.0)             # collision: wire > workpiece + 100
        hot = env.state.wire_temperature
        hot[7::13, 60:64] = 1600.0                                                    # breaks at the first step
        hot[70, 127] = 900.0                                                          # a hot last cell (Neumann end)
        hot[71, 1] = 900.0                                                            # a hot first interior cell
        a = env.make_action(0.1, 80.0, 17, 3.0, 20.0)
        for k in (1, 2, 1000, 1, 1300):
            env.step_many(a, k)
        env.reset(seed=78, options={"mask": idx % 3 == 0})
        env.state.wire_position = torch.where(idx % 3 == 0, 35.0, env.state.wire_position.cpu())
        env.state.wire_unwinding_velocity[::7] = 0.0                                  # mixed advection inside a wave
        for k in (1, 900, 600):
            env.step_many(a, k)
    assert f"wedm_step_regs<{lanes}>" in gpu._backend.last_kernel()
    check(gpu, cpu, n)
    st = gpu.state
    assert int(st.spark_count.sum()) > 10 * n
    if mode == "default":
        assert bool(st.is_wire_broken.any()) and bool(st.is_target_distance_reached.any())
    if mode == "autoreset":
        assert int(st.episode.max()) >= 1
    if mode == "autoreset":
        return   # (the oracle seam samples a trace after single microseconds, and every launch boundary is an episode boundary here)
    # a launch with a trace sample runs the register kernel's TRACE instantiation (round 4), results unchanged
    traces = [e.bind_trace(["voltage", "wire_max_temperature"], every=1, capacity=64, envs=(0, 64)) for e in (gpu, cpu)]
    for env in (gpu, cpu):
        env.step_many(env.make_action(0.1, 80.0, 17, 3.0, 20.0), 40)
    assert "wedm_step_regs<" in gpu._backend.last_kernel()
    assert_rings_equal(*traces)
    check(gpu, cpu, n)


@pytest.mark.parametrize("mode", ["default", "autoreset", "reference"])
def test_wide_register_kernel_on_the_default_grid_matches_oracle(mode):
    """Kernel 8 (16 lanes per environment, 32 cells each in registers, no LDS, no walk table) on the default grid --
    400 segments: lane 12 holds the wire's last 16 cells and 16 cells of padding, lanes 13..15 padding only; the zone
    starts inside a tile (cell 149), the contacts at cells 100 and 300 -- against the oracle batch, every byte: sparks
    in every tile of the zone (plasma cell recomputed inside its tile), current between the contacts, wire breaks by
    temperature (frozen lanes inside live waves) and by collision, reached targets; launches of 1, 2, 1000 and 1300 us;
    in-launch autoreset with the progress reward; the reference's reset semantics with stepping past `terminated`; a
    batch that does not fill its last block."""
    n = 333
    kw = dict(config=EnvironmentConfig(target_cutting_distance=5000.0))
    if mode == "autoreset":
        kw.update(autoreset=True, reward="progress", crater_log_capacity=8)
    if mode == "reference":
        kw.update(reset_semantics="reference", freeze_terminated=False, ignition_params=IgnitionModuleParameters(default_current_mode="I13"))
    gpu, cpu = make_pair(n, **kw)
    assert gpu.n_segments == 400
    idx = torch.arange(n)
    for env in (gpu, cpu):
        env.reset(seed=77)
        close_gap(env, 21.0, 10.0)
        env.state.workpiece_position = torch.where(idx % 9 == 2, 11.2, 21.0)          # hard shorts
        env.state.target_position = torch.where(idx % 4 == 1, 21.0005, 5000.0)        # reached after the first craters
        env.state.wire_position = torch.where(idx % 11 == 5, 125.0, 10.0)             # collision: wire > workpiece + 100
        hot = env.state.wire_temperature
        hot[7::13, 190:194] = 1600.0                                                  # breaks at the first step
        hot[70, 399] = 900.0                                                          # a hot last cell (Neumann end)
        hot[71, 1] = 900.0                                                            # a hot first interior cell
        hot[72, 383:386] = 700.0                                                      # across the lanes 11 | 12
        a = env.make_action(0.1, 80.0, 17, 3.0, 20.0)
        for k in (1, 2, 1000, 1, 1300):
            env.step_many(a, k)
        env.reset(seed=78, options={"mask": idx % 3 == 0})
        env.state.wire_position = torch.where(idx % 3 == 0, 35.0, env.state.wire_position.cpu())
        env.state.wire_unwinding_velocity[::7] = 0.0                                  # mixed advection inside a wave
        for k in (2, 900, 600):
            env.step_many(a, k)
    assert "wedm_step_regs_wide<16>" in gpu._backend.last_kernel()                    # (chosen by itself for fused launches)
    check(gpu, cpu, n)
    st = gpu.state
    assert int(st.spark_count.sum()) > 10 * n
    if mode == "default":
        assert bool(st.is_wire_broken.any()) and bool(st.is_target_distance_reached.any())
    if mode == "autoreset":
        assert int(st.episode.max()) >= 1
        return   # (the oracle seam samples a trace after single microseconds, and every launch boundary is an episode boundary here)
    # a launch with a trace sample: the instantiation with the trace point, wire temperature included
    traces = [e.bind_trace(["voltage", "wire_max_temperature"], every=1, capacity=64, envs=(0, 64), wire_temperature=True) for e in (gpu, cpu)]
    for env in (gpu, cpu):
        env.step_many(env.make_action(0.1, 80.0, 17, 3.0, 20.0), 40)
    assert "wedm_step_regs_wide<16>" in gpu._backend.last_kernel()
    assert_rings_equal(*traces)
    check(gpu, cpu, n)


WIDE_N = [9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 128, 200, 255, 256, 257, 264, 300, 383, 384, 385, 390, 392, 396, 399,
          401, 408, 415, 416, 417, 440, 448, 479, 480, 481, 496, 504, 511, 512]


@pytest.mark.parametrize("part", [0, 1, 2])
def test_wide_register_kernel_over_wire_lengths(part):
    """Kernel 8 forced over wire lengths from 9 to 512 segments: the wire's end at every kind of place -- closing a
    tile (n_seg a multiple of 8: the last cell patched inside a regular tile, in chunk A or chunk B of its lane),
    cutting one (the predicated per-cell code for that tile index in every lane), at a lane's first cell, at the last
    cell of the last lane (512) -- zone and contact indices wherever the geometry puts them; sparks, current, a wire
    break (frozen lanes in a live wave), hot end cells; fused launches and single microseconds."""
    n_envs = 96
    for n_seg in WIDE_N[part::3]:
        kw = dict(wire_params=WireModuleParameters(segment_len=80.0 / (n_seg + 0.5)),
                  config=EnvironmentConfig(target_cutting_distance=5000.0))
        gpu, cpu = make_pair(n_envs, **kw)
        assert gpu.n_segments == n_seg
        fewest = 4 if n_seg <= 128 else 8 if n_seg <= 256 else 16      # lanes per environment: 32 cells each

        def scenario(env):
            env.reset(seed=1000 + n_seg)
            close_gap(env, 21.0, 10.0)
            hot = env.state.wire_temperature
            hot[5, n_seg // 2] = 1600.0       # environment 5 breaks its wire at the first step: frozen lanes in its wave
            hot[70, n_seg - 1] = 900.0        # a hot last cell (Neumann end) ...
            hot[71, 1] = 900.0                # ... and a hot first interior cell
            act = env.make_action(0.1, 80.0, 17, 3.0, 20.0)
            env.step_many(act, 290)
            for _ in range(6):
                env.step(act)

        scenario(cpu)
        assert int(cpu.state.spark_count.sum()) > n_envs and bool(cpu.state.is_wire_broken[5])
        want = cpu.state.clone_blocks()
        for lanes in sorted({0, fewest, 16}):                           # 0: the fewest lanes that hold the wire
            gpu.set_kernel(8, lanes)
            scenario(gpu)
            torch.cuda.synchronize()
            assert f"wedm_step_regs_wide<{lanes or fewest}>" in gpu._backend.last_kernel()
            diffs = block_diffs(gpu.state.clone_blocks(), want, n_envs)
            assert not diffs, f"n_seg {n_seg}, kernel {gpu._backend.last_kernel()}:\n" + "\n".join(diffs[:10])
        if fewest > 4:
            from sparc_amd._lib import WedmError
            gpu.set_kernel(8, 4)                                        # too few lanes for this wire
            with pytest.raises(WedmError, match="UNSUPPORTED"):
                gpu.step_many(gpu.make_action(), 2)
        gpu.close()


def test_wide_register_kernel_is_the_choice_for_small_batches_of_the_headline_grid():
    """128 segments: 4 lanes per environment hold the wire; a batch that one round of blocks covers takes the wide register
    kernel by itself (a larger one the two-lane register kernel or the LDS kernels); against the oracle, dense sparking."""
    n = 3000
    kw = dict(wire_params=WireModuleParameters(segment_len=0.625))
    gpu, cpu = make_pair(n, **kw)
    both((gpu, cpu), lambda e: (e.reset(seed=606), close_gap(e, 18.0, 10.0)))
    rng = np.random.default_rng(1)
    modes = rng.choice([5, 9, 13, 17], n).astype(np.int32)
    on = rng.choice([1.0, 2.0, 3.5, 5.0], n)
    for env in (gpu, cpu):
        a = env.make_action(0.05, 80.0, modes, on, 15.0)
        for k in (1000, 777):
            env.step_many(a, k)
    assert "wedm_step_regs_wide<4>" in gpu._backend.last_kernel(), gpu._backend.last_kernel()
    check(gpu, cpu, n)
    assert int(gpu.state.spark_count.sum()) / n / 1.777 > 5.0          # densely sparking indeed
    big = WireEDMEnv(num_envs=20000, device="cuda:0", **kw)
    big.reset(seed=1)
    big.step_many(big.make_action(), 10)
    assert "wedm_step_regs_wide" not in big._backend.last_kernel()


def test_wide_register_kernel_config2_batch_densely_sparking_matches_oracle():
    """The bench's config-2 batch (4 096 x 400, the automatic choice) with mixed current modes and ON times at a small gap:
    general preludes, Joule terms on most steps and plasma cells in every lane of the zone, every byte."""
    n = 4096
    gpu, cpu = make_pair(n)
    both((gpu, cpu), lambda e: (e.reset(seed=606), close_gap(e, 18.0, 10.0)))
    rng = np.random.default_rng(1)
    modes = rng.choice([5, 9, 13, 17], n).astype(np.int32)
    on = rng.choice([1.0, 2.0, 3.5, 5.0], n)
    for env in (gpu, cpu):
        a = env.make_action(0.05, 80.0, modes, on, 15.0)
        for k in (1000, 777):
            env.step_many(a, k)
    assert "wedm_step_regs_wide<16>" in gpu._backend.last_kernel(), gpu._backend.last_kernel()
    check(gpu, cpu, n)
    assert int(gpu.state.spark_count.sum()) / n / 1.777 > 5.0          # densely sparking indeed


@pytest.mark.parametrize("segment_len", [0.2, 0.625])
def test_negative_plasma_heat_every_kernel_matches_oracle(segment_len):
    """A negative plasma efficiency makes the plasma heat negative: the plasma cell's true temperature then lies BELOW
    the interior formula's result, so a kernel that patches the cell after its walk must keep the regular value out
    of the running maximum (the LDS and two-lane register kernels walk such a wave on the predicated formula; the
    wide register kernel patches before it takes the maximum).  Densely sparking, hot wire: Tmax, the critical-time
    counter and every cell against the oracle, every kernel that accepts the shape."""
    from sparc_amd._lib import WedmError

    n = 200
    kw = dict(wire_params=WireModuleParameters(segment_len=segment_len, plasma_efficiency=-0.2),
              config=EnvironmentConfig(target_cutting_distance=5000.0))
    gpu, cpu = make_pair(n, **kw)
    ran = 0
    for variant, lanes in KERNELS + [(0, 0), (7, 0), (8, 0)] + SERVED + SERVED_ANY:
        gpu.set_kernel(variant, lanes)
        for env in (gpu, cpu):
            env.reset(seed=515)
            close_gap(env, 18.0, 10.0)
        try:
            gpu.step_many(gpu.make_action(0.05, 80.0, 17, 3.0, 15.0), 700)
            gpu.step(gpu.make_action(0.05, 80.0, 17, 3.0, 15.0))
        except WedmError as exc:
            assert "UNSUPPORTED" in str(exc)
            continue
        cpu.step_many(cpu.make_action(0.05, 80.0, 17, 3.0, 15.0), 701)
        torch.cuda.synchronize()
        diffs = block_diffs(gpu.state.clone_blocks(), cpu.state.clone_blocks(), n)
        assert not diffs, f"kernel {gpu._backend.last_kernel()}:\n" + "\n".join(diffs[:10])
        ran += 1
    assert ran >= 8 and int(cpu.state.spark_count.sum()) > 5 * n
    T = cpu.state.wire_temperature
    assert float(T.tensor().min()) < 293.0                      # cells cooled below the spool temperature by the negative heat


# ------------------------------------------------------------------ the automatic launch plan
PLAN_POINTS = [(4096, 128), (16384, 128), (20480, 128), (32768, 128), (65536, 128), (4096, 200), (16384, 200), (8192, 256),
               (32768, 256), (2048, 400), (4096, 400), (8192, 400), (16384, 400), (32768, 400)]


@pytest.mark.parametrize("n,n_seg", PLAN_POINTS)
def test_automatic_plan_is_within_reach_of_the_best_forced_kernel(n, n_seg):
    """`wedm_step`'s automatic kernel choice against every forced variant that accepts the shape (tools/plan_sweep.py;
    the whole grid is recorded in profiles/r4/plan_sweep.txt): the plan's thresholds were fitted on single boxes, and a
    cliff between two of them -- 16 384 / 20 480 x 128, 4 096 / 8 192 x 400 -- would otherwise go unnoticed.  Median of
    three fused launches per kernel; 7 % of slack (5 % asked + launch-to-launch noise of a 2-ms kernel)."""
    import sys

    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
    import plan_sweep

    r = plan_sweep.sweep_point(n, n_seg)
    (ams, aname), (bms, bname, bkey) = r["auto"], r["best"]
    assert ams <= 1.07 * bms, f"{n} x {n_seg}: auto {aname} {ams:.3f} ms, forced {bname} {bkey} {bms:.3f} ms"


@pytest.mark.parametrize("n,n_seg", [(65536, 128), (16384, 128), (4096, 400), (32768, 400), (16384, 200)])
def test_automatic_plan_in_the_float64_typing_is_within_reach_of_the_best_forced_kernel(n, n_seg):
    """The same for `stencil_dtype="float64"` (kernels 3, 7, 8: profiles/r4/plan_sweep_f64.txt)."""
    import sys

    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
    import plan_sweep

    r = plan_sweep.sweep_point(n, n_seg, stencil_dtype="float64")
    (ams, aname), (bms, bname, bkey) = r["auto"], r["best"]
    assert ams <= 1.07 * bms, f"{n} x {n_seg}: auto {aname} {ams:.3f} ms, forced {bname} {bkey} {bms:.3f} ms"
