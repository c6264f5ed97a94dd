"""SURVEY.md §8f rows built on top of the path: on-device controller + driver loop, the
vector/auto-reset adapter, the signal logger and the module statistics.  CPU tests use the
oracle test seam in LIBM math mode, which is bit-identical to the reference."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from sparc_amd import (EnvironmentConfig, GapController, SimulationLogger, WireEDMEnv, WireEDMVectorEnv, run_controlled)
from tests._fixture_env import check_step
from tests._golden import Fixture
from tests._oracle_backend import OracleBackend


class LibmOracleBackend(OracleBackend):
    math_mode = orc.MATH_LIBM  # glibc pow/exp like the reference -> bit-exact against its fixtures


def driver_env(n, seed, mode="position", backend=LibmOracleBackend, device="cpu"):
    env = WireEDMEnv(num_envs=n, device=device, backend=backend, mechanics_control_mode=mode)
    env.reset(seed=seed)
    env.state.workpiece_position = 70.0   # experiments/run_simulation.py:199-201
    env.state.wire_position = 10.0
    env.state.target_position = 5000.0
    return env


@pytest.mark.parametrize("name,seed,mode,env_ids,n", [
    ("f7_gap_controller_philox_env%d", 77, "position", (0, 9), 16),
    ("f7_gap_controller_velocity_philox_env%d", 78, "velocity", (3,), 8),
])
def test_gap_controller_reproduces_the_reference_driver(golden_dir, name, seed, mode, env_ids, n):
    """run_simulation.py's loop (controller recomputed after every control step) with the
    on-device GapController, one microsecond per call: every recorded quantity of the reference
    is reproduced exactly."""
    fxs = {i: Fixture(golden_dir / ((name % i) + ".npz")) for i in env_ids}
    env = driver_env(n, seed, mode)
    ctl = GapController()
    action = ctl(env)
    steps = min(f.n_steps for f in fxs.values())
    for step in range(steps):
        env.step(action)
        for i, fx in fxs.items():
            check_step(env, fx, i, step, exact_floats=True)
        if bool(env.state.control_step[0]):
            action = ctl(env)
            for i, fx in fxs.items():  # the action the reference computed at this control step
                row = fx.actions[fx.action_idx[min(step + 1, steps - 1)]]
                assert float(action.servo[i]) == row[0] and int(action.current_mode[i]) == int(row[4])
    for i, fx in fxs.items():
        assert np.array_equal(env.state.wire_temperature[i].numpy(), fx.T_snaps[-1]) or steps < fx.n_steps


def test_run_controlled_fused_launches_equal_per_microsecond_driver():
    a, b = driver_env(8, 5), driver_env(8, 5)
    ctl_a, ctl_b = GapController(), GapController()
    calls = []
    n = run_controlled(a, ctl_a, 4300, on_control_step=lambda env, t: calls.append(t))
    assert n == 4300 and calls == [1001, 2001, 3001, 4001]
    action = ctl_b(b)
    for _ in range(4300):
        b.step(action)
        if bool(b.state.control_step[0]):
            action = ctl_b(b)
    A, B = a.state.clone_blocks(), b.state.clone_blocks()
    for k in ("i32", "i8", "T", "obs"):
        assert torch.equal(A[k], B[k]), k
    assert bool(((A["f64"] == B["f64"]) | (A["f64"].isnan() & B["f64"].isnan())).all())


def test_vector_env_autoreset():
    env = WireEDMEnv(num_envs=6, device="cpu", backend=OracleBackend)
    vec = WireEDMVectorEnv(env)
    obs, info = vec.reset(seed=3)
    assert obs.shape == (6, 8)
    env.state.workpiece_position = 25.0
    env.state.wire_position = 10.0
    env.state.target_position[:3] = 25.0005    # the first craters finish these three
    act = env.make_action()
    terminated_seen = torch.zeros(6, dtype=torch.bool)
    for _ in range(4):
        obs, reward, terminated, truncated, info = vec.step(act)
        terminated_seen |= terminated
        assert reward.shape == (6,) and not truncated.any()
    assert terminated_seen[:3].all() and not terminated_seen[3:].any()
    assert (vec.episode_count[:3] >= 1).all() and (vec.episode_count[3:] == 0).all()
    assert (env.state.episode[:3] >= 1).all()            # fresh Philox stream per episode
    assert (env.state.time[3:] == 4000).all() and (env.state.time[:3] < 4000).all()
    vec2 = WireEDMVectorEnv(WireEDMEnv(num_envs=2, device="cpu", backend=OracleBackend), max_episode_steps=2000)
    vec2.reset(seed=1)
    a2 = vec2.env.make_action()
    _, _, term, trunc, _ = vec2.step(a2)
    assert not trunc.any()
    _, _, term, trunc, _ = vec2.step(a2)
    assert trunc.all() and not term.any()
    vec2.step(a2)
    assert (vec2.env.state.time == 1000).all()           # reset happened before the third interval


def test_vector_env_progress_reward():
    env = WireEDMEnv(num_envs=5, device="cpu", backend=OracleBackend)
    vec = WireEDMVectorEnv(env, reward="progress")
    vec.reset(seed=4)
    env.state.workpiece_position = 24.0
    env.state.wire_position = 10.0
    env.state.target_position = 5000.0
    act = env.make_action(0.05, 80.0, 13, 2.0, 20.0)
    total = torch.zeros(5)
    for _ in range(3):
        _, reward, *_ = vec.step(act)
        assert reward.dtype == torch.float32 and reward.shape == (5,)
        total += reward
    cut = (env.state.workpiece_position - 24.0).to(torch.float32)
    assert torch.allclose(total, cut, atol=1e-5) and bool((cut > 0).all())          # micrometres of material removed
    plain = WireEDMVectorEnv(WireEDMEnv(num_envs=2, device="cpu", backend=OracleBackend))
    plain.reset(seed=1)
    assert float(plain.step(plain.env.make_action())[1].abs().sum()) == 0.0          # the reference's constant 0.0
    custom = WireEDMVectorEnv(env, reward=lambda e, prev: e.state.voltage.to(torch.float32))
    assert torch.equal(custom.step(act)[1], env.state.voltage.to(torch.float32))
    with pytest.raises(ValueError):
        WireEDMVectorEnv(env, reward="nope")


def test_signal_logger_frequencies_and_npz(tmp_path):
    env = driver_env(4, 9, backend=OracleBackend)
    cfg = {"signals_to_log": ["time", "voltage", "wire_position", "spark_status", "wire_temperature"],
           "log_frequency": {"type": "control_step"},
           "backend": {"type": "numpy", "filepath": str(tmp_path / "log.npz"), "compress": True}}
    logger = SimulationLogger(cfg, env_reference=env)
    run_controlled(env, GapController(), 3500, on_control_step=lambda e, t: logger.collect(e.state, control_step=True))
    logger.finalize()
    data = logger.get_data()
    assert data["time"].shape == (3, 4) and data["time"][:, 0].tolist() == [1001, 2001, 3001]
    assert data["wire_temperature"].shape == (3, 4, env.n_segments)
    z = np.load(tmp_path / "log.npz")
    assert np.array_equal(z["wire_position"], data["wire_position"])
    every = SimulationLogger({"signals_to_log": ["time"], "log_frequency": {"type": "interval", "value": 2}})
    for _ in range(6):
        env.step(env.make_action())
        every.collect(env.state)
    assert every.get_data()["time"].shape == (3, 4)
    with pytest.raises(ValueError):
        SimulationLogger({"log_frequency": {"type": "sometimes"}})


def test_module_statistics_helpers():
    env = WireEDMEnv(num_envs=4, device="cpu", backend=OracleBackend)
    env.reset(seed=2)
    env.state.workpiece_position = 11.0   # gap < 2 um -> debris short for 50 us
    env.state.wire_position = 10.0
    env.step_many(env.make_action(servo=-0.5), 10)
    sc = env.get_short_circuit_status()
    assert sc["has_debris_short"].all() and (sc["debris_short_remaining_us"] == 41).all()
    assert (sc["total_short_remaining_us"] == 41).all() and not sc["has_random_short"].any()
    deb = env.get_debris_statistics()
    assert set(deb) == {"debris_volume_mm3", "debris_density", "cavity_volume_mm3", "flow_condition", "debris_fill_percentage"}
    assert (env.get_crater_count() == 0).all()
    assert env.zone_mean_temperature().shape == (4,)


def test_checkpoint_resume_is_bit_identical(tmp_path):
    a = driver_env(6, 21, backend=OracleBackend)
    a.state.workpiece_position = 24.0
    act = a.make_action(0.1, 80.0, 9, 3.0, 40.0)
    a.step_many(act, 1700)
    a.save_checkpoint(tmp_path / "ck.pt")
    a.step_many(act, 1500)
    b = WireEDMEnv(num_envs=6, device="cpu", backend=OracleBackend)
    b.reset(seed=999)                         # different key: everything must come from the checkpoint
    b.load_checkpoint(tmp_path / "ck.pt")
    b.step_many(b.make_action(0.1, 80.0, 9, 3.0, 40.0), 1500)
    A, B = a.state.clone_blocks(), b.state.clone_blocks()
    for k in A:
        same = (A[k] == B[k]) | ((A[k] != A[k]) & (B[k] != B[k])) if A[k].is_floating_point() else (A[k] == B[k])
        assert bool(same.all()), k
    assert int(a.state.spark_count.sum()) > 20
    assert b.steps_since_reset == a.steps_since_reset == 3200
    with pytest.raises(ValueError):
        WireEDMEnv(num_envs=5, device="cpu", backend=OracleBackend).load_checkpoint(tmp_path / "ck.pt")
    # same shape, different physics (control mode / a module parameter): refused instead of silently diverging
    from sparc_amd import MechanicsModuleParameters

    with pytest.raises(ValueError, match="different physics"):
        WireEDMEnv(num_envs=6, device="cpu", backend=OracleBackend,
                   mechanics_control_mode="velocity").load_checkpoint(tmp_path / "ck.pt")
    with pytest.raises(ValueError, match="different physics"):
        WireEDMEnv(num_envs=6, device="cpu", backend=OracleBackend,
                   mechanics_params=MechanicsModuleParameters(zeta=0.5)).load_checkpoint(tmp_path / "ck.pt")


def test_the_clock_is_64_bit_and_no_launch_count_limits_a_run():
    """`state.time` is an unbounded Python int in the reference (wire_edm.py:135).  Here: low 32 bits in the row the
    kernels carry (also the Philox counter word) + a high word bumped when the low word wraps inside a launch, so an
    environment's own clock stays exact past 2**31 and 2**32 us, and nothing counts LAUNCHES: an autoreset batch can be
    stepped for ever (round 2 raised OverflowError after 2**31 cumulated microseconds, i.e. ~2.9 h of training, although
    every environment's own clock had been reset thousands of times)."""
    env = WireEDMEnv(num_envs=3, device="cpu", backend=OracleBackend, autoreset=True,
                     config=EnvironmentConfig(target_cutting_distance=5000.0))
    env.reset(seed=1)
    act = env.make_action()
    env.step_many(act, 10)
    env.steps_since_reset = 2**31 - 1 - 5          # as if ~35.8 simulated minutes of launches had been cumulated
    env.step_many(act, 700)                         # no OverflowError
    assert env.state.time.tolist() == [710, 710, 710] and env.state.time.dtype == torch.int64
    # per-environment clocks across the sign bit and across the 32-bit wrap, against a twin that never comes near them
    twin = WireEDMEnv(num_envs=3, device="cpu", backend=OracleBackend, autoreset=True,
                      config=EnvironmentConfig(target_cutting_distance=5000.0))
    twin.reset(seed=1)
    twin.step_many(act, 710)
    env.state.time = torch.tensor([2**31 - 300, 2**32 - 300, 3 * 2**32 - 1])
    env.state.time_since_open_voltage = env.state.time
    assert env.state.time.tolist() == [2**31 - 300, 2**32 - 300, 3 * 2**32 - 1]
    for k in (1, 299, 1, 1500, 1):
        env.step_many(act, k)
        twin.step_many(act, k)
    assert env.state.time.tolist() == [2**31 + 1502, 2**32 + 1502, 3 * 2**32 + 1801]
    assert env.state.time_since_open_voltage.tolist() == env.state.time.tolist()
    assert env.state.time_high32.tolist() == [0, 1, 3] and twin.state.time.tolist() == [2512] * 3
    # the physics does not read the clock; only the variates do (Philox counter word = low 32 bits), so positions differ
    # from the twin's while every invariant of the step holds
    assert (env.state.time_since_servo == twin.state.time_since_servo).all()
    # assignment through the wide attribute round-trips
    env.state.time = 5
    assert env.state.time.tolist() == [5, 5, 5] and env.state.time_high32.tolist() == [0, 0, 0]
    # `time_since_open_voltage` is stored as a 32-bit row next to `time`'s 64 bits: its exact value is composed from the
    # constant distance between the two clocks, not from `time`'s high word (the two low words wrap at different moments)
    env.state.time_since_open_voltage = 0
    env.state.time = 2**32 - 100
    assert env.state.time_since_open_voltage.tolist() == [0, 0, 0]          # assigning `time` leaves the other clock alone
    env.step_many(act, 300)
    assert env.state.time.tolist() == [2**32 + 200] * 3
    assert env.state.time_since_open_voltage.tolist() == [300] * 3            # the reference's value (was 2**32 + 300)
    env.state.time_since_open_voltage = 2**32 + 7                             # assigning it leaves `time` alone
    assert env.state.time.tolist() == [2**32 + 200] * 3 and env.state.time_since_open_voltage.tolist() == [2**32 + 7] * 3
    with pytest.raises(ValueError, match="time_since_open_voltage"):          # further than 32 bits from `time`: refused, loudly
        env.state.time_since_open_voltage = 7
    # one launch may not span 2**31 us (the high word is carried per launch)
    long_dt = WireEDMEnv(num_envs=1, device="cpu", backend=OracleBackend, config=EnvironmentConfig(dt=4, servo_interval=1000))
    with pytest.raises(ValueError, match="2\\*\\*31"):
        long_dt.step_many(long_dt.make_action(), 2**29)


def test_a_launch_of_2_to_the_31_microseconds_is_refused_in_steps_of_dt():
    """The limit is on n_substeps * dt, not on n_substeps: at dt = 7 the first refused launch is one of ceil(2**31 / 7)
    steps, and the one a step shorter reaches the backend."""
    env = WireEDMEnv(num_envs=2, device="cpu", backend=OracleBackend, config=EnvironmentConfig(dt=7, servo_interval=50))
    env.reset(seed=1)
    act = env.make_action()
    first_refused = -(-2**31 // 7)
    assert (first_refused - 1) * 7 < 2**31 <= first_refused * 7 and first_refused < 2**31 // 4
    for n in (first_refused, first_refused + 1, 2**31 // 4):
        with pytest.raises(ValueError) as exc:
            env.step_many(act, n)
        assert str(exc.value) == f"one launch may advance an environment by less than 2**31 us (asked: {n} x 7 us)"
    assert env.steps_since_reset == 0 and env.state.time.tolist() == [0, 0]      # a refused launch leaves everything as it was
    asked = []
    env._backend.step = lambda n, ptrs: asked.append(n)                           # (not run: 2**31 us of oracle steps)
    env.step_many(act, first_refused - 1)
    assert asked == [first_refused - 1]


def terminating_pair(n, backend, device="cpu", **kw):
    """Two identical batches whose environments reach their cutting target at different moments."""
    envs = []
    for in_kernel in (True, False):
        env = WireEDMEnv(num_envs=n, device=device, backend=backend, env_id_offset=1000,
                         **(dict(autoreset=True, reward="progress") if in_kernel else {}), **kw)
        env.reset(seed=31)
        env.state.workpiece_position = 25.0
        env.state.wire_position = 10.0
        env.state.target_position = 25.0 + torch.linspace(0.0005, 0.03, n, dtype=torch.float64)
        envs.append(env)
    return envs


def run_autoreset_pair(a, b, intervals=6, min_fraction=0.3):
    """`a` resets inside the launch (wedm_params.autoreset, reward written by the kernel), `b` is driven
    the round-1 way: a masked reset launch from the host + a torch reward.  Everything must agree."""
    from tests._compare import assert_blocks_equal

    va, vb = WireEDMVectorEnv(a), WireEDMVectorEnv(b, reward="progress")
    assert va._in_kernel_reset and not vb._in_kernel_reset
    act_a, act_b = a.make_action(0.05, 80.0, 13, 2.0, 20.0), b.make_action(0.05, 80.0, 13, 2.0, 20.0)
    seen = torch.zeros(a.num_envs, dtype=torch.bool)
    most = 0.0
    for k in range(intervals):
        oa, ra, ta, ua, ia = va.step(act_a)
        ob, rb, tb, ub, ib = vb.step(act_b)
        assert torch.equal(ta.cpu(), tb.cpu()) and torch.equal(ua.cpu(), ub.cpu()), k
        assert torch.equal(ra.cpu(), rb.cpu()) and ra.dtype == torch.float32, k
        assert torch.equal(oa.cpu(), ob.cpu()), k
        assert torch.equal(ia["episode"].cpu(), ib["episode"].cpu()), k
        assert_blocks_equal(a.state.clone_blocks(), b.state.clone_blocks(), a.num_envs, skip_rows=("reward",))
        seen |= ta.cpu()
        most = max(most, float(ta.float().mean()))
    assert most >= min_fraction, most                     # a large share terminates inside one launch
    assert bool(seen.all()) or float(seen.float().mean()) > 0.6
    assert int(a.state.episode.max()) >= 1 and int(a.state.time.min()) < 1000 * intervals
    return va, vb


def test_in_kernel_autoreset_and_reward_equal_the_host_driven_path():
    a, b = terminating_pair(48, OracleBackend)
    run_autoreset_pair(a, b)


def test_in_kernel_autoreset_with_truncation():
    a = WireEDMEnv(num_envs=6, device="cpu", backend=OracleBackend, autoreset=True)
    b = WireEDMEnv(num_envs=6, device="cpu", backend=OracleBackend)
    va, vb = WireEDMVectorEnv(a, max_episode_steps=2000), WireEDMVectorEnv(b, max_episode_steps=2000)
    va.reset(seed=3), vb.reset(seed=3)
    act_a, act_b = a.make_action(), b.make_action()
    for k in range(5):
        ra, rb = va.step(act_a), vb.step(act_b)
        assert torch.equal(ra[2], rb[2]) and torch.equal(ra[3], rb[3]), k
        assert torch.equal(a.state.time, b.state.time) and torch.equal(a.state.episode, b.state.episode), k
    assert a.state.time.tolist() == [1000] * 6 and a.state.episode.tolist() == [2] * 6
    with pytest.raises(ValueError):
        WireEDMVectorEnv(a, autoreset=False)
