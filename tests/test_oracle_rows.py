"""The CPU oracle's per-environment physics rows and pulse tally (`wedm_oracle_step_batch_ex`, the oracle side of
wedm_bind_env_params / wedm_bind_pulse_stats in include/wedm_hip.h) against references that do not use them.

Rows: every environment of a batch with its own draw of all 15 randomisable parameters equals, on every byte, a
one-environment run whose dataclasses hold that draw (same seed, ``env_id_offset = e``).  Rows holding the uniform values
change nothing.  Pulse: the published rows, the accumulators and the observation's columns 8-10 equal the Python
definition (`tally`, and the reference driver's formula `reference_counts`) applied to a per-step trace of the same run,
across launch lengths that cut control intervals, resets, frozen and keep-stepping environments.  These tests make the
oracle the checker of the kernels' ENVP and PULSE forms (tests/test_env_params_fuzz.py)."""
from __future__ import annotations

import zlib

import numpy as np
import pytest
import torch

from sparc_amd import EnvironmentConfig, WireEDMEnv, WireModuleParameters, _abi
from sparc_amd.core import env_params as envp
from tests import _envp_draw as D
from tests._compare import block_diffs
from tests._oracle_backend import OracleBackend, OracleBackendRows
from tests.test_pulse_stats import reference_counts, tally

N = 24
SEED = 4242
LAUNCHES = (1000, 7, 1300, 1, 400)


def _config(**kw):
    return EnvironmentConfig(target_cutting_distance=5000.0, **kw)


# mode -> (WireEDMEnv keywords, extras)
MODES = {
    "position": ({}, {}),
    "velocity": (dict(mechanics_control_mode="velocity"), {}),
    "dt2": (dict(config=_config(dt=2)), {}),
    "servo200": (dict(config=_config(servo_interval=200)), {}),
    "servo1000_short_wire": (dict(wire_params=WireModuleParameters(segment_len=0.625)), {}),
    "per_env_geometry": ({}, dict(geometry=True)),
    "autoreset_crater_log": (dict(autoreset=True, reward="progress", crater_log_capacity=8), dict(terminate=True)),
    "reference_keep_stepping": (dict(reset_semantics="reference", freeze_terminated=False),
                                dict(terminate=True, masked_reset=True)),
    "stencil_f64": (dict(stencil_dtype="float64"), {}),
}


def _start(rng, n):
    gaps = np.where(rng.random(n) < 0.5, rng.uniform(0.5, 5.0, n), rng.uniform(5.0, 30.0, n))
    debris = np.where(rng.random(n) < 0.3, rng.uniform(0.0, 0.2, n), rng.uniform(0.0, 0.01, n))
    return gaps, debris


def _prepare(env, lo, hi, gaps, debris, terminate):
    env.reset(seed=SEED)
    idx = np.arange(lo, hi)
    env.state.wire_position = 10.0
    env.state.workpiece_position = torch.as_tensor(10.0 + gaps[lo:hi])
    env.state.debris_volume = torch.as_tensor(debris[lo:hi])
    if terminate:  # three environments in five sit right before their cutting targets
        env.state.target_position = torch.as_tensor(np.where(idx % 5 < 3, 10.0 + gaps[lo:hi] + 0.001, 5000.0))
    else:
        env.state.target_position = 5000.0


def _cols(blocks, e, nq=None):
    out = {k: v[:, e:e + 1] for k, v in blocks.items()}
    if nq is not None:
        out["T"] = out["T"][:nq]
    return out


def _run_rows_mode(mode, values, *, backend=OracleBackendRows, with_rows=True):
    kw, extra = MODES[mode]
    rng = np.random.default_rng(17)
    gaps, debris = _start(rng, N)
    velocity = kw.get("mechanics_control_mode") == "velocity"
    servo = rng.uniform(50, 300, N) if velocity else rng.uniform(-0.05, 0.3, N) * rng.choice([1.0, 1.0, 20.0, -3.0], N)
    modes = rng.choice([1, 5, 9, 13, 15, 17], N).astype(np.int32)
    geom = {}
    if extra.get("geometry"):
        geom = dict(workpiece_height=rng.uniform(8, 32, N), wire_diameter=rng.choice([0.1, 0.15, 0.25], N))
    terminate, masked_reset = extra.get("terminate", False), extra.get("masked_reset", False)
    mask = np.arange(N) % 3 == 1

    def drive(env, lo, hi):
        _prepare(env, lo, hi, gaps, debris, terminate)
        a = env.make_action(servo[lo:hi], 80.0, modes[lo:hi], 2.0, 25.0)
        for i, k in enumerate(LAUNCHES):
            if masked_reset and i == 2:
                env.reset(options={"mask": mask[lo:hi]})
            env.step_many(a, k)
        return env.state.clone_blocks()

    batch_kw = dict(kw, **geom)
    if with_rows:
        batch_kw["env_params"] = values
    batch = WireEDMEnv(num_envs=N, device="cpu", backend=backend, **batch_kw)
    got = drive(batch, 0, N)
    return got, batch, drive, kw, geom


@pytest.mark.parametrize("mode", list(MODES))
def test_rows_equal_one_environment_uniform_runs(mode):
    """Environment e of the batch (its own draw of every name) == a one-environment run built from that draw's
    dataclasses, env_id_offset = e, same seed: every block, the crater log included."""
    values = D.draw(np.random.default_rng(zlib.crc32(mode.encode())), N)
    D.spread_ok(values)
    got, batch, drive, kw, geom = _run_rows_mode(mode, values)
    extra = MODES[mode][1]
    assert batch._backend.last_kernel() == "oracle[envp]"
    for e in range(N):
        ekw = dict(kw)
        base = {k: ekw.pop(k) for k in list(ekw) if k in D.CLS}
        ekw.update(D.uniform_kw(D.column(values, e), base))
        if geom:
            ekw.update(workpiece_height=geom["workpiece_height"][e:e + 1], wire_diameter=geom["wire_diameter"][e:e + 1])
        one = WireEDMEnv(num_envs=1, device="cpu", backend=OracleBackend, env_id_offset=e, **ekw)
        want = drive(one, e, e + 1)
        nq = want["T"].shape[0]
        diffs = block_diffs(_cols(got, e, nq), _cols(want, 0), 1)
        assert not diffs, f"{mode}: environment {e}:\n" + "\n".join(diffs[:12])
        if "crater_log" in want:
            assert torch.equal(got["crater_log"][:, e], want["crater_log"][:, 0]), (mode, e)
    episodes = int(got["i32"][_abi.I32.EPISODE, :N].sum())
    if kw.get("autoreset"):  # the in-launch autoreset took the environments that reached their targets (and their counts)
        assert episodes >= 3, episodes
    else:
        assert int(got["i32"][_abi.I32.SPARK_COUNT, :N].sum()) > 50
    if extra.get("terminate") and not kw.get("autoreset"):
        assert bool(got["i8"][_abi.I8.TARGET_REACHED, :N].any())


@pytest.mark.parametrize("mode", ["position", "velocity", "dt2", "per_env_geometry", "autoreset_crater_log"])
def test_rows_holding_the_uniform_values_change_nothing(mode):
    uni = envp.uniform_values(WireEDMEnv(num_envs=1, device="cpu", backend=OracleBackend, **MODES[mode][0]))
    with_rows, b1, *_ = _run_rows_mode(mode, {n: np.full(N, v) for n, v in uni.items()})
    plain, b2, *_ = _run_rows_mode(mode, None, backend=OracleBackend, with_rows=False)
    assert b1._backend.last_kernel() == "oracle[envp]" and b2._backend.last_kernel() == "oracle"
    diffs = block_diffs(with_rows, plain, N)
    assert not diffs, "\n".join(diffs[:12])


def test_rows_are_read_at_every_launch():
    """`set_env_params` between launches (masked) takes effect at the next launch: the changed environments follow a
    one-environment run of the new values from the copied state."""
    values = D.draw(np.random.default_rng(5), N)
    env = WireEDMEnv(num_envs=N, device="cpu", backend=OracleBackendRows, env_params=values)
    rng = np.random.default_rng(17)
    gaps, debris = _start(rng, N)
    _prepare(env, 0, N, gaps, debris, False)
    a = env.make_action(0.1, 80.0, 9, 2.0, 25.0)
    env.step_many(a, 700)
    mid = env.state.clone_blocks()
    new = D.draw(np.random.default_rng(6), N)
    new["omega_n"] = D.omega_26bit(new["omega_n"])
    mask = np.arange(N) % 2 == 0
    env.set_env_params({k: torch.from_numpy(v) for k, v in new.items()}, mask=torch.from_numpy(mask))
    env.step_many(a, 1300)
    got = env.state.clone_blocks()
    for e in range(N):
        vals = D.column(new if mask[e] else values, e)
        one = WireEDMEnv(num_envs=1, device="cpu", backend=OracleBackend, env_id_offset=e, **D.uniform_kw(vals),
                         config=_config())
        one.reset(seed=SEED)
        blocks = one.state.clone_blocks()
        for k in ("f64", "i32", "i8", "T", "obs", "stats", "reward"):
            blocks[k][:, 0] = mid[k][:, e]  # environment e's state after the first launch
        one.state.load_blocks(blocks)
        one.step_many(one.make_action(0.1, 80.0, 9, 2.0, 25.0), 1300)
        diffs = block_diffs(_cols(got, e), _cols(one.state.clone_blocks(), 0), 1)
        assert not diffs, f"environment {e}:\n" + "\n".join(diffs[:12])


# ------------------------------------------------------------------------------------------------------------ pulse
PULSE_SCENARIOS = {
    # name: (WireEDMEnv keywords, launch lengths, masked reset before launch i (or None))
    "servo1000": (dict(config=_config()), (1, 7, 400, 1300, 1000, 7, 1, 1300), 4),
    "servo200": (dict(config=_config(servo_interval=200)), (1300, 7, 1, 400, 7, 1300), 3),
    "servo500_dt2": (dict(config=_config(servo_interval=500, dt=2)), (7, 400, 1, 1300, 400), 2),
    "velocity": (dict(config=_config(), mechanics_control_mode="velocity"), (400, 1300, 7, 1000), None),
    "autoreset": (dict(config=_config(servo_interval=500), autoreset=True), (400, 1300, 7, 400, 1, 1300), 3),
    "keep_stepping_reference": (dict(config=_config(), freeze_terminated=False, reset_semantics="reference"),
                                (1300, 400, 7, 1300), 2),
}


def _pulse_start(env, gaps):
    env.reset(seed=SEED)
    env.state.wire_position = 10.0
    env.state.workpiece_position = torch.as_tensor(10.0 + gaps)
    # every 4th environment right before its cutting target: terminations (frozen, stepped on, or reset in the launch)
    env.state.target_position = torch.as_tensor(np.where(np.arange(len(gaps)) % 4 == 1, 10.0 + gaps + 0.004, 5000.0))


@pytest.mark.parametrize("name", list(PULSE_SCENARIOS))
def test_pulse_rows_equal_the_definition_on_a_per_step_trace(name):
    kw, launches, reset_at = PULSE_SCENARIOS[name]
    n = N
    gaps = np.linspace(0.4, 15.0, n)  # a hard short to an idle 15 um: every kind of pulse
    env = WireEDMEnv(num_envs=n, device="cpu", backend=OracleBackendRows, pulse_stats=True, **kw)
    # the trace: the same run in launches of one microsecond, without the tally; the in-launch autoreset as the masked
    # reset it is defined to be (wedm_params.autoreset), at the same launch boundaries
    ref = WireEDMEnv(num_envs=n, device="cpu", backend=OracleBackend, **dict(kw, autoreset=False))
    keep = not kw.get("freeze_terminated", True)
    servo = np.where(np.arange(n) % 3 == 0, 0.2, 0.0) if kw.get("mechanics_control_mode") != "velocity" else 120.0
    acts = []
    for x in (env, ref):
        _pulse_start(x, gaps)
        acts.append(x.make_action(servo, 80.0, 9, 3.0, 30.0))
    segs = [[[]] for _ in range(n)]  # per environment: the samples since each reset
    mask = torch.from_numpy(np.arange(n) % 3 == 2)
    resets = 0
    for i, k in enumerate(launches):
        if i == reset_at:
            for x in (env, ref):
                x.reset(options={"mask": mask})
            for e in np.nonzero(mask.numpy())[0]:
                segs[e].append([])
        if kw.get("autoreset"):
            done = ref.state.done.clone()
            if bool(done.any()):
                ref.reset(options={"mask": done})
                resets += int(done.sum())
                for e in np.nonzero(done.numpy())[0]:
                    segs[e].append([])
        env.step_many(acts[0], k)
        for _ in range(k):
            ran = keep | ~ref.state.done.numpy().astype(bool)
            ref.step_many(acts[1], 1)
            cur, sh = ref.state.current.numpy(), ref.state.is_short_circuit.numpy()
            ctrl = ref.state.control_step.numpy()
            for e in np.nonzero(ran)[0]:
                segs[e][-1].append((float(cur[e]), bool(sh[e]), bool(ctrl[e])))
        # after every launch: the two runs are the same trajectory, and the rows hold what the definition gives
        g, w = env.state.clone_blocks(), ref.state.clone_blocks()
        g["obs"], w["obs"] = g["obs"][:8], w["obs"][:8]
        g.pop("reward"), w.pop("reward")
        diffs = block_diffs(g, w, n)
        assert not diffs, "\n".join(diffs[:12])
        want, totals = _expected(segs, n)
        got = env.state.pulse[:, :n].numpy()
        assert np.array_equal(got, want), (name, i, k, np.argwhere(got != want)[:8])
        assert np.array_equal(env.state.obs[8:11, :n].numpy(), want[3:6].astype(np.float32)), (name, i, k)
    assert env._backend.last_kernel() == "oracle[pulse]"
    assert totals[0] > 20 and totals[1] > 0 and totals[2] > 0, totals
    assert want[3:6].sum() > 0
    if kw.get("autoreset"):
        assert resets > 0
    if not keep and not kw.get("autoreset"):
        assert bool(ref.state.done.any())  # some environments sat frozen


def _expected(segs, n):
    """The six rows per environment from its samples since its last reset (`tally`), and the run's totals; on every
    stretch between two resets the published and running counts add up to the reference driver's formula."""
    want = np.zeros((_abi.PULSE_COUNT, n), dtype=np.int32)
    totals = np.zeros(3, dtype=np.int64)
    for e in range(n):
        for j, seg in enumerate(segs[e]):
            cur, sh = np.array([s[0] for s in seg]), np.array([s[1] for s in seg], dtype=bool)
            published, rest = tally(cur, sh, [s[2] for s in seg])
            r_short, r_spark = reference_counts(np.r_[0.0, cur], np.r_[False, sh])  # (the reset state in front)
            assert (sum(p[0] for p in published) + rest[0], sum(p[1] for p in published) + rest[1]) == (r_spark, r_short)
            totals += np.array([r_spark, r_short, int(sh.sum())])
            if j == len(segs[e]) - 1:
                want[0:3, e] = rest
                want[3:6, e] = published[-1] if published else (0, 0, 0)
    return want, totals


def test_pulse_rows_are_cleared_by_a_reset_and_survive_a_plain_backend_refusal():
    env = WireEDMEnv(num_envs=8, device="cpu", backend=OracleBackendRows, pulse_stats=True, config=_config())
    _pulse_start(env, np.linspace(0.4, 15.0, 8))
    env.step_many(env.make_action(0.0, 80.0, 9, 3.0, 30.0), 2100)
    assert int(env.state.pulse[_abi.PULSE.SPARK_LAST, :8].sum()) > 0
    mask = torch.tensor([True, False] * 4)
    before = env.state.pulse[:, :8].clone()
    env.reset(options={"mask": mask})
    assert int(env.state.pulse[:, :8][:, mask].abs().sum()) == 0
    assert torch.equal(env.state.pulse[:, :8][:, ~mask], before[:, ~mask])
    for kw in (dict(pulse_stats=True), dict(env_params={"zeta": 0.5})):
        with pytest.raises(ValueError, match="backend"):
            WireEDMEnv(num_envs=4, device="cpu", backend=OracleBackend, **kw)


def test_batch_seam_with_injected_variates_follows_the_reference_recording(golden_dir):
    """The oracle side of wedm_bind_rng_replay (`wedm_oracle_step_batch_replay`: the table read by step and slot, as the
    kernels read it) against the reference's own run: with the recorded NumPy PCG64 draws of fixture F1 as the table, every
    environment of a batch equals the recording, ints at every checked step and floats wherever the fixture holds them, bit
    for bit in the libm math mode.  This makes the oracle the checker of kernel 1's REPLAY forms
    (tests/test_registry_coverage.py)."""
    from oracle import oracle as orc
    from tests._fixture_env import check_step, env_from_fixture
    from tests._golden import Fixture, replay_table

    class LibmRows(OracleBackendRows):
        math_mode = orc.MATH_LIBM
        n_threads = 1

    fx = Fixture(golden_dir / "f1_config1_native.npz")
    env = env_from_fixture(fx, 3, device="cpu", backend=LibmRows)
    env.bind_rng_replay(replay_table(fx))
    servo, tv, on, off, mode = fx.actions[0]
    act = env.make_action(servo, tv, int(mode), on, off)
    assert len(fx.actions) == 1 and int(fx.int_row("spark_state").max()) > 0
    step = -1
    for us in [1] + [7] * ((fx.n_steps - 1) // 7) + [(fx.n_steps - 1) % 7]:   # (the fixture holds the floats of steps 0, 7, 14, ...)
        if us:
            env.step_many(act, us)
            step += us
            for e in range(3):
                check_step(env, fx, e, step, exact_floats=True)
    assert step == fx.n_steps - 1 and env._backend.last_kernel() == "oracle[injected variates]"
    assert not bool(env.state.error.any())
    T = env.state.wire_temperature.numpy()[:, : fx.T_snaps.shape[1]]
    assert all(np.array_equal(T[e], fx.T_snaps[-1]) for e in range(3))
