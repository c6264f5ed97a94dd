"""Every registered instantiation of a step kernel, once, against the CPU oracle on a real MI355X.

One test per kernel family runs that family's recipes of tests/_registry_catalogue.py.  A recipe is a handle (forced kernel and
lane count, bindings, wire length) and a sequence of launches; after every launch the test reads which instantiation ran
(`last_form()`: wedm_debug_last_form), asserts that it is the one the recipe expected, and compares every block -- the pulse
and signal blocks where bound, the trace ring where a trace is bound -- bit for bit with the oracle's half of the same
launches.  Each test ends with: reached == the family's registry entries - UNREACHABLE.

The scenario is the one of tests/test_packed_walk.py: 100 environments (every family's last block is partly dead), a gap that
sparks, environment 5 breaks its wire at the first step, a hot last cell and a hot first interior cell.  The only other
batches are the float64 wide forms at two blocks per CU (more than 65 536 lanes).  The injected-variates forms of kernel 1 run
the same scenario and launches: both sides read one table of variates drawn per environment (wedm_bind_rng_replay), by step
and slot, so the environments take different courses and every block is compared like everywhere else.

On the default grid (g0: dt 1, servo_interval 1000) the 597 steps of a handle end before the first control step.  The same
recipes therefore run again on g1 (dt 1, servo_interval 100) and g2 (dt 3, servo_interval 100: `time_since_servo` steps
from 99 to 102), the environments starting at staggered points of the control interval and every launch offering a new
action per environment: the latch, the rows published at control steps (VOLT_SUM, the pulse and signal *_LAST rows), the
observation and the reward of a control step are then compared in every instantiation and in every launch, the launches
of a single step included.  The oracle half asserts that the control steps are really there (`_reference`)."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from sparc_amd import EnvironmentConfig, WireEDMEnv, WireModuleParameters, _abi, _lib
from sparc_amd.core.tables import VALID_CRATER_MODES
from tests import _envp_draw
from tests import _registry_catalogue as cat
from tests._compare import assert_blocks_equal
from tests._oracle_backend import OracleBackend, OracleBackendRows
from tests._signal_oracle import SignalOracleBackend
from tests._wmat_draw import BRASS, COPPER

pytestmark = pytest.mark.gpu

K, F = _abi.KERNEL, _abi.FORM
MATERIALS = (BRASS, COPPER)
TINY_ROLLS = 7   # the environment whose injected debris rolls are tiny


def _kw(n_seg, n_envs, bind, autoreset, grid="g0"):
    dt, interval = cat.GRIDS[grid]
    kw = dict(wire_params=WireModuleParameters(segment_len=80.0 / (n_seg + 0.5)),
              config=EnvironmentConfig(target_cutting_distance=5000.0) if grid == "g0" else
              EnvironmentConfig(target_cutting_distance=5000.0, dt=dt, servo_interval=interval))
    if "f64" in bind:
        kw["stencil_dtype"] = "float64"
    if "pulse" in bind:
        kw["pulse_stats"] = True
    if "sig" in bind:
        kw["signal_stats"] = True
    if "envp" in bind:
        kw["env_params"] = _envp_draw.draw(np.random.default_rng(11), n_envs)
    if "wmat" in bind:  # (environment 5, whose wire breaks at 1600 K, is of brass)
        kw["wire_material"] = [MATERIALS[(k + 1) % 2] for k in range(n_envs)]
    if autoreset:
        kw["autoreset"] = True
    return kw


def _make(device, n_seg, n_envs, bind, autoreset, grid="g0"):
    kw = _kw(n_seg, n_envs, bind, autoreset, grid)
    if device == "cpu":
        kw["backend"] = SignalOracleBackend if "sig" in bind else OracleBackendRows if bind & {"pulse", "envp", "wmat", "replay"} else OracleBackend
    env = WireEDMEnv(num_envs=n_envs, device=device, **kw)
    assert env.n_segments == n_seg and (env.dt, env.servo_interval) == cat.GRIDS[grid]
    if "replay" in bind:
        env.bind_rng_replay(_variates(n_envs, float(env.config.workpiece_height)))
    return env


@functools.lru_cache(maxsize=None)
def _variates(n_envs, height):
    """float64[REPLAY_STEPS, 5, n_envs]: per step and environment the three rolls in [0, 1), a spark location in [0, height)
    and a crater volume in um^3 (the slots of `_abi.REPLAY_SLOTS`), every slot filled whether the step draws it or not."""
    rng = np.random.default_rng(23)
    t = rng.uniform(0.0, 1.0, (cat.REPLAY_STEPS, _abi.REPLAY_SLOTS, n_envs))
    t[:, 3] = rng.uniform(0.0, height, (cat.REPLAY_STEPS, n_envs))
    t[:, 4] = rng.uniform(500.0, 5000.0, (cat.REPLAY_STEPS, n_envs))
    # a native NumPy uniform can be arbitrarily small, and the kernel's injected-variates form alone evaluates the debris
    # sigmoid for exponents of 24 to 500 (a Philox uniform is at least 2^-33): environment TINY_ROLLS rolls 1e-10 ... 1e-300
    t[:, 0, TINY_ROLLS] = 10.0 ** -rng.uniform(10.0, 300.0, cat.REPLAY_STEPS)
    return t


def _scenario(env, n_seg):
    env.reset(seed=1000 + n_seg)
    env.state.workpiece_position = 21.0
    env.state.wire_position = 10.0
    env.state.target_position = 5000.0
    hot = env.state.wire_temperature
    hot[5, n_seg // 2] = 1600.0       # environment 5 breaks its wire at the first step: a frozen lane in its wave
    hot[70, n_seg - 1] = 900.0        # a hot last cell (Neumann end) ...
    hot[71, 1] = 900.0                # ... and a hot first interior cell
    return env.make_action(0.1, 80.0, 17, 3.0, 20.0)


def _stagger(env, grid, seq):
    """g1, g2: after the reset every environment is at its own point of the control interval (cat.stagger)."""
    tss = torch.tensor(cat.stagger(grid, seq, env.num_envs), dtype=torch.int32)
    interval = cat.GRIDS[grid][1]
    assert int(tss.min()) >= 0 and bool((tss == interval).any()) and bool((tss < interval).any())
    env.state.time_since_servo = tss
    return tss


def _launch_action(env, grid, act, index):
    """The action of launch number `index`: the scenario's one action on g0, on g1 and g2 a new one per launch that
    differs per environment in every leaf (cat.action_leaves)."""
    if grid == "g0":
        return act
    return env.make_action(*(np.asarray(leaf) for leaf in cat.action_leaves(VALID_CRATER_MODES, index, env.num_envs)))


def _snapshot(env, trace):
    blocks = env.state.clone_blocks()
    ring = {k: v.detach().cpu().clone() for k, v in trace.read().items()} if trace is not None else None
    return blocks, ring, (trace.count if trace is not None else 0)


def _assert_latched_late(env, grid, bind):
    """After a handle's last launch on g1 / g2: the latched rows are no longer what launch 0 offered in more than half of
    the environments, and the rows published at control steps are alive."""
    st, n = env.state, env.num_envs
    first = cat.action_leaves(VALID_CRATER_MODES, 0, n)
    rows = (st.target_delta, st.target_voltage, st.current_mode, st.ON_time, st.OFF_time)
    for name, row, offered in zip(("target_delta", "target_voltage", "current_mode", "ON_time", "OFF_time"), rows, first):
        moved = int((row.to(torch.float64) != torch.tensor(offered, dtype=torch.float64)).sum())
        assert moved > n // 2, f"{grid}: {name} still holds launch 0's value in {n - moved} of {n} environments"
    assert bool((st.voltage_sum_at_control_step != 0).any())
    blocks = st.clone_blocks()
    if "pulse" in bind:
        last = blocks["pulse"][int(_abi.PULSE.SPARK_LAST):int(_abi.PULSE.SHORT_STEPS_LAST) + 1, :n]
        assert any(bool((r != 0).any()) and len(set(r.tolist())) > 1 for r in last), f"{grid}: no published pulse row is alive"
    if "sig" in bind:
        last = blocks["signal"][int(_abi.SIG.SAMPLES_LAST):int(_abi.SIG.TMAX_PEAK_LAST) + 1, :n]
        assert any(bool((r != 0).any()) and len(set(r.tolist())) > 1 for r in last), f"{grid}: no published signal row is alive"


@functools.lru_cache(maxsize=None)
def _reference(n_seg, n_envs, bind, seq, autoreset, grid="g0"):
    """The oracle's half of a recipe: blocks (and trace ring) after every launch, computed once per (shape, bindings, mode,
    launch sequence, grid) and left unchanged.  On g1 and g2 it asserts that the launches really hold control steps."""
    env = _make("cpu", n_seg, n_envs, bind, autoreset, grid)
    act = _scenario(env, n_seg)
    dt = cat.GRIDS[grid][0]
    if grid != "g0":
        _stagger(env, grid, seq)
    snaps, trace = [], None
    for index, (us, traced) in enumerate(cat.SEQS[seq]):
        if traced and trace is None:
            trace = env.bind_trace(cat.TRACE_SIGNALS, every=cat.TRACE_EVERY, capacity=cat.TRACE_CAPACITY)
        before, episode = env.state.time_since_servo.clone(), env.state.episode.clone()
        env.step_many(_launch_action(env, grid, act, index), us)
        snaps.append(_snapshot(env, trace))
        if index == 0:  # the termination the FROZEN_OK recipes count on
            assert bool(env.state.is_wire_broken[5]) or autoreset, "environment 5 breaks its wire at the first step"
        if grid != "g0":
            # an environment that ran the whole launch in one episode latched in it iff `time_since_servo` was set back
            ran = ~env.state.done & (env.state.episode == episode)
            latched = ran & (env.state.time_since_servo < before + us * dt)
            assert bool(latched.any()), f"{grid}, launch {index} of {us} steps holds no control step"
            if us == 1:
                assert torch.equal(latched, ran & env.state.control_step), (grid, index)
                assert bool((ran & ~latched).any()), f"{grid}, launch {index}: every environment latches in the single step"
    if grid != "g0":
        _assert_latched_late(env, grid, bind)
    total = sum(us for us, _ in cat.SEQS[seq])
    assert total <= cat.REPLAY_STEPS and not bool(env.state.error.any())
    if total >= 290:  # the scenario sparks
        assert int(env.state.spark_count.sum()) > (n_envs if not bind - {"f64"} else 0), (n_seg, sorted(bind))
    if "replay" in bind:  # the environments took different courses: it matters whose row an environment reads
        assert len(set(env.state.spark_count.tolist())) > 1 and len(set(env.state.workpiece_position.tolist())) > n_envs // 2
        # ... and a tiny debris roll began a short that no Philox uniform could begin
        assert bool(env.state.is_short_circuit[TINY_ROLLS]) and int(env.state.is_short_circuit.sum()) < n_envs // 2
    if trace is not None:
        assert snaps[-1][2] == sum(us for us, t in cat.SEQS[seq] if t) // cat.TRACE_EVERY
    return tuple(snaps)


def _same(a, b):
    if a.is_floating_point():
        return bool(((a == b) | (a.isnan() & b.isnan())).all())
    return torch.equal(a, b)


def _compare(gpu, trace, want, n, where):
    blocks, ring, count = _snapshot(gpu, trace)
    w_blocks, w_ring, w_count = want
    assert_blocks_equal(blocks, w_blocks, n)
    for extra in ("pulse", "signal"):
        assert (extra in blocks) == (extra in w_blocks), (where, extra)
        if extra in blocks:
            assert _same(blocks[extra], w_blocks[extra]), f"{where}: the {extra} block differs"
    assert count == w_count, (where, count, w_count)
    if w_ring is not None:
        for name in cat.TRACE_SIGNALS:
            assert ring[name].shape == w_ring[name].shape and _same(ring[name], w_ring[name]), f"{where}: traced {name} differs"


def _run(recipe, reached, grid="g0"):
    snaps = _reference(*recipe.oracle_key, grid)
    gpu = _make("cuda:0", recipe.n_seg, recipe.n_envs, recipe.bind, recipe.autoreset, grid)
    try:
        gpu.set_kernel(int(recipe.kernel), recipe.lanes)
        act = _scenario(gpu, recipe.n_seg)
        if grid != "g0":
            _stagger(gpu, grid, recipe.seq)
        trace = None
        for index, ((us, traced, sample, expected), want) in enumerate(zip(recipe.launches(), snaps)):
            if traced and trace is None:
                trace = gpu.bind_trace(cat.TRACE_SIGNALS, every=cat.TRACE_EVERY, capacity=cat.TRACE_CAPACITY)
            gpu.step_many(_launch_action(gpu, grid, act, index), us)
            torch.cuda.synchronize()
            ran = gpu._backend.last_form()
            where = f"{recipe.id} on {grid}, launch {index} of {us} steps ({gpu._backend.last_kernel()})"
            assert ran == expected, f"{where}: ran {cat.describe(ran)}, the recipe expected {cat.describe(expected)}"
            reached.add(ran)
            _compare(gpu, trace, want, recipe.n_envs, where)
    finally:
        gpu.close()


FAMILIES = [k for k in K if k != K.AUTO]


def _family_on(family, grid):
    registered = {e for e in _lib.registry() if e[0] == int(family)}
    reached = set()
    for recipe in cat.CATALOGUE[int(family)]:
        _run(recipe, reached, grid)
    missing = registered - set(cat.UNREACHABLE) - reached
    assert not missing, "never launched: " + "; ".join(cat.describe(e) for e in sorted(missing))
    assert reached == registered - set(cat.UNREACHABLE), [cat.describe(e) for e in sorted(reached - registered)]


@pytest.mark.parametrize("family", FAMILIES, ids=[k.name.lower() for k in FAMILIES])
def test_every_instantiation_of_the_family_runs_and_matches_the_oracle(family):
    _family_on(family, "g0")


@pytest.mark.parametrize("family", FAMILIES, ids=[k.name.lower() for k in FAMILIES])
@pytest.mark.parametrize("grid", ["g1", "g2"])
def test_every_instantiation_of_the_family_holds_across_control_steps(grid, family):
    """The same recipes, handles, launch lengths and `last_form()` assertions on the grids g1 (dt 1, servo_interval 100) and
    g2 (dt 3, servo_interval 100): the environments start at staggered points of the control interval and every launch
    offers a new action per environment, so the latch, the rows published at control steps, the observation and the reward
    of a control step are compared in every instantiation, in every launch."""
    _family_on(family, grid)
