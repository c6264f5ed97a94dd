"""The CPU oracle's per-environment wire-material rows (`wedm_oracle_step_batch_wmat`'s ``wmat_rows``, the oracle side of
wedm_bind_wire_material in include/wedm_hip.h) against references that do not use them.

Every environment of a mixed batch -- brass, fixture F14's copper and two synthetic materials whose critical and breaking
temperatures round up and down in float32 -- equals, on every byte, a one-environment run whose configuration holds that
environment's material (``EnvironmentConfig(wire_material=name)``, same seed, ``env_id_offset = e``, same geometry).  Hot
bands sit between each environment's own critical and breaking temperatures, on the float32 neighbours of both limits
and above the breaking one, so the per-environment limits decide.  Rows holding the configuration's own material change
nothing, and a masked `set_wire_material` takes effect at the next launch.  These tests make the oracle the checker of
the kernels' MAT forms (tests/test_wire_material_fuzz.py, tests/test_thermal_limits.py)."""
from __future__ import annotations

import zlib

import numpy as np
import pytest
import torch

from sparc_amd import EnvironmentConfig, WireEDMEnv, _abi
from tests import _envp_draw as D
from tests import _wmat_draw as W
from tests._compare import block_diffs
from tests._oracle_backend import OracleBackend, OracleBackendRows

N = 24
SEED = 4242
LAUNCHES = (1000, 7, 1300, 1, 400)
BAND = slice(170, 176)  # inside the workpiece zone for every height drawn here
MATERIALS = W.fixed_materials()
NAMES = [m.name for m in MATERIALS]


@pytest.fixture(autouse=True)
def _materials():
    W.register(MATERIALS)


def test_the_materials_round_both_ways():
    tc, tb = W.limits(MATERIALS, np.arange(len(MATERIALS)))
    assert {W.rounding(x) for x in tc} == {-1, +1}
    assert {W.rounding(x) for x in tb} == {-1, 0, +1}
    assert (tc + 100.0 < tb).all()


# mode -> (WireEDMEnv keywords, EnvironmentConfig keywords, extras)
MODES = {
    "position": ({}, {}, {}),
    "velocity": (dict(mechanics_control_mode="velocity"), {}, {}),
    "dt2": ({}, dict(dt=2), {}),
    "reference_reset": (dict(reset_semantics="reference"), {}, dict(terminate=True, masked_reset=True)),
    "keep_stepping": (dict(freeze_terminated=False), {}, dict(terminate=True)),
    "autoreset_crater_log": (dict(autoreset=True, reward="progress", crater_log_capacity=8), {}, dict(terminate=True)),
    "stencil_f64": (dict(stencil_dtype="float64"), {}, {}),
    "pulse_stats": (dict(pulse_stats=True), {}, {}),
    "env_params": ({}, {}, dict(envp=True)),
}


def _config(material, **kw):
    return EnvironmentConfig(target_cutting_distance=5000.0, wire_material=material, **kw)


class Scene:
    """One mode's draw: materials, geometry, start, bands and actions per environment."""

    def __init__(self, mode, seed):
        self.kw, self.cfg, self.extra = MODES[mode]
        rng = np.random.default_rng(seed)
        self.mid = np.r_[np.arange(len(NAMES)), rng.integers(0, len(NAMES), N - len(NAMES))]
        rng.shuffle(self.mid)
        self.h, self.d = rng.uniform(10.0, 30.0, N), rng.choice([0.1, 0.15, 0.25], N)
        self.gaps = np.where(rng.random(N) < 0.5, rng.uniform(0.5, 5.0, N), rng.uniform(5.0, 30.0, N))
        self.debris = np.where(rng.random(N) < 0.3, rng.uniform(0.0, 0.2, N), rng.uniform(0.0, 0.01, N))
        tc, tb = W.limits(MATERIALS, self.mid)
        self.band = W.hot_bands(rng, tc, tb)
        velocity = self.kw.get("mechanics_control_mode") == "velocity"
        self.servo = rng.uniform(50, 300, N) if velocity else \
            rng.uniform(-0.05, 0.3, N) * rng.choice([1.0, 1.0, 20.0, -3.0], N)
        self.modes = rng.choice([1, 5, 9, 13, 15, 17], N).astype(np.int32)
        self.envp = D.draw(rng, N) if self.extra.get("envp") else None
        self.reset_mask = np.arange(N) % 3 == 1

    def prepare(self, env, lo, hi):
        env.reset(seed=SEED)
        idx = np.arange(lo, hi)
        env.state.wire_position = 10.0
        env.state.workpiece_position = torch.as_tensor(10.0 + self.gaps[lo:hi])
        env.state.debris_volume = torch.as_tensor(self.debris[lo:hi])
        if self.extra.get("terminate"):  # three environments in five sit right before their cutting targets
            env.state.target_position = torch.as_tensor(np.where(idx % 5 < 3, 10.0 + self.gaps[lo:hi] + 0.001, 5000.0))
        else:
            env.state.target_position = 5000.0
        T = env.state.wire_temperature
        for j, e in enumerate(idx):
            T[j, BAND] = float(self.band[e])

    def drive(self, env, lo, hi):
        self.prepare(env, lo, hi)
        a = env.make_action(self.servo[lo:hi], 80.0, self.modes[lo:hi], 2.0, 25.0)
        for i, k in enumerate(LAUNCHES):
            if self.extra.get("masked_reset") and i == 2:
                env.reset(options={"mask": self.reset_mask[lo:hi]})
            env.step_many(a, k)
        return env.state.clone_blocks()

    def batch(self, backend=OracleBackendRows, materials=None):
        kw = dict(self.kw, config=_config("brass", **self.cfg), workpiece_height=self.h, wire_diameter=self.d)
        if materials is not None:
            kw.update(wire_material=materials, wire_material_table=NAMES)  # (indices into NAMES)
        if self.envp is not None:
            kw["env_params"] = self.envp
        return WireEDMEnv(num_envs=N, device="cpu", backend=backend, **kw)

    def single(self, e, material):
        kw = dict(self.kw, config=_config(material, **self.cfg), workpiece_height=self.h[e:e + 1],
                  wire_diameter=self.d[e:e + 1])
        if self.envp is not None:
            kw.update(D.uniform_kw(D.column(self.envp, e)))
        # (OracleBackendRows for the pulse tally alone: no material rows are bound here)
        return WireEDMEnv(num_envs=1, device="cpu", backend=OracleBackendRows, env_id_offset=e, **kw)


def _cols(blocks, e, nq=None):
    out = {k: v[:, e:e + 1] for k, v in blocks.items()}
    if nq is not None:
        out["T"] = out["T"][:nq]
    return out


def assert_env_equal(got, want, e, where):
    nq = want["T"].shape[0]
    diffs = block_diffs(_cols(got, e, nq), _cols(want, 0), 1)
    assert not diffs, f"{where}: environment {e}:\n" + "\n".join(diffs[:12])
    for extra in ("crater_log", "pulse"):
        if extra in want:
            assert torch.equal(got[extra][:, e], want[extra][:, 0]), (where, e, extra)


@pytest.mark.parametrize("mode", list(MODES))
def test_batch_equals_one_environment_uniform_runs(mode):
    """Environment e of the mixed batch == a one-environment run whose configured material is e's, every block."""
    sc = Scene(mode, zlib.crc32(mode.encode()))
    batch = sc.batch(materials=[NAMES[k] for k in sc.mid])
    got = sc.drive(batch, 0, N)
    name = batch._backend.last_kernel()
    assert "[wmat]" in name and ("[envp]" in name) == (sc.envp is not None), name
    assert ("[pulse]" in name) == bool(sc.kw.get("pulse_stats")), name
    for e in range(N):
        want = sc.drive(sc.single(e, NAMES[sc.mid[e]]), e, e + 1)
        assert_env_equal(got, want, e, mode)
    # the limits were per environment: some band between a material's limits was counted critical, some broke
    tcrit = got["i32"][_abi.I32.TIME_CRITICAL, :N].numpy()
    broken = got["i8"][_abi.I8.WIRE_BROKEN, :N].numpy() != 0
    if not sc.kw.get("autoreset"):
        assert broken.any() and not broken.all(), broken
    assert (tcrit > 0).any() or sc.kw.get("autoreset") or broken.all()
    if sc.kw.get("autoreset"):
        assert int(got["i32"][_abi.I32.EPISODE, :N].sum()) >= 3


def test_the_rows_matter():
    """The same mixed batch with the rows left unbound (every environment brass) differs in every non-brass material."""
    sc = Scene("position", 99)
    got = sc.drive(sc.batch(materials=[NAMES[k] for k in sc.mid]), 0, N)
    plain = sc.drive(sc.batch(backend=OracleBackend), 0, N)
    for k in range(1, len(NAMES)):
        idx = np.nonzero(sc.mid == k)[0]
        assert any(block_diffs(_cols(got, e), _cols(plain, e), 1) for e in idx), NAMES[k]
    brass = np.nonzero(sc.mid == 0)[0]
    for e in brass:  # (brass is the configured material: its rows change nothing)
        assert not block_diffs(_cols(got, e), _cols(plain, e), 1), e


@pytest.mark.parametrize("mode", ["position", "velocity", "dt2", "autoreset_crater_log", "stencil_f64", "pulse_stats"])
@pytest.mark.parametrize("material", ["brass", "synthetic_crit_up"])
def test_rows_holding_the_configured_material_change_nothing(mode, material):
    sc = Scene(mode, 5)
    kw = dict(sc.kw, config=_config(material, **sc.cfg), workpiece_height=sc.h, wire_diameter=sc.d)
    rows = WireEDMEnv(num_envs=N, device="cpu", backend=OracleBackendRows, wire_material=[material] * N, **kw)
    plain = WireEDMEnv(num_envs=N, device="cpu", backend=OracleBackendRows, **kw)
    with_rows, without = sc.drive(rows, 0, N), sc.drive(plain, 0, N)
    assert "[wmat]" in rows._backend.last_kernel() and "[wmat]" not in plain._backend.last_kernel()
    diffs = block_diffs(with_rows, without, N)
    assert not diffs, "\n".join(diffs[:12])
    for extra in ("crater_log", "pulse"):
        if extra in without:
            assert torch.equal(with_rows[extra], without[extra]), extra


def test_a_masked_switch_takes_effect_at_the_next_launch_only_where_masked():
    """`set_wire_material` between launches (masked): the switched environments follow a one-environment run of the new
    material from the copied state; the others keep theirs."""
    sc = Scene("position", 7)
    env = sc.batch(materials=[NAMES[k] for k in sc.mid])
    sc.prepare(env, 0, N)
    a = env.make_action(sc.servo, 80.0, sc.modes, 2.0, 25.0)
    env.step_many(a, 700)
    mid = env.state.clone_blocks()
    new = (sc.mid + 1 + np.arange(N) % 3) % len(NAMES)
    mask = np.arange(N) % 2 == 0
    env.set_wire_material(torch.from_numpy(new), mask=torch.from_numpy(mask))
    assert [m.name for m in env.wire_materials] == NAMES
    now = env.get_wire_material_index().numpy()
    assert np.array_equal(now, np.where(mask, new, sc.mid))
    env.step_many(a, 1300)
    got = env.state.clone_blocks()
    for e in range(N):
        one = sc.single(e, NAMES[now[e]])
        one.reset(seed=SEED)
        blocks = one.state.clone_blocks()
        nq = blocks["T"].shape[0]
        for k in ("f64", "i32", "i8", "obs", "stats", "reward"):
            blocks[k][:, 0] = mid[k][:, e]  # environment e's state after the first launch
        blocks["T"][:, 0] = mid["T"][:nq, e]
        one.state.load_blocks(blocks)
        one.step_many(one.make_action(sc.servo[e:e + 1], 80.0, sc.modes[e:e + 1], 2.0, 25.0), 1300)
        assert_env_equal(got, one.state.clone_blocks(), e, "after the switch")
    # the switch changed something where it applied (the old material's continuation is another trajectory)
    changed = mask & (new != sc.mid)
    assert changed.sum() >= 6
