"""Per-environment physics parameters (include/wedm_hip.h, enum wedm_envp_field), host side: the C-ABI mirror and export,
the row derivation against `derive.build_params`, validation, the oracle's refusal, the rows a backend is handed and the
checkpoint round trip (against a stub backend that records what is bound), the vector adapter's masked resampling."""
from __future__ import annotations

import dataclasses
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from sparc_amd import _abi, _lib
from sparc_amd.core import derive
from sparc_amd.core import env_params as envp

ROOT = Path(__file__).resolve().parents[1]
DRAWS = 10_000


def test_envp_enum_in_the_header_matches_its_mirror():
    text = (ROOT / "include" / "wedm_hip.h").read_text()
    body = re.search(r"enum wedm_envp_field \{(.*?)\};", text, re.S).group(1)
    names = re.findall(r"WEDM_EP_([A-Z_0-9]+)", body)
    assert names == [f.name for f in _abi.ENVP]
    assert [f.value for f in _abi.ENVP] == list(range(len(names)))
    assert "WEDM_ENVP_COUNT" in body and _abi.ENVP_COUNT == len(names)


def test_bind_env_params_is_exported_and_listed():
    assert "wedm_bind_env_params" in _lib.EXPORTS
    assert "wedm_bind_env_params(" in (ROOT / "include" / "wedm_hip.h").read_text()
    lib_path = ROOT / "sparc_amd" / "libwedm_hip.so"
    if lib_path.exists():
        assert hasattr(_lib.load(), "wedm_bind_env_params")


def _params_for(draw):
    """`build_params` with the dataclasses holding one draw (name -> Python float)."""
    from sparc_amd import (DielectricModuleParameters, EnvironmentConfig, IgnitionModuleParameters,
                           MaterialModuleParameters, MechanicsModuleParameters, WireModuleParameters)
    from sparc_amd.core.material_db import get_material_db

    cls = {"ignition_params": IgnitionModuleParameters, "wire_params": WireModuleParameters,
           "dielectric_params": DielectricModuleParameters, "mechanics_params": MechanicsModuleParameters}
    dc = {src: dataclasses.replace(c(), **{n: draw[n] for n, s in envp.SOURCES.items() if s == src})
          for src, c in cls.items()}
    cfg = EnvironmentConfig()
    mat = get_material_db().get_wire_material(cfg.wire_material)
    geo = derive.derive_geometry(cfg.workpiece_height, cfg.wire_diameter, dc["wire_params"], mat, MaterialModuleParameters())
    return derive.build_params(cfg, "position", dc["ignition_params"], dc["wire_params"], MaterialModuleParameters(),
                               dc["dielectric_params"], dc["mechanics_params"], mat, geometry=geo), dc


# the wedm_params field each device row mirrors
_PARAM_FIELD = {
    _abi.ENVP.BASE_CRITICAL_DENSITY: "base_critical_density", _abi.ENVP.GAP_COEFFICIENT: "gap_coefficient",
    _abi.ENVP.MAX_CRITICAL_DENSITY: "max_critical_density", _abi.ENVP.HARD_SHORT_GAP: "hard_short_gap",
    _abi.ENVP.SIGMOID_STEEPNESS: "sigmoid_steepness", _abi.ENVP.SPARK_VOLTAGE_FACTOR: "spark_voltage_factor",
    _abi.ENVP.DEBRIS_REMOVAL_PER_US: "debris_removal_per_us", _abi.ENVP.DIELECTRIC_TEMPERATURE: "dielectric_temperature",
    _abi.ENVP.PLASMA_EFFICIENCY: "plasma_efficiency", _abi.ENVP.BASE_CONVECTION: "base_convection",
    _abi.ENVP.DAMPING_COEFF: "damping_coeff", _abi.ENVP.STIFFNESS_COEFF: "stiffness_coeff", _abi.ENVP.OMEGA_N: "omega_n",
    _abi.ENVP.MAX_ACCELERATION: "max_acceleration", _abi.ENVP.MAX_JERK_DT: "max_jerk_dt", _abi.ENVP.MAX_SPEED: "max_speed",
}


def _draws(n, seed=0):
    rng = np.random.default_rng(seed)
    uni = {n_: float(getattr(getattr(_UniformHolder, s), n_)) for n_, s in envp.SOURCES.items()}
    # log-uniform factors over two decades around the default: exercises every exponent / rounding pattern
    return {name: uni[name] * np.exp(rng.uniform(-np.log(10.0), np.log(10.0), n)) for name in envp.NAMES}


class _UniformHolder:
    from sparc_amd import (DielectricModuleParameters, IgnitionModuleParameters, MechanicsModuleParameters,
                           WireModuleParameters)

    ignition_params = IgnitionModuleParameters()
    wire_params = WireModuleParameters()
    dielectric_params = DielectricModuleParameters()
    mechanics_params = MechanicsModuleParameters()


def test_row_derivation_is_bit_identical_to_build_params_over_many_draws():
    """Every device row for DRAWS random scalar inputs, from NumPy arrays and from CPU tensors (the host path), against
    what build_params writes for each draw as scalars.  Python's `omega_n ** 2` is C pow: it differs from x * x for some
    of these draws, and the host path must still agree."""
    cols = _draws(DRAWS)
    params = [_params_for({k: float(v[i]) for k, v in cols.items()})[0] for i in range(DRAWS)]
    p0 = params[0]
    consts = {"base_flow_rate": float(_UniformHolder.dielectric_params.base_flow_rate), "dt_s": float(p0.dt_s)}
    want = np.array([[getattr(p, _PARAM_FIELD[r]) for p in params] for r in _abi.ENVP], dtype=np.float64)
    got_np = envp.derive_rows(cols, consts)
    got_t = envp.derive_rows({k: envp.host_column(k, torch.from_numpy(v), DRAWS) for k, v in cols.items()}, consts)
    for got in (got_np, got_t):
        for r in _abi.ENVP:
            assert np.array_equal(got[r].view(np.uint64), want[r].view(np.uint64)), r.name
    w = cols["omega_n"]
    assert (w * w != np.array([v ** 2 for v in w.tolist()])).any()  # (the case the host path exists for)


def test_device_derivation_is_bit_identical_to_build_params_where_it_promises():
    """The torch expressions the device path evaluates (here on CPU tensors: the same IEEE products): every row for
    arbitrary draws, the stiffness row for omega_n with 26 significant bits (what uniform_param_sampler draws)."""
    cols = _draws(DRAWS, seed=1)
    w = cols["omega_n"]
    cols["omega_n"] = (w.view(np.int64) & ~np.int64((1 << 27) - 1)).view(np.float64)
    params = [_params_for({k: float(v[i]) for k, v in cols.items()})[0] for i in range(DRAWS)]
    consts = {"base_flow_rate": float(_UniformHolder.dielectric_params.base_flow_rate), "dt_s": float(params[0].dt_s)}
    got = envp.derive_rows({k: torch.from_numpy(v) for k, v in cols.items()}, consts).numpy()
    for r in _abi.ENVP:
        want = np.array([getattr(p, _PARAM_FIELD[r]) for p in params], dtype=np.float64)
        assert np.array_equal(got[r].view(np.uint64), want.view(np.uint64)), r.name


class StubBackend:
    """Records what the environment binds; steps nothing."""

    name = "stub"
    instances = []

    def __init__(self, params, num_envs, n_seg_max, device):
        self.params, self.num_envs, self.envp_ptr = params, num_envs, "never bound"
        StubBackend.instances.append(self)

    def bind_state(self, ptrs):
        pass

    def bind_geometry(self, ptrs):
        pass

    def bind_env_params(self, ptr):
        self.envp_ptr = ptr

    def reset(self, mask_ptr, seed, reseed, fresh=False):
        pass

    def step(self, n_substeps, action):
        pass

    def close(self):
        pass


def _stub_env(n=100, **kw):
    from sparc_amd import WireEDMEnv

    return WireEDMEnv(num_envs=n, device="cpu", backend=StubBackend, **kw)


def test_constructor_rows_equal_build_params_per_environment_and_are_bound():
    from sparc_amd import MechanicsModuleParameters

    n = 300
    rng = np.random.default_rng(3)
    omega = rng.uniform(100.0, 400.0, n)
    zeta = torch.from_numpy(rng.uniform(0.2, 0.9, n))
    env = _stub_env(n, env_params={"omega_n": omega, "zeta": zeta, "dielectric_temperature": 280.0,
                                   "debris_removal_efficiency": list(rng.uniform(0.001, 0.05, n))},
                    mechanics_params=MechanicsModuleParameters(max_jerk=2.0e8))
    assert env._backend.envp_ptr == env._envp_rows.data_ptr()
    assert env.env_param_names == ("debris_removal_efficiency", "dielectric_temperature", "omega_n", "zeta")
    rows = env._envp_rows.numpy()
    got = env.get_env_params()
    for e in (0, 1, 57, n - 1):
        draw = {k: float(v[e]) for k, v in got.items()}
        p, _ = _params_for(draw)
        for r in _abi.ENVP:
            assert rows[r, e] == getattr(p, _PARAM_FIELD[r]), (r.name, e)
    assert got["max_jerk"].eq(2.0e8).all() and got["dielectric_temperature"].eq(280.0).all()
    assert np.array_equal(got["omega_n"].numpy(), omega)
    # padding columns repeat the last environment
    assert (rows[:, n:] == rows[:, n - 1: n]).all()


def test_validation_errors():
    with pytest.raises(ValueError, match="unknown per-environment parameter"):
        _stub_env(4, env_params={"omega": 1.0})
    with pytest.raises(ValueError, match="unknown per-environment parameter"):
        _stub_env(4, env_params={"random_short_max_probability": 0.1})  # (excluded on purpose)
    with pytest.raises(ValueError, match="one value per environment"):
        _stub_env(4, env_params={"zeta": [0.3, 0.4, 0.5]})
    with pytest.raises(ValueError, match="non-finite"):
        _stub_env(4, env_params={"zeta": [0.3, float("nan"), 0.5, 0.4]})
    with pytest.raises(ValueError, match="non-finite"):
        _stub_env(4, env_params={"max_speed": np.array([1.0, 2.0, np.inf, 3.0])})
    env = _stub_env(4, env_params={"zeta": 0.4})
    with pytest.raises(ValueError, match="not randomised in this environment"):
        env.set_env_params({"omega_n": 200.0})
    with pytest.raises(ValueError, match="unknown per-environment parameter"):
        env.set_env_params({"zta": 0.2})
    with pytest.raises(ValueError, match="one value per environment"):
        env.set_env_params({"zeta": torch.ones(5, dtype=torch.float64)})
    with pytest.raises(ValueError, match="non-finite"):
        env.set_env_params({"zeta": [0.1, 0.2, float("-inf"), 0.3]})
    with pytest.raises(ValueError, match="mask must have one entry"):
        env.set_env_params({"zeta": 0.5}, mask=[True, False])
    plain = _stub_env(4)
    with pytest.raises(RuntimeError, match="env_params"):
        plain.set_env_params({"zeta": 0.5})
    with pytest.raises(RuntimeError, match="env_params"):
        plain.get_env_params()


def test_oracle_backend_refuses_env_params():
    from sparc_amd import WireEDMEnv
    from tests._oracle_backend import OracleBackend

    with pytest.raises(ValueError, match="env_params needs a backend"):
        WireEDMEnv(num_envs=4, device="cpu", env_params={"zeta": 0.5}, backend=OracleBackend)


def test_masked_set_env_params_changes_only_the_masked_environments_and_derives_rows():
    n = 64
    env = _stub_env(n, env_params={"omega_n": 235.0, "zeta": 0.38, "max_jerk": 1e8})
    before = env._envp_rows.clone()
    mask = torch.arange(n) % 3 == 0
    omega = torch.linspace(150.0, 300.0, n, dtype=torch.float64)
    env.set_env_params({"omega_n": omega, "max_jerk": 5e7}, mask=mask)
    rows, got = env._envp_rows, env.get_env_params()
    E = _abi.ENVP
    assert torch.equal(rows[:, :n][:, ~mask], before[:, :n][:, ~mask])
    assert torch.equal(got["omega_n"][mask], omega[mask]) and got["omega_n"][~mask].eq(235.0).all()
    for e in torch.nonzero(mask).flatten().tolist():
        p, _ = _params_for({k: float(v[e]) for k, v in got.items()})
        for r in (E.OMEGA_N, E.STIFFNESS_COEFF, E.DAMPING_COEFF, E.MAX_JERK_DT):
            assert rows[r, e].item() == getattr(p, _PARAM_FIELD[r]), (r.name, e)
    assert torch.equal(rows[E.SIGMOID_STEEPNESS], before[E.SIGMOID_STEEPNESS])  # not named: untouched


def test_state_dict_carries_the_rows_and_refuses_another_set_of_names(tmp_path):
    n = 50
    a = _stub_env(n, env_params={"zeta": 0.4, "plasma_efficiency": np.linspace(0.05, 0.2, n)})
    a.set_env_params({"zeta": torch.linspace(0.2, 0.8, n, dtype=torch.float64)})
    a.save_checkpoint(tmp_path / "a.pt")
    b = _stub_env(n, env_params={"zeta": 0.4, "plasma_efficiency": 0.1})
    assert not torch.equal(b._envp_rows, a._envp_rows)
    ptr = b._envp_rows.data_ptr()
    b.load_checkpoint(tmp_path / "a.pt")
    assert torch.equal(b._envp_rows, a._envp_rows) and torch.equal(b._envp_src, a._envp_src)
    assert b._envp_rows.data_ptr() == ptr == b._backend.envp_ptr  # loaded in place: the bound pointer stays valid
    for k, v in a.get_env_params().items():
        assert torch.equal(b.get_env_params()[k], v)
    with pytest.raises(ValueError, match="per-environment physics parameters"):
        _stub_env(n, env_params={"zeta": 0.4}).load_state_dict(a.state_dict())
    with pytest.raises(ValueError, match="per-environment physics parameters"):
        _stub_env(n).load_state_dict(a.state_dict())
    with pytest.raises(ValueError, match="per-environment physics parameters"):
        a.load_state_dict(_stub_env(n).state_dict())


def test_uniform_param_sampler_and_the_vector_adapter_resample_only_where_reset():
    from sparc_amd import WireEDMVectorEnv, uniform_param_sampler

    n = 200
    env = _stub_env(n, env_params={"omega_n": 235.0, "sigmoid_steepness": 500.0})
    sampler = uniform_param_sampler({"omega_n": (150.0, 300.0), "sigmoid_steepness": (300.0, 700.0)},
                                    torch.Generator().manual_seed(0))
    vec = WireEDMVectorEnv(env, param_sampler=sampler)
    vec.reset(seed=1)
    p0 = env.get_env_params()
    assert p0["omega_n"].min() >= 150.0 and p0["omega_n"].max() < 300.0 and p0["omega_n"].unique().numel() > n // 2
    w = p0["omega_n"]
    assert torch.equal(w * w, torch.tensor([v ** 2 for v in w.tolist()], dtype=torch.float64))  # 26 bits: exact squares
    mask = torch.arange(n) % 4 == 1
    vec._need_reset = mask.clone()
    vec._apply_sampler(vec._need_reset)
    p1 = env.get_env_params()
    changed = (p1["omega_n"] != p0["omega_n"]) | (p1["sigmoid_steepness"] != p0["sigmoid_steepness"])
    assert changed[mask].all() and not changed[~mask].any()
    with pytest.raises(ValueError, match="param_sampler needs an environment built with env_params"):
        WireEDMVectorEnv(_stub_env(8), param_sampler=sampler)
