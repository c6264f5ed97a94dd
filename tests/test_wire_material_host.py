"""Per-environment wire material (include/wedm_hip.h, enum wedm_wmat_field), host side: the C-ABI mirror and export, the
material rows and the material's geometry rows against `derive.build_params` / `derive.derive_geometry`, padding,
validation, `MaterialDatabase.add_wire_material`, the rows a backend is handed, device-free switching and the checkpoint
round trip (against a stub backend that records what is bound)."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest
import torch

from sparc_amd import _abi, _lib
from sparc_amd.core import derive
from sparc_amd.core.material_db import MaterialDatabase, WireMaterial, get_material_db
from sparc_amd.modules.parameters import (DielectricModuleParameters, IgnitionModuleParameters, MaterialModuleParameters,
                                          MechanicsModuleParameters, WireModuleParameters)

ROOT = Path(__file__).resolve().parents[1]

# brass (built in), the f14 fixture's copper, and a synthetic material that differs from both in every field
COPPER = WireMaterial(name="copper", density=8960, specific_heat=385, thermal_conductivity=401,
                      electrical_resistivity=1.68e-08, temperature_coefficient=0.00393, melting_point=1358,
                      breaking_temperature=1600)
SYNTH = WireMaterial(name="synthetic_host", density=7700.5, specific_heat=460.25, thermal_conductivity=52.5,
                     electrical_resistivity=1.1e-07, temperature_coefficient=0.0052, melting_point=1650.5,
                     breaking_temperature=1720.0)


def _materials():
    return (get_material_db().get_wire_material("brass"), COPPER, SYNTH)


def test_wmat_enum_in_the_header_matches_its_mirror():
    text = (ROOT / "include" / "wedm_hip.h").read_text()
    body = re.search(r"enum wedm_wmat_field \{(.*?)\};", text, re.S).group(1)
    names = re.findall(r"WEDM_WM_([A-Z_0-9]+)", body)
    assert names == [f.name for f in _abi.WMAT]
    assert [f.value for f in _abi.WMAT] == list(range(len(names)))
    assert "WEDM_WMAT_COUNT" in body and _abi.WMAT_COUNT == len(names)


def test_bind_wire_material_is_declared_exported_and_listed():
    assert "wedm_bind_wire_material" in _lib.EXPORTS
    assert "int32_t wedm_bind_wire_material(wedm_ctx* ctx, const double* rows);" in (ROOT / "include" / "wedm_hip.h").read_text()
    lib_path = ROOT / "sparc_amd" / "libwedm_hip.so"
    if lib_path.exists():
        assert hasattr(_lib.load(), "wedm_bind_wire_material")
    assert hasattr(_lib.HipBackend, "bind_wire_material")


def _params(material):
    from sparc_amd import EnvironmentConfig

    return derive.build_params(EnvironmentConfig(), "position", IgnitionModuleParameters(), WireModuleParameters(),
                               MaterialModuleParameters(), DielectricModuleParameters(), MechanicsModuleParameters(),
                               material, geometry=None)


FIELD_OF_ROW = {_abi.WMAT.RHO_ELEC: "rho_elec", _abi.WMAT.ALPHA_RHO: "alpha_rho", _abi.WMAT.RHO_C: "rho_c",
                _abi.WMAT.CRITICAL_TEMPERATURE: "critical_temperature",
                _abi.WMAT.BREAKING_TEMPERATURE: "breaking_temperature"}


@pytest.mark.parametrize("threshold", [0.9, 0.85, 0.7777])
def test_material_rows_equal_build_params_bit_for_bit(threshold):
    mats = _materials()
    wire = WireModuleParameters(critical_temp_threshold=threshold)
    idx = np.array([2, 0, 1, 1, 2, 0, 0])
    rows = derive.material_rows(mats, idx, wire, 64)
    assert rows.shape == (_abi.WMAT_COUNT, 64) and rows.dtype == np.float64
    for e, k in enumerate(idx):
        from sparc_amd import EnvironmentConfig

        p = derive.build_params(EnvironmentConfig(), "position", IgnitionModuleParameters(), wire, MaterialModuleParameters(),
                                DielectricModuleParameters(), MechanicsModuleParameters(), mats[k], geometry=None)
        for r, field in FIELD_OF_ROW.items():
            assert rows[r, e].tobytes() == np.float64(getattr(p, field)).tobytes(), (e, field)


def test_geometry_rows_per_environment_material_equal_derive_geometry():
    mats = _materials()
    rng = np.random.default_rng(3)
    n = 37
    h = rng.choice([10.0, 20.0, 30.0], n)
    d = rng.choice([0.1, 0.25, 0.3], n)
    idx = rng.integers(0, 3, n)
    wire, mp = WireModuleParameters(), MaterialModuleParameters()
    f64, i32, nmax = derive.geometry_rows(h, d, wire, [mats[k] for k in idx], mp, 64)
    for e in range(n):
        g = derive.derive_geometry(h[e], d[e], wire, mats[idx[e]], mp)
        assert f64[_abi.GF64.K_COND, e].tobytes() == np.float64(g.k_cond).tobytes()
        assert f64[_abi.GF64.TUF, e].tobytes() == np.float64(g.tuf).tobytes()
        assert f64[_abi.GF64.A_SURF, e] == g.a_surf and i32[_abi.GI32.N_SEG, e] == g.n_seg
    # one material for all: the rows the single-material call gives
    same = derive.geometry_rows(h, d, wire, mats[0], mp, 64)
    alls = derive.geometry_rows(h, d, wire, [mats[0]] * n, mp, 64)
    assert np.array_equal(same[0], alls[0]) and np.array_equal(same[1], alls[1]) and same[2] == alls[2] == nmax
    # the materials really differ in K_COND / TUF
    assert len({f64[_abi.GF64.K_COND, e] for e in range(n) if (h[e], d[e]) == (h[0], d[0])}) == len(
        {idx[e] for e in range(n) if (h[e], d[e]) == (h[0], d[0])})
    with pytest.raises(ValueError, match="one per environment"):
        derive.geometry_rows(h, d, wire, [mats[0]] * (n - 1), mp, 64)


def test_padding_columns_repeat_the_last_environment():
    mats = _materials()
    rows = derive.material_rows(mats, np.array([0, 1, 2]), WireModuleParameters(), 64)
    assert np.array_equal(rows[:, 3:], np.repeat(rows[:, 2:3], 61, axis=1))
    assert not np.array_equal(rows[:, 0], rows[:, 2])


def test_material_rows_validation():
    mats = _materials()
    wire = WireModuleParameters()
    with pytest.raises(ValueError, match="out of range"):
        derive.material_rows(mats, np.array([0, 3]), wire, 64)
    with pytest.raises(ValueError, match="out of range"):
        derive.material_rows(mats, np.array([-1]), wire, 64)
    with pytest.raises(ValueError, match="integers"):
        derive.material_rows(mats, np.array([0.0, 1.0]), wire, 64)
    with pytest.raises(ValueError, match="entries"):
        derive.material_rows(mats, np.zeros(65, dtype=np.int64), wire, 64)


def test_add_wire_material():
    db = MaterialDatabase()
    assert "synthetic_host" not in db.names()
    db.add_wire_material(SYNTH)
    assert db.get_wire_material("synthetic_host") is SYNTH and "synthetic_host" in db.names()
    with pytest.raises(TypeError):
        db.add_wire_material({"name": "x"})


class StubBackend:
    """Records what the environment binds; steps nothing."""

    def __init__(self, params, num_envs, n_seg_max, device):
        self.params, self.num_envs, self.wmat_ptr, self.geom = params, num_envs, "never bound", None

    def bind_state(self, ptrs):
        pass

    def bind_geometry(self, ptrs):
        self.geom = ptrs

    def bind_env_params(self, ptr):
        pass

    def bind_wire_material(self, ptr):
        self.wmat_ptr = ptr

    def reset(self, mask_ptr, seed, reseed, fresh=False):
        pass

    def step(self, n_substeps, action):
        pass

    def close(self):
        pass


def _stub_env(n=100, **kw):
    from sparc_amd import WireEDMEnv

    get_material_db().add_wire_material(COPPER)
    return WireEDMEnv(num_envs=n, device="cpu", backend=StubBackend, **kw)


def _names(idx):
    return [("brass", "copper", SYNTH)[k] for k in idx]


def test_constructor_rows_equal_build_params_per_environment_and_are_bound():
    n = 100
    idx = np.random.default_rng(0).integers(0, 3, n)
    h = np.linspace(10.0, 30.0, n)
    env = _stub_env(n, wire_material=_names(idx), workpiece_height=h)
    given = [m.name if isinstance(m, WireMaterial) else m for m in _names(idx)]
    assert [m.name for m in env.wire_materials] == list(dict.fromkeys(given))  # distinct, in order of first appearance
    assert env._backend.wmat_ptr == env._wmat_rows.data_ptr()
    assert env.per_env_geometry and env._backend.geom is not None
    got = env.get_wire_material_index()
    assert got.dtype == torch.int64 and got.shape == (n,)
    mats = [env.wire_materials[k] for k in got.tolist()]
    assert [m.name for m in mats] == given
    d = np.full(n, env.config.wire_diameter)
    for e in range(n):
        p = _params(mats[e])
        for r, field in FIELD_OF_ROW.items():
            assert env._wmat_rows[r, e].item() == getattr(p, field), (e, field)
        g = derive.derive_geometry(h[e], d[e], env.wire_params, mats[e], env.material_params)
        assert env._geom_f64[_abi.GF64.K_COND, e].item() == g.k_cond and env._geom_f64[_abi.GF64.TUF, e].item() == g.tuf
    # padding columns follow the last environment
    assert torch.equal(env._wmat_rows[:, n:], env._wmat_rows[:, n - 1: n].expand(-1, env.state.stride - n))
    assert torch.equal(env._geom_f64[:, n:], env._geom_f64[:, n - 1: n].expand(-1, env.state.stride - n))


def test_validation_errors():
    from sparc_amd import WireEDMEnv
    from tests._oracle_backend import OracleBackend

    with pytest.raises(ValueError, match="one per environment"):
        _stub_env(10, wire_material=["brass"] * 9)
    with pytest.raises(ValueError, match="Unknown wire material"):
        _stub_env(3, wire_material=["brass", "unobtainium", "brass"])
    with pytest.raises(ValueError, match="sequence"):
        _stub_env(3, wire_material="brass")
    with pytest.raises(ValueError, match="two different materials"):
        _stub_env(2, wire_material=[COPPER, WireMaterial(**{**COPPER.__dict__, "density": 1.0})])
    with pytest.raises(ValueError, match="bind_wire_material"):
        WireEDMEnv(num_envs=4, device="cpu", wire_material=["brass"] * 4, backend=OracleBackend)
    env = _stub_env(5, wire_material=["brass", "copper", "brass", "brass", "copper"])
    with pytest.raises(ValueError, match="out of range"):
        env.set_wire_material([0, 1, 2, 0, 1])
    with pytest.raises(ValueError, match="out of range"):
        env.set_wire_material(-1)
    with pytest.raises(ValueError, match="one entry per environment"):
        env.set_wire_material([0, 1])
    with pytest.raises(ValueError, match="integers"):
        env.set_wire_material([0.5] * 5)
    with pytest.raises(ValueError, match="mask"):
        env.set_wire_material(1, mask=[True, False])
    with pytest.raises(RuntimeError, match="wire_material"):
        _stub_env(4).set_wire_material(0)
    with pytest.raises(RuntimeError, match="wire_material"):
        _stub_env(4).get_wire_material_index()


def test_masked_switch_is_a_column_select_of_the_material_tables():
    n = 64
    env = _stub_env(n, wire_material=_names(np.arange(n) % 3), wire_diameter=np.linspace(0.1, 0.3, n))
    before_geom, before_rows = env._geom_f64.clone(), env._wmat_rows.clone()
    mask = torch.arange(n) % 4 == 0
    env.set_wire_material(torch.full((n,), 2), mask=mask)
    idx = env.get_wire_material_index()
    want = torch.where(mask, torch.full((n,), 2), torch.as_tensor(np.arange(n) % 3))
    assert torch.equal(idx, want)
    for e in range(n):
        k = int(idx[e])
        assert torch.equal(env._wmat_rows[:, e], env._wmat_table[k, :, e])
        assert torch.equal(env._geom_f64[:, e], env._wmat_geom_table[k, :, e])
        if not mask[e]:
            assert torch.equal(env._wmat_rows[:, e], before_rows[:, e]) and torch.equal(env._geom_f64[:, e], before_geom[:, e])
    # back again: the original rows, bit for bit
    env.set_wire_material(np.arange(n) % 3)
    assert torch.equal(env._wmat_rows, before_rows) and torch.equal(env._geom_f64, before_geom)


def test_state_dict_keeps_the_index_and_refuses_another_material_table(tmp_path):
    n = 50
    names = _names(np.arange(n) % 3)
    a = _stub_env(n, wire_material=names)
    a.set_wire_material(np.arange(n)[::-1] % 3)
    a.save_checkpoint(tmp_path / "a.pt")
    b = _stub_env(n, wire_material=names)
    assert not torch.equal(b.get_wire_material_index(), a.get_wire_material_index())
    ptr = b._wmat_rows.data_ptr()
    b.load_checkpoint(tmp_path / "a.pt")
    assert torch.equal(b.get_wire_material_index(), a.get_wire_material_index())
    assert torch.equal(b._wmat_rows, a._wmat_rows) and torch.equal(b._geom_f64, a._geom_f64)
    assert b._wmat_rows.data_ptr() == ptr == b._backend.wmat_ptr  # switched in place: the bound pointer stays valid
    other = WireMaterial(**{**SYNTH.__dict__, "breaking_temperature": 1700.0})
    with pytest.raises(ValueError, match="material table differs"):
        _stub_env(n, wire_material=[other if m is SYNTH else m for m in names]).load_state_dict(a.state_dict())
    with pytest.raises(ValueError, match="wire materials"):
        _stub_env(n, wire_material=["brass"] * n).load_state_dict(a.state_dict())
    with pytest.raises(ValueError, match="wire materials"):
        _stub_env(n).load_state_dict(a.state_dict())
    with pytest.raises(ValueError, match="wire materials"):
        a.load_state_dict(_stub_env(n).state_dict())


def test_uniform_material_sampler_and_the_vector_adapter_resample_only_where_reset():
    from sparc_amd import WireEDMVectorEnv, uniform_material_sampler

    n = 300
    env = _stub_env(n, wire_material=["brass", "copper", SYNTH] * (n // 3))
    vec = WireEDMVectorEnv(env, material_sampler=uniform_material_sampler(torch.Generator().manual_seed(0)))
    vec.reset(seed=1)
    i0 = env.get_wire_material_index()
    assert set(i0.tolist()) == {0, 1, 2}
    mask = torch.arange(n) % 4 == 1
    vec._apply_sampler(mask)
    i1 = env.get_wire_material_index()
    assert torch.equal(i1[~mask], i0[~mask]) and bool((i1[mask] != i0[mask]).any())
    with pytest.raises(ValueError, match="material_sampler needs an environment built with wire_material"):
        WireEDMVectorEnv(_stub_env(8), material_sampler=uniform_material_sampler())


def test_a_fixed_material_table_orders_env_wire_materials():
    env = _stub_env(4, wire_material=["copper", "brass", "copper", "brass"], wire_material_table=["brass", SYNTH, "copper"])
    assert [m.name for m in env.wire_materials] == ["brass", "synthetic_host", "copper"]
    assert env.get_wire_material_index().tolist() == [2, 0, 2, 0]
    with pytest.raises(ValueError, match="not in wire_material_table"):
        _stub_env(2, wire_material=["brass", SYNTH], wire_material_table=["brass", "copper"])
    with pytest.raises(ValueError, match="twice"):
        _stub_env(2, wire_material=["brass", "brass"], wire_material_table=["brass", "brass"])
    with pytest.raises(ValueError, match="needs wire_material"):
        _stub_env(2, wire_material_table=["brass"])


def _shard_worker(rank, world, port, out):
    import os

    import torch.distributed as dist

    from sparc_amd.parallel import ShardedWireEDMEnv

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        get_material_db().add_wire_material(COPPER)
        # rank 0's half holds brass and copper, rank 1's half the synthetic material and brass
        mats = ["copper", "brass", "copper", "brass", SYNTH, "brass", SYNTH, "brass"]
        sh = ShardedWireEDMEnv(8, device="cpu", backend=StubBackend, wire_material=mats)
        sh.set_wire_material(torch.tensor([2, 2, 0, 0, 1, 1, 2, 2]), mask=torch.tensor([True] * 4 + [False] * 4))
        try:
            ShardedWireEDMEnv(8, device="cpu", backend=StubBackend, wire_material="brass")
            refused = ""
        except ValueError as exc:
            refused = str(exc)
        torch.save({"names": [m.name for m in sh.env.wire_materials], "index": sh.env.get_wire_material_index(),
                    "refused": refused}, f"{out}/rank{rank}.pt")
    finally:
        dist.destroy_process_group()


def test_shards_share_the_whole_batch_material_table(tmp_path):
    import socket

    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_shard_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt") for r in range(2))
    assert r0["names"] == r1["names"] == ["copper", "brass", "synthetic_host"]
    assert r0["index"].tolist() == [2, 2, 0, 0]  # the masked global switch: rank 0's range moved
    assert r1["index"].tolist() == [2, 1, 2, 1]  # rank 1's range kept its materials, indexed in the shared table
    assert "sequence" in r0["refused"] and "sequence" in r1["refused"]
