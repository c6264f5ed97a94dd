"""Seeded per-episode domain randomisation without a GPU: the host path of
`sparc_amd.randomize.EpisodeSampler` (what a backend without ``draw_episode`` runs, and what the kernel is checked against)
bit for bit against the independent definition of `tests._episode_draw_ref`; the properties of a draw; its invariance under
batch size, offset and masking; checkpoints; refusals; and the adapter on the CPU oracle backend."""
from __future__ import annotations

import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from sparc_amd import (EnvironmentConfig, EpisodeSampler, WireEDMEnv, WireEDMVectorEnv, WireModuleParameters, _abi, _lib,
                       uniform_param_sampler)
from sparc_amd.core import env_params as envp
from sparc_amd.core.material_db import WireMaterial
from sparc_amd.randomize import philox4x32_10
from tests import _episode_draw_ref as ref
from tests import _geometry_ref as gref
from tests._oracle_backend import OracleBackendRows

ROOT = Path(__file__).resolve().parents[1]
WIRE = WireModuleParameters(buffer_len_bottom=2.0, buffer_len_top=2.0, contact_offset_bottom=1.0, contact_offset_top=1.0)
DIAMETERS = (0.1, 0.2, 0.25)
MATERIALS = [gref.BRASS, gref.COPPER,
             WireMaterial(name="steel", density=7850, specific_heat=490, thermal_conductivity=45, electrical_resistivity=1.7e-07,
                          temperature_coefficient=0.005, melting_point=1700, breaking_temperature=1900),
             WireMaterial(name="moly", density=10220, specific_heat=251, thermal_conductivity=138, electrical_resistivity=5.3e-08,
                          temperature_coefficient=0.0047, melting_point=2896, breaking_temperature=3000)]
DEFAULTS = {'base_critical_density': 0.3, 'gap_coefficient': 0.02, 'max_critical_density': 0.95, 'hard_short_gap': 2.0,
            'sigmoid_steepness': 500.0, 'spark_voltage_factor': 0.3, 'debris_removal_efficiency': 0.01,
            'dielectric_temperature': 293.15, 'plasma_efficiency': 0.1, 'base_convection_coefficient': 14000.0, 'omega_n': 235.0,
            'zeta': 0.38, 'max_acceleration': 300000.0, 'max_jerk': 100000000.0, 'max_speed': 30000.0}
assert tuple(DEFAULTS) == envp.NAMES
# ranges around the dataclass values: every name, so that every Philox call and every derived row takes part
RANGES = {name: (0.8 * v, 1.25 * v) for name, v in DEFAULTS.items()}
HEIGHT = (1.0, 10.0)
N = 12
SEED = 0x1234_5678_9ABC_DEF0


def build(n=N, materials=4, diameters=3, dynamic=True, offset=0, params=True, **kw):
    """An environment on the CPU oracle backend with every per-environment block the sampler can write."""
    kw.setdefault("config", EnvironmentConfig(target_cutting_distance=5000.0))
    if params:
        kw["env_params"] = dict(DEFAULTS)
    if materials:
        kw["wire_material"] = [MATERIALS[k % materials] for k in range(n)]
        kw["wire_material_table"] = MATERIALS[:materials]
    if dynamic:
        kw["dynamic_geometry"] = {"max_workpiece_height": 10.0, "wire_diameters": DIAMETERS[:diameters]}
        kw["wire_diameter"] = np.resize(DIAMETERS[:diameters], n)
    return WireEDMEnv(num_envs=n, device="cpu", backend=OracleBackendRows, wire_params=WIRE, env_id_offset=offset,
                      workpiece_height=np.linspace(1.5, 9.5, n), **kw)


def spec_of(group, materials, diameters):
    """(keyword arguments of EpisodeSampler, the reference's spec) of a slot group."""
    kw, spec = {}, {"params": {}}
    if group in ("params", "all"):
        kw["params"] = spec["params"] = RANGES
    if group == "damping":  # one operand drawn, the other read from the source rows
        kw["params"] = spec["params"] = {"zeta": RANGES["zeta"], "max_speed": RANGES["max_speed"]}
    if group in ("materials", "all") and materials:
        kw["materials"], spec["materials"] = True, materials
    if group in ("geometry", "all"):
        kw["height"], spec["height"] = HEIGHT, HEIGHT
        kw["diameters"], spec["diameters"] = True, diameters
    if group == "height":
        kw["height"], spec["height"] = HEIGHT, HEIGHT
    return kw, spec


def blocks_of(env, sampler) -> dict:
    """NumPy views of everything the call may touch (CPU tensors share their memory)."""
    b = {"count": sampler._count.numpy()}
    if env._envp_src is not None:
        b.update(envp_src=env._envp_src.numpy(), envp_rows=env._envp_rows.numpy())
    if env._wmat_rows is not None:
        b.update(mat_index=env._wmat_index.numpy(), wmat_rows=env._wmat_rows.numpy(), wmat_table=env._wmat_table.numpy())
        if env._wmat_geom_table is not None:
            b["wmat_geom_table"] = env._wmat_geom_table.numpy()
    if env.per_env_geometry:
        b.update(geom_f64=env._geom_f64.numpy(), geom_i32=env._geom_i32.numpy())
    if env._dyn is not None:
        b.update(height=env._dyn.height.numpy(), dia=env._dyn.dia.numpy())
    return b


WRITTEN = ("count", "envp_src", "envp_rows", "mat_index", "wmat_rows", "geom_f64", "geom_i32", "height", "dia")


def geom_of(env):
    dyn = env._dyn
    return None if dyn is None else {"wire": env.wire_params, "combo": dyn.combo_host, "n_diameters": len(dyn.diameters),
                                     "n_seg_max": dyn.n_seg_max}


def masks(n):
    one = np.zeros(n, dtype=bool)
    one[n // 2] = True
    return {"none": None, "zero": np.zeros(n, dtype=bool), "alternating": np.arange(n) % 2 == 0, "single": one}


def check_draw(env, sampler, spec, mask, draws=2):
    """`draws` draws under `mask` with poison in every column the call must not touch: every block equals the reference's."""
    n = env.num_envs
    sampler.bind(env)
    b = blocks_of(env, sampler)
    asked = np.ones(n, dtype=bool) if mask is None else mask
    keep = np.concatenate([~asked, np.ones(b["count"].shape[0] - n, dtype=bool)])  # unmasked and padding columns
    for name in WRITTEN:
        if name in b:
            b[name][..., keep] = ref.poisoned(b[name][..., keep].shape, b[name].dtype)
    consts = env._envp_consts()
    for _ in range(draws):
        want = {name: a.copy() for name, a in b.items()}
        counts = b["count"].copy()
        status = ref.draw_columns(want, spec, sampler.seed, env.env_id_offset, n, mask, consts, geom_of(env))
        sampler.draw(env, mask=None if mask is None else torch.from_numpy(mask), reset=False)
        assert status == 0 and (env._dyn is None or int(env._dyn.status.item()) == 0)
        for name in WRITTEN:
            if name in b:
                assert b[name].tobytes() == want[name].tobytes(), name
                assert ref.is_poison(b[name][..., keep]), name
        assert np.array_equal(b["count"][:n][asked], counts[:n][asked] + 1)


# ------------------------------------------------------------------------------------------------ the generator
def test_product_philox_equals_the_oracle_library():
    rng = np.random.default_rng(11)
    ctr = rng.integers(0, 2 ** 32, (1000, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, (1000, 2), dtype=np.uint64)
    ctr[:4] = [[0, 0, 0, 0], [2 ** 32 - 1] * 4, [0, 0, 2 ** 31 + 5, 0x80000004], [1, 0, 0, 0x80000000]]
    for i in range(1000):  # one key per call of the product function
        got = philox4x32_10(tuple(ctr[i]), (int(key[i, 0]), int(key[i, 1])))
        assert tuple(int(w) for w in got) == orc.philox([int(c) for c in ctr[i]], [int(k) for k in key[i]]), i
    # and vectorised over the counter, as the host path calls it
    got = np.stack(philox4x32_10((ctr[:, 0], 0, ctr[:, 2], 0x80000001), (7, 9)), axis=1)
    for i in range(0, 1000, 50):
        assert tuple(int(w) for w in got[i]) == orc.philox([int(ctr[i, 0]), 0, int(ctr[i, 2]), 0x80000001], [7, 9])


# ------------------------------------------------------------------------------------------------ host path == reference
@pytest.mark.parametrize("mask_name", ["none", "zero", "alternating", "single"])
@pytest.mark.parametrize("group", ["params", "damping", "materials", "geometry", "height", "all"])
def test_host_path_equals_the_reference_in_every_written_block(group, mask_name):
    env = build()
    kw, spec = spec_of(group, 4, 3)
    check_draw(env, EpisodeSampler(SEED, **kw), spec, masks(N)[mask_name])


@pytest.mark.parametrize("materials, diameters", [(1, 1), (1, 3), (4, 1)])
def test_host_path_equals_the_reference_with_one_material_or_one_diameter(materials, diameters):
    env = build(materials=materials, diameters=diameters)
    for group in ("materials", "geometry", "all"):
        kw, spec = spec_of(group, materials, diameters)
        check_draw(env, EpisodeSampler(SEED + 1, **kw), spec, masks(N)["alternating"], draws=1)


@pytest.mark.parametrize("layout", ["static geometry", "no material", "params only"])
def test_host_path_equals_the_reference_in_the_other_layouts(layout):
    """Materials with the geometry rows selected from the per-material table (no dynamic geometry); dynamic geometry
    without a material block (material 0); an environment with nothing but physics parameters, at a large offset."""
    if layout == "static geometry":
        env, (kw, spec) = build(dynamic=False), spec_of("materials", 4, 0)
        kw["params"] = spec["params"] = {"omega_n": RANGES["omega_n"]}
    elif layout == "no material":
        env, (kw, spec) = build(materials=0), spec_of("geometry", 0, 3)
    else:
        env = WireEDMEnv(num_envs=N, device="cpu", backend=OracleBackendRows, env_params=dict(DEFAULTS),
                         env_id_offset=2 ** 31 + 5)
        kw, spec = spec_of("params", 0, 0)
    for mask_name in ("none", "alternating"):
        check_draw(env, EpisodeSampler(3, **kw), spec, masks(N)[mask_name])


# ------------------------------------------------------------------------------------------------ properties of a draw
def test_derived_rows_omega_n_and_ranges():
    env = build(n=64)
    s = EpisodeSampler(21, params=RANGES)
    s.draw(env, reset=False)
    src = {name: env._envp_src[envp.INDEX[name], :64] for name in envp.NAMES}
    assert torch.equal(envp.derive_rows(src, env._envp_consts()), env._envp_rows[:, :64])
    host = {name: t.numpy() for name, t in src.items()}
    assert np.array_equal(envp.derive_rows(host, env._envp_consts()), env._envp_rows[:, :64].numpy())  # Python floats, C pow
    w = src["omega_n"].numpy()
    assert (w.view(np.int64) & ((1 << 27) - 1) == 0).all() and len(set(w.tolist())) > 32
    assert env._envp_rows[_abi.ENVP.STIFFNESS_COEFF, :64].tolist() == [-(x ** 2) for x in w.tolist()]
    big = s.expected(np.arange(4096), np.arange(4096) % 7)
    for name, (lo, hi) in RANGES.items():
        assert ((lo <= big[name]) & (big[name] <= hi)).all(), name
    assert (big["omega_n"].view(np.int64) & ((1 << 27) - 1) == 0).all()
    # lo == hi, and a range of one ulp
    up = float(np.nextafter(3.0, 4.0))
    tight = EpisodeSampler(5, params={"zeta": (0.38, 0.38), "max_speed": (3.0, up)}, height=(2.5, 2.5))
    got = tight.expected(np.arange(512), 3)
    assert (got["zeta"] == 0.38).all() and (got["workpiece_height"] == 2.5).all()
    assert set(got["max_speed"].tolist()) <= {3.0, up}


def test_every_choice_occurs():
    got = EpisodeSampler(9, materials=3, diameters=3).expected(np.arange(4096), 0)
    for key in ("wire_material", "wire_diameter_index"):
        assert sorted(set(got[key].tolist())) == [0, 1, 2], key
        assert np.bincount(got[key]).min() > 4096 // 3 - 200
    assert (got["wire_material"] != got["wire_diameter_index"]).any()  # two slots, two words
    one = EpisodeSampler(9, materials=1).expected(np.arange(256), np.arange(256))
    assert (one["wire_material"] == 0).all()


def test_enabling_another_slot_changes_no_other_draw():
    ids, k = np.arange(200) + 2 ** 31, np.arange(200) % 5
    full = EpisodeSampler(77, params=RANGES, materials=4, height=HEIGHT, diameters=3).expected(ids, k)
    for name in ("omega_n", "max_speed"):
        assert np.array_equal(EpisodeSampler(77, params={name: RANGES[name]}).expected(ids, k)[name], full[name])
    assert np.array_equal(EpisodeSampler(77, materials=4).expected(ids, k)["wire_material"], full["wire_material"])
    assert np.array_equal(EpisodeSampler(77, height=HEIGHT).expected(ids, k)["workpiece_height"], full["workpiece_height"])
    assert np.array_equal(EpisodeSampler(77, diameters=3).expected(ids, k)["wire_diameter_index"], full["wire_diameter_index"])
    assert not np.array_equal(EpisodeSampler(78, height=HEIGHT).expected(ids, k)["workpiece_height"], full["workpiece_height"])
    # the reference's scalar definition, at ids and draw numbers past 2^31
    spec = {"params": RANGES, "materials": 4, "height": HEIGHT, "diameters": 3}
    for i in (0, 7, 199):
        want = ref.values(spec, 77, int(ids[i]), int(k[i]))
        assert {key: full[key][i] for key in want} == want


def reported(env):
    out = {name: t.numpy() for name, t in env.get_env_params().items()}
    out["wire_material"] = env.get_wire_material_index().numpy()
    g = env.get_geometry()
    out.update(workpiece_height=g["workpiece_height"].numpy(), wire_diameter=g["wire_diameter"].numpy())
    return out


def assert_holds(env, sampler, draw_numbers, where=None):
    """Every environment (of `where`) reports what `expected` says for its global id at its draw number."""
    n = env.num_envs
    want = sampler.expected(env.env_id_offset + np.arange(n), draw_numbers)
    got = reported(env)
    sel = np.ones(n, dtype=bool) if where is None else where
    assert set(want) - {"wire_diameter_index"} <= set(got)
    for key, v in want.items():
        if key != "wire_diameter_index":
            assert got[key][sel].tobytes() == v[sel].astype(got[key].dtype).tobytes(), key
    assert np.array_equal(env._dyn.dia[:n].numpy()[sel], want["wire_diameter_index"][sel])


def test_expected_equals_what_the_environment_reports():
    env = build(offset=1000)
    s = EpisodeSampler(SEED, params=RANGES, materials=True, height=HEIGHT, diameters=True)
    with pytest.raises(RuntimeError, match="bind"):
        s.expected(0, 0)  # how many materials there are is the environment's
    s.draw(env)
    assert_holds(env, s, 0)
    m = masks(N)["alternating"]
    s.draw(env, mask=m)
    assert_holds(env, s, np.where(m, 1, 0))
    assert s.draw_counts().tolist() == np.where(m, 2, 1).tolist()
    env.check_errors()
    # the same numbers without an environment
    free = EpisodeSampler(SEED, params=RANGES, materials=4, height=HEIGHT, diameters=3)
    a, b = free.expected(1000 + np.arange(N), 1), s.expected(1000 + np.arange(N), 1)
    assert all(np.array_equal(a[key], b[key]) for key in a)


# ------------------------------------------------------------------------------------------------ invariance
def rows_of(env, lo=0, hi=None):
    hi = env.num_envs if hi is None else hi
    return [t[..., lo:hi].clone() for t in (env._envp_src, env._envp_rows, env._wmat_index, env._wmat_rows, env._geom_f64,
                                            env._geom_i32, env._dyn.height, env._dyn.dia)]


def all_slots(seed=SEED):
    return EpisodeSampler(seed, params=RANGES, materials=True, height=HEIGHT, diameters=True)


def test_a_draw_does_not_depend_on_batch_size_offset_or_masking():
    whole, left, right, wide, halves = build(96), build(48), build(48, offset=48), build(160), build(96)
    first = np.arange(96) < 40
    for env, steps in ((whole, [None, None]), (left, [None, None]), (right, [None, None]), (wide, [None, None]),
                       (halves, [first, ~first, ~first, first])):
        s = all_slots()
        for mask in steps:
            s.draw(env, mask=mask, reset=False)
        env.check_errors()
    want = rows_of(whole)
    for got in ([torch.cat([a, b], dim=-1) for a, b in zip(rows_of(left), rows_of(right))], rows_of(wide, 0, 96), rows_of(halves)):
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    assert not torch.equal(rows_of(wide, 96, 160)[0][:, :64], want[0][:, :64])


def test_state_dict_round_trip_continues_the_sequence():
    a, b = build(), build()
    sa = all_slots()
    for mask in (None, masks(N)["alternating"], masks(N)["single"]):
        sa.draw(a, mask=mask, reset=False)
    sd = sa.state_dict()
    assert sd["seed"] == SEED and sd["draw_count"].tolist() == [2 + (e == N // 2) if e % 2 == 0 else 1 for e in range(N)]
    sb = all_slots(seed=1)
    sb.load_state_dict(sd)  # before the first use: applied when it is bound
    late = all_slots(seed=2)
    late.bind(b)
    for s in (sa, sb):
        s.draw(a if s is sa else b, reset=False)
    for x, y in zip(rows_of(a), rows_of(b)):
        assert torch.equal(x, y)
    assert torch.equal(sa.draw_counts(), sb.draw_counts())
    c = build()
    late2 = all_slots(seed=2)
    late2.bind(c)
    late2.load_state_dict(sd)  # after binding
    late2.draw(c, reset=False)
    assert torch.equal(rows_of(c)[0], rows_of(a)[0]) and torch.equal(late2.draw_counts(), sa.draw_counts())
    # another spec, another batch
    with pytest.raises(ValueError, match="other names or from other ranges"):
        EpisodeSampler(SEED, params=RANGES, materials=4, height=(1.0, 9.0), diameters=3).load_state_dict(sd)
    with pytest.raises(ValueError, match="other names or from other ranges"):
        EpisodeSampler(SEED, params=RANGES, materials=4, height=HEIGHT).load_state_dict(sd)
    other = all_slots()
    other.bind(build(n=8))
    with pytest.raises(ValueError, match="draw counts are for 12"):
        other.load_state_dict(sd)
    # reseed: draw 0 of the new seed
    sa.reseed(5)
    assert sa.draw_counts().tolist() == [0] * N
    sa.draw(a, reset=False)
    fresh = all_slots(seed=5)
    fresh.draw(b, reset=False)
    for x, y in zip(rows_of(a), rows_of(b)):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    with pytest.raises(ValueError, match="unknown per-environment parameter"):
        EpisodeSampler(0, params={"omega": (1.0, 2.0)})
    for bad in ((2.0, 1.0), (float("nan"), 1.0), (0.0, float("inf"))):
        with pytest.raises(ValueError, match="finite with low <= high"):
            EpisodeSampler(0, params={"zeta": bad})
        with pytest.raises(ValueError, match="finite with low <= high"):
            EpisodeSampler(0, height=bad)
    with pytest.raises(ValueError, match="0 < low"):
        EpisodeSampler(0, height=(0.0, 5.0))
    with pytest.raises(ValueError, match="positive number"):
        EpisodeSampler(0, materials=0)
    env = build()
    with pytest.raises(ValueError, match="above max_workpiece_height"):
        EpisodeSampler(0, height=(1.0, 10.5)).bind(env)
    EpisodeSampler(0, height=(1.0, 10.0)).bind(env)
    with pytest.raises(ValueError, match="diameters=2"):
        EpisodeSampler(0, diameters=2).bind(env)
    with pytest.raises(ValueError, match="materials=3"):
        EpisodeSampler(0, materials=3).bind(env)
    # a name outside the environment's env_params
    few = WireEDMEnv(num_envs=N, device="cpu", backend=OracleBackendRows, env_params={"zeta": 0.4})
    with pytest.raises(ValueError, match="not randomised in this environment"):
        EpisodeSampler(0, params={"omega_n": RANGES["omega_n"]}).bind(few)
    with pytest.raises(ValueError, match="wire_material"):
        EpisodeSampler(0, materials=True).draw(few)
    for kw in (dict(height=HEIGHT), dict(diameters=True)):
        with pytest.raises(ValueError, match="dynamic_geometry"):
            EpisodeSampler(0, **kw).bind(few)
    with pytest.raises(ValueError, match="dynamic_geometry"):
        EpisodeSampler(0, height=HEIGHT).bind(build(dynamic=False))
    # one sampler, one environment
    s = EpisodeSampler(0, params={"zeta": RANGES["zeta"]})
    s.bind(few)
    with pytest.raises(ValueError, match="another environment"):
        s.bind(env)
    # the adapter
    with pytest.raises(ValueError, match="give either"):
        WireEDMVectorEnv(env, episode_sampler=all_slots(), param_sampler=uniform_param_sampler({"zeta": (0.3, 0.4)}))
    vec = WireEDMVectorEnv(env, episode_sampler=all_slots())
    with pytest.raises(ValueError, match="no mask"):
        vec.reset(seed=4, options={"mask": masks(N)["alternating"]})
    with pytest.raises(ValueError, match="one entry per environment"):
        vec.reset(options={"mask": np.ones(N + 1, dtype=bool)})
    vec.reset(options={"mask": masks(N)["alternating"]})
    vec.reset(seed=4)


# ------------------------------------------------------------------------------------------------ the ABI mirror
def test_header_declares_and_library_exports_the_call():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "wedm_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bwedm_draw_episode\s*\(", text) and "wedm_draw_desc" in text
    assert "#define WEDM_ABI_VERSION 4" in text
    assert "wedm_draw_episode" in _lib.EXPORTS and hasattr(_lib.HipBackend, "draw_episode")
    L = _lib.load()
    assert L.wedm_draw_episode(None, None, None, None) == _abi.ERR_BAD_ARG
    assert b"wedm_draw_episode: null descriptor" in L.wedm_last_error(None)
    d = _abi.DrawDesc(num_envs=4, stride=2)
    assert L.wedm_draw_episode(C.byref(d), None, 8, None) == _abi.ERR_BAD_ARG
    assert b"stride smaller than num_envs" in L.wedm_last_error(None)
    # the slots are the names of env_params, in their order
    body = re.search(r"enum wedm_draw_slot_id \{(.*?)\};", text, flags=re.S).group(1)
    names = [n.strip().split("=")[0].strip() for n in body.split(",") if n.strip()]
    assert names == ["WEDM_DS_" + n.upper() for n in envp.NAMES] + ["WEDM_DS_MATERIAL", "WEDM_DS_HEIGHT", "WEDM_DS_DIAMETER",
                                                                   "WEDM_DRAW_SLOTS"]
    assert (_abi.DRAW_ENVP_SLOTS, _abi.DRAW_SLOT_MATERIAL, _abi.DRAW_SLOT_HEIGHT, _abi.DRAW_SLOT_DIAMETER, _abi.DRAW_SLOTS) == \
        (len(envp.NAMES), 15, 16, 17, 18)
    assert (ref.SLOT_MATERIAL, ref.SLOT_HEIGHT, ref.SLOT_DIAMETER) == (15, 16, 17)


def test_bad_arguments_are_refused_before_anything_is_launched():
    """Every pointer below is an address nobody owns: each case returns WEDM_ERR_BAD_ARG with exactly this text."""
    L = _lib.load()
    uniform, choice = _abi.DRAW_UNIFORM, _abi.DRAW_CHOICE

    def answer(draw_count=8, slots={}, **kw):
        d = _abi.DrawDesc(**dict(dict(num_envs=4, stride=4), **kw))
        for s, fields in slots.items():
            for name, value in fields.items():
                setattr(d.slot[s], name, value)
        rc = L.wedm_draw_episode(C.byref(d), None, draw_count, None)
        return rc, L.wedm_last_error(None).decode()

    unit = dict(kind=uniform, lo=0.0, hi=1.0, span=1.0)
    for kw, text in ((dict(draw_count=None), "draw_count is null or not aligned to its element"),
                     (dict(draw_count=6), "draw_count is null or not aligned to its element"),
                     (dict(num_envs=0), "num_envs must be positive"),
                     (dict(dynamic=2), "dynamic must be 0 or 1"),
                     (dict(slots={0: dict(kind=choice, k=2)}), "slot 0: a kind this slot does not take"),
                     (dict(slots={15: dict(kind=choice, k=0)}), "slot 15: a choice needs k >= 1"),
                     (dict(slots={3: dict(unit, lo=float("inf"))}), "slot 3: bounds must be finite"),
                     (dict(slots={3: dict(unit, lo=2.0)}), "slot 3: lo > hi"),
                     (dict(slots={0: unit}), "envp_src or envp_rows is null or misaligned"),
                     (dict(slots={0: unit}, envp_src=8, envp_rows=8, dt_s=float("nan")), "base_flow_rate and dt_s must be finite"),
                     (dict(slots={15: dict(kind=choice, k=2)}), "material_index, wmat_table or wmat_rows is null or misaligned"),
                     (dict(slots={16: unit}), "height and diameter are drawn with dynamic geometry only"),
                     (dict(slots={16: unit}, dynamic=1), "geom: null combination table or geometry block")):
        assert answer(**kw) == (_abi.ERR_BAD_ARG, "wedm_draw_episode: " + text), kw


def test_descriptor_mirrors_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wedm_hip.h"', "int main(void) {"]
    for cname, mirror in (("wedm_draw_slot", _abi.DrawSlot), ("wedm_draw_desc", _abi.DrawDesc)):
        lines.append(f'  printf("{cname}.size %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{field} %zu\\n", offsetof({cname}, {field}));' for field, _ in mirror._fields_]
    lines += ['  printf("stream0 %u\\n", WEDM_DRAW_STREAM0);',
              '  printf("kinds %d\\n", WEDM_DRAW_NONE + 10 * WEDM_DRAW_UNIFORM + 100 * WEDM_DRAW_CHOICE);', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                   check=True)
    out = dict(row.split() for row in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("stream0")) == _abi.DRAW_STREAM0
    assert int(out.pop("kinds")) == _abi.DRAW_NONE + 10 * _abi.DRAW_UNIFORM + 100 * _abi.DRAW_CHOICE
    for cname, mirror in (("wedm_draw_slot", _abi.DrawSlot), ("wedm_draw_desc", _abi.DrawDesc)):
        assert C.sizeof(mirror) == int(out.pop(f"{cname}.size"))
        assert {f: getattr(mirror, f).offset for f, _ in mirror._fields_} == \
            {k.split(".")[1]: int(v) for k, v in out.items() if k.startswith(cname + ".")}


# ------------------------------------------------------------------------------------------------ the adapter
def test_vector_adapter_gives_every_new_episode_its_expected_draw():
    """Ten control steps with short episodes on the oracle backend (the adapter's own masked reset): after each step every
    environment holds `expected` of its global id at the episode it is in, whichever step it began in."""
    env = build(offset=500, config=EnvironmentConfig(target_cutting_distance=50.01))  # 10 nm past the initial gap
    s = all_slots()
    vec = WireEDMVectorEnv(env, episode_sampler=s)
    vec.reset(seed=2)
    assert s.seed == 2
    assert_holds(env, s, 0)
    act = env.make_action(0.5, 80.0, 9, 3.0, 30.0)
    episode = np.zeros(N, dtype=np.int64)
    seen = np.zeros(N, dtype=bool)
    for _ in range(10):
        due = vec._need_reset.numpy().copy()
        before = reported(env)
        vec.step(act)
        episode += due
        seen |= due
        assert_holds(env, s, episode)
        after = reported(env)
        for key in before:
            assert before[key][~due].tobytes() == after[key][~due].tobytes(), key
        assert (before["workpiece_height"][due] != after["workpiece_height"][due]).all()
        assert s.draw_counts().tolist() == (episode + 1).tolist()
        assert torch.equal(vec.episode_count, torch.from_numpy(episode))
    assert seen.any() and not seen.all() and episode.max() >= 2
    env.check_errors()
    # fork: the destination keeps its own stream of draws
    counts = s.draw_counts().clone()
    vec.fork([0], [1])
    assert torch.equal(s.draw_counts(), counts)
    # a masked reset draws for the masked environments only; a seed starts everyone at draw 0 of the new seed
    m = masks(N)["single"]
    vec.reset(options={"mask": m})
    assert_holds(env, s, episode + 1, where=m)
    assert s.draw_counts().tolist() == (episode + 1 + m).tolist()
    vec.reset(seed=9)
    assert_holds(env, s, 0)
    assert not np.array_equal(s.expected(500 + np.arange(N), 0)["omega_n"], all_slots(2).bind(build()).expected(500 + np.arange(N), 0)["omega_n"])
