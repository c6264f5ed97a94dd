"""The wire profile (sparc_amd/profile.py) on the host side: the ABI mirror of ``wedm_profile_desc``
and the export with its status codes (no device is needed), `torch_wire_profile` against the definition written out in
tests/_wire_profile_ref.py, the environment's methods on the CPU oracle backends (which have no ``wire_profile`` and so
run the host path), the vector adapter's observation, and the refusals of host indices."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from sparc_amd import WireEDMVectorEnv, _abi, _lib
from sparc_amd.profile import profile_names, torch_wire_profile
from tests._snapshot_common import WINDOW, make, scenario
from tests._wire_profile_ref import bin_edges, pack, reference_rows, same_bits

ROOT = Path(__file__).resolve().parent.parent
N = 70
SEGMENTS = (1, 3, 4, 5, 13, 128, 401)
BINS = (0, 1, 3, 8, 64)


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_desc_struct_mirror_matches_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wedm_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(wedm_profile_desc));']
    for field, _ in _abi.ProfileDesc._fields_:
        lines.append(f'  printf("{field} %zu\\n", offsetof(wedm_profile_desc, {field}));')
    lines += ['  printf("consts %d %d %d %d abi %d\\n", WEDM_PROFILE_MAX_BINS, WEDM_PR_FIXED, WEDM_PROFILE_ROWS(0), '
              'WEDM_PROFILE_ROWS(8), WEDM_ABI_VERSION);',
              '  printf("fields %d %d %d %d\\n", WEDM_PR_ZONE_MEAN, WEDM_PR_WIRE_MEAN, WEDM_PR_WIRE_MAX, WEDM_PR_HOT_CELL);',
              "  return 0;", "}"]
    src = tmp_path / "desc.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "desc"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                   check=True)
    out = dict(row.split(" ", 1) for row in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("size")) == C.sizeof(_abi.ProfileDesc)
    assert out.pop("consts") == f"{_abi.PROFILE_MAX_BINS} {_abi.PR_FIXED} {_abi.profile_rows(0)} {_abi.profile_rows(8)} abi 4"
    assert (_abi.PROFILE_MAX_BINS, _abi.PR_FIXED, _abi.profile_rows(8), _abi.ABI_VERSION) == (64, 4, 20, 4)
    assert out.pop("fields") == " ".join(str(int(f)) for f in _abi.PR) == "0 1 2 3"
    assert {k: int(v) for k, v in out.items()} == {f: getattr(_abi.ProfileDesc, f).offset for f, _ in _abi.ProfileDesc._fields_}


def test_the_call_is_exported_and_refuses_bad_arguments_without_a_device():
    assert "wedm_wire_profile" in _lib.EXPORTS
    L = _lib.load()
    A = 0x10000   # never dereferenced: every call below returns before a launch

    def desc(**kw):
        f = dict(T=A, stride=128, num_envs=70, n_seg_max=13, n_seg=13, az_start=3, az_end=9, geom_i32=None, bins=8,
                 out=A + 0x100000, out_stride=64, out_cols=40)
        f.update(kw)
        return _abi.ProfileDesc(**f)

    def call(d, count=0, idx=None):
        return L.wedm_wire_profile(C.byref(d), idx, count, None, None)

    assert call(desc()) == _abi.OK                       # count == 0: checked, nothing launched
    assert call(desc(bins=0)) == _abi.OK and call(desc(bins=64)) == _abi.OK
    assert call(desc(geom_i32=A, n_seg=0)) == _abi.OK    # the uniform fields are not read with geometry rows
    assert call(desc(out_cols=64, stride=70)) == _abi.OK
    assert L.wedm_wire_profile(None, None, 0, None, None) == _abi.ERR_BAD_ARG
    for bad in (dict(T=None), dict(out=None), dict(T=A + 8), dict(T=A + 4), dict(bins=-1), dict(bins=65),
                dict(out_cols=65), dict(stride=69), dict(num_envs=0), dict(n_seg_max=0), dict(n_seg=0), dict(n_seg=14),
                dict(out_cols=-1)):
        assert call(desc(**bad)) == _abi.ERR_BAD_ARG, bad
        assert b"wedm_wire_profile" in L.wedm_last_error(None)
    assert call(desc(), count=-1) == _abi.ERR_BAD_ARG
    assert call(desc(), count=41) == _abi.ERR_BAD_ARG                                  # count > out_cols
    assert call(desc(out_stride=128, out_cols=128), count=71) == _abi.ERR_BAD_ARG      # no index list: count > num_envs
    assert call(desc(out_stride=128, out_cols=128, T=None), count=71, idx=A) == _abi.ERR_BAD_ARG


# ------------------------------------------------------------------------------------------------ the host path
def _random_case(rng, num_envs, n_max, per_env):
    """Cells in [250, 4000), geometry with every kind of zone: inside the wire, empty or reversed, past the wire's end,
    negative; tied maxima in every third environment (the same value at two or three cells)."""
    cells = rng.uniform(250.0, 4000.0, (num_envs, n_max)).astype(np.float32)
    n = rng.integers(1, n_max + 1, num_envs) if per_env else np.full(num_envs, n_max)
    if per_env:
        n[0], n[-1] = 1, n_max
    zs, ze = np.zeros(num_envs, dtype=np.int64), np.zeros(num_envs, dtype=np.int64)
    for e in range(num_envs):
        kind = e % 5
        a, b = sorted(rng.integers(0, n[e] + 1, 2))
        zs[e], ze[e] = ((a, b), (b, a), (a, n[e] + 1 + e % 3), (-1, b), (0, n[e]))[kind]
        if e % 3 == 0 and n[e] >= 2:
            spots = rng.choice(n[e], size=min(3, n[e]), replace=False)
            cells[e, spots] = np.float32(4000.5)
    if not per_env:
        zs[:], ze[:] = zs[1], ze[1]
    return cells, n, zs, ze


@pytest.mark.parametrize("per_env", [False, True])
@pytest.mark.parametrize("n_max", SEGMENTS)
def test_host_path_equals_the_definition(n_max, per_env):
    rng = np.random.default_rng(1000 * n_max + per_env)
    num_envs, stride = 11, 64
    zones = 1 if per_env else 4   # uniform geometry: one zone per draw, so several draws
    for _ in range(zones):
        cells, n, zs, ze = _random_case(rng, num_envs, n_max, per_env)
        T = torch.from_numpy(pack(cells, n, stride, dead=1.0e30))
        geom = (n, zs, ze) if per_env else (int(n[0]), int(zs[0]), int(ze[0]))
        for bins in BINS:
            got = torch_wire_profile(T, num_envs, *geom, bins).numpy()
            want = reference_rows(cells, n, zs, ze, bins)
            assert got.shape == (4 + 2 * bins, num_envs) and got.dtype == np.float32
            assert same_bits(got, want), (n_max, per_env, bins)
        ids = [10, 0, 0, 7]
        assert same_bits(torch_wire_profile(T, num_envs, *geom, 3, ids).numpy(), reference_rows(cells, n, zs, ze, 3, ids))


def test_tied_maxima_name_the_lowest_index_and_bins_tile_the_wire():
    t = np.full((1, 13), 300.0, dtype=np.float32)
    t[0, [4, 9, 12]] = 900.0
    rows = torch_wire_profile(torch.from_numpy(pack(t, 13, 64, dead=np.nan)), 1, 13, 0, 0, 8).numpy()[:, 0]
    assert rows[_abi.PR.HOT_CELL] == 4.0 and rows[_abi.PR.WIRE_MAX] == 900.0
    for n, bins in ((13, 8), (128, 8), (401, 64), (64, 64)):   # n >= bins: a partition
        e = bin_edges(n, bins)
        assert e[0][0] == 0 and e[-1][1] == n and all(a[1] == b[0] for a, b in zip(e, e[1:]))
    for n, bins in ((3, 8), (1, 64), (5, 64)):                 # n < bins: one cell each, every cell named
        e = bin_edges(n, bins)
        assert all(hi == lo + 1 for lo, hi in e) and {lo for lo, _ in e} == set(range(n))


# ------------------------------------------------------------------------------------------------ the environment
def _after_window(env):
    act = scenario(env)
    for k in WINDOW:
        env.step_many(act, k)
    return env


def _uniform_zone_mean_of_the_parent(env):
    g = env.geometry
    T = env.state.wire_temperature.tensor().t()
    return T[g.az_start: g.az_end].mean(dim=0) if g.az_end > g.az_start else T[: g.n_seg].mean(dim=0)


HEIGHTS = dict(workpiece_height=np.linspace(5.0, 40.0, N), wire_diameter=np.resize([0.1, 0.2, 0.3], N))
ENVS = {"plain-s128": ("plain", "s128", {}), "plain-s13": ("plain", "s13", {}), "wmat-s128": ("wmat", "s128", {}),
        "wmat-s13": ("wmat", "s13", {}), "autoreset-s128": ("autoreset", "s128", {}), "autoreset-s13": ("autoreset", "s13", {}),
        "heights": ("plain", "s128", HEIGHTS)}


@pytest.fixture(scope="module", params=sorted(ENVS))
def stepped(request):
    binding, geometry, kw = ENVS[request.param]
    return request.param, _after_window(make("cpu", N, binding, geometry, **kw))


def test_wire_max_is_the_states_maximum_and_the_profile_is_the_definition(stepped):
    """After 300 us of the snapshot tests' scenario: ``wire_max`` equals ``state.wire_max_temperature`` (what the kernels
    keep) cast to float32, for every environment, bit for bit; every row equals the definition on the environment's cells."""
    name, env = stepped
    prof = env.wire_profile()
    assert prof["rows"].shape == (20, N) and prof["bin_max"].shape == (8, N) and prof["zone_mean"].shape == (N,)
    assert same_bits(prof["wire_max"].numpy(), env.state.wire_max_temperature.to(torch.float32).numpy()), name
    assert len(set(prof["wire_max"].tolist())) > 10, "the scenario heats the wires, each its own way"
    if env.geometry is not None:
        geom = (env.geometry.n_seg, env.geometry.az_start, env.geometry.az_end)
    else:
        gi = env._geom_i32.numpy()[:, :N]
        geom = (gi[_abi.GI32.N_SEG], gi[_abi.GI32.AZ_START], gi[_abi.GI32.AZ_END])
    cells = env.state.wire_temperature.tensor().numpy()
    assert same_bits(prof["rows"].numpy(), reference_rows(cells, *geom, 8))
    assert same_bits(env.wire_profile(3, [5, 2, 2])["rows"].numpy(), reference_rows(cells, *geom, 3, [5, 2, 2]))


def test_zone_mean_temperature_for_every_geometry(stepped):
    """Uniform geometry: what the parent's expression returns, bit for bit.  Per-environment geometry and materials (where
    it raised ``NotImplementedError``): every environment's own zone, also as the ``wire_average_temperature`` signal."""
    name, env = stepped
    got = env.zone_mean_temperature()
    assert got.shape == (N,) and got.dtype == torch.float32
    if env.geometry is not None:
        assert same_bits(got.numpy(), _uniform_zone_mean_of_the_parent(env).numpy())
    else:
        gi = env._geom_i32.numpy()[:, :N]
        cells = env.state.wire_temperature.tensor().numpy()
        want = reference_rows(cells, gi[_abi.GI32.N_SEG], gi[_abi.GI32.AZ_START], gi[_abi.GI32.AZ_END], 0)[_abi.PR.ZONE_MEAN]
        assert same_bits(got.numpy(), want)
        if name == "heights":
            assert len(set(gi[_abi.GI32.N_SEG].tolist())) > 4, "wires of many lengths in one batch"
    assert same_bits(env.state.wire_average_temperature.numpy(), got.numpy())
    assert same_bits(env.wire.compute_zone_mean_temperature().numpy(), got.numpy())


# ------------------------------------------------------------------------------------------------ the vector adapter
def test_vector_env_appends_the_profile_to_the_observation():
    plain = WireEDMVectorEnv(make("cpu", 6, "plain", "s13"))
    env = make("cpu", 6, "plain", "s13")
    vec = WireEDMVectorEnv(env, wire_profile_bins=4)
    d = env.obs_dim
    assert vec.obs_names == tuple(env.obs_names) + profile_names(4) and len(vec.obs_names) == d + 12
    assert vec.obs_names[d: d + 5] == ("wire_zone_mean", "wire_mean", "wire_max", "wire_hot_cell", "wire_bin_max_0")
    assert vec.single_observation_space.shape == (d + 12,) and vec.observation_space.shape == (d + 12,)
    assert plain.obs_names == tuple(env.obs_names) and plain.single_observation_space.shape == (d,)
    o0, _ = plain.reset(seed=5)
    o1, _ = vec.reset(seed=5)
    assert o1.shape == (6, d + 12) and o1.dtype == torch.float32 and torch.equal(o1[:, :d], o0)
    for e in (plain.env, env):
        e.state.workpiece_position = torch.linspace(10.5, 14.0, 6, dtype=torch.float64)
        e.state.wire_position = 10.0
    action = env.make_action(0.0, 80.0, 9, 3.0, 30.0)
    for _ in range(2):
        a = plain.step(action)
        b = vec.step(action)
        assert b[0].shape == (6, d + 12) and torch.equal(b[0][:, :d], a[0])
        assert all(torch.equal(x, y) for x, y in zip(a[1:4], b[1:4]))
        assert same_bits(b[0][:, d:].numpy().T, env.wire_profile(4)["rows"].numpy())
        assert same_bits(b[0][:, d + 2].numpy(), env.state.wire_max_temperature.to(torch.float32).numpy())
    assert len(set(b[0][:, d + 2].tolist())) > 2, "the wires were heated"
    with pytest.raises(ValueError, match="bins must be an integer"):
        WireEDMVectorEnv(env, wire_profile_bins=65)


# ------------------------------------------------------------------------------------------------ refusals
def test_host_indices_and_bins_are_refused_before_anything_is_computed():
    env = make("cpu", 6, "plain", "s13")
    for call, match in ((lambda: env.wire_profile(8, [6]), "out of range"),
                        (lambda: env.wire_profile(8, [0, -1]), "out of range"),
                        (lambda: env.wire_profile(8, torch.tensor([0, 7])), "out of range"),
                        (lambda: env.wire_profile(8, [0.5]), "must be integers"),
                        (lambda: env.wire_profile(65), "bins must be an integer"),
                        (lambda: env.wire_profile(-1), "bins must be an integer"),
                        (lambda: env.wire_profile(2.5), "bins must be an integer")):
        with pytest.raises(ValueError, match=match):
            call()
    assert env.wire_profile(0)["rows"].shape == (4, 6) and env.wire_profile(8, [])["rows"].shape == (20, 0)
    assert env.wire_profile(8, np.array([3, 3, 1]))["bin_mean"].shape == (8, 3)
    env.check_errors()
