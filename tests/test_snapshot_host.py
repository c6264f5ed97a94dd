"""Snapshot, restore and fork of environment subsets (sparc_amd/snapshot.py) on the host side: the
three methods on the CPU oracle backends of tests/_oracle_backend.py and tests/_signal_oracle.py, which have no
``copy_columns`` and so run the plain-torch path; every refusal; the ABI mirror of ``wedm_copy_plane``; and the export with
its status codes (no device is needed for any of this)."""
from __future__ import annotations

import ctypes as C
import io
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from sparc_amd import EnvSnapshot, IgnitionModuleParameters, WireEDMEnv, WireEDMVectorEnv, _abi, _lib
from tests._oracle_backend import OracleBackend
from tests._snapshot_common import WINDOW, assert_same, copy_columns_numpy, diffs, everything, make, scenario
from tests._wmat_draw import BRASS, COPPER

ROOT = Path(__file__).resolve().parent.parent
N = 12
BINDINGS = ("plain", "pulse", "signal", "envp", "wmat", "crater", "autoreset")


def _prepared(binding, n=N, **kw):
    """An environment of the scenario, 150 us in (mid-interval, sparks behind it), with two environments about to reach
    their target at the next step: under ``autoreset`` they terminate in the window's first launch and are reset by its
    second."""
    env = make("cpu", n, binding, **kw)
    act = scenario(env)
    env.step_many(act, 150)
    for e in (1, 4):
        env.state.target_position[e] = env.state.workpiece_position[e]
    return env, act


def _window(env, act):
    for k in WINDOW:
        env.step_many(act, k)


@pytest.mark.parametrize("binding", BINDINGS)
def test_round_trip_and_replay(binding):
    """Snapshot all, 300 us, restore all: every block is what it was, byte for byte; the 300 us stepped again give the
    blocks they gave the first time.  A block or a row missing from the plane list changes the second run."""
    env, act = _prepared(binding)
    at_snapshot = everything(env)
    sparks = int(env.state.spark_count.sum())
    episode = env.state.episode.clone()
    snap = env.snapshot()
    assert snap.count == N and snap.stride == 64 and snap.blocks["f64"].shape == (_abi.F64_COUNT, 64)
    _window(env, act)
    first = everything(env)
    assert int(env.state.spark_count.sum()) > sparks and diffs(first, at_snapshot), "the window sparks and moves the state"
    assert bool(env.state.done.any()) or binding == "autoreset"
    if binding == "autoreset":
        assert bool((env.state.episode > episode).any()), "an environment terminated and was reset inside the window"
    if binding == "crater":
        assert bool((env.state.crater_log[:, :N] != 0).any())
    env.restore(snap)
    assert_same(everything(env), at_snapshot, "restored")
    _window(env, act)
    assert_same(everything(env), first, "replayed")


def test_fork_copies_every_block_and_leaves_sources_and_bystanders():
    """All bindings at once.  Destinations equal their sources in every block, in the env-param values and rows, the
    material index and the rows selected by it; one source feeds many destinations, a scalar source serves all."""
    env, act = _prepared("all")
    before = everything(env)
    env.fork([0, 1, 2], [5, 6, 7])
    env.fork(3, np.array([8, 9, 10, 11]))
    after = everything(env)
    src, dst = [0, 1, 2, 3, 3, 3, 3], [5, 6, 7, 8, 9, 10, 11]
    assert_same(after, after, "destinations", cols_got=dst, cols_want=src)
    assert_same(after, before, "sources and the bystander", cols_got=[0, 1, 2, 3, 4], cols_want=[0, 1, 2, 3, 4])
    pad = list(range(N, env.state.stride))
    names = [k for k in after if not k.startswith("_wmat") and k != "_geom_f64"]   # (their padding repeats the last environment)
    assert_same({k: after[k] for k in names}, {k: before[k] for k in names}, "padding columns", cols_got=pad, cols_want=pad)
    assert diffs(after, before, cols_got=dst, cols_want=dst), "the destinations changed"
    assert not torch.equal(before["_wmat_index"][:, 5], before["_wmat_index"][:, 0]), "a fork across materials"
    assert_same(after, copy_columns_numpy(before, src, dst), "against NumPy on the raw bytes",
                cols_got=list(range(N)), cols_want=list(range(N)))


@pytest.mark.parametrize("binding", ["plain", "signal"])
def test_a_forked_environment_continues_with_its_own_slots_random_stream(binding):
    """After 300 further us a destination at slot j equals a fresh environment that was given the same blocks and stepped
    at slot j: the Philox key and episode travel with the state, the counter holds the slot's id.  So the fork is not a
    replay of its source (an independent sample of the same state), and a restore into the source's own slot is."""
    env, act = _prepared(binding)
    src, dst = [0, 2, 2], [6, 8, 9]
    blocks = copy_columns_numpy(env.state.clone_blocks(), src, dst)
    env.fork(src, dst)
    fresh = make("cpu", N, binding)
    scenario(fresh)
    fresh.state.load_blocks(blocks)
    _window(env, act)
    _window(fresh, fresh.make_action(0.0, 80.0, 9, 3.0, 30.0))
    assert_same(everything(env), everything(fresh), "forked against freshly loaded")
    f64 = env.state.f64
    assert not torch.equal(f64[:, 8], f64[:, 2]) and not torch.equal(f64[:, 8], f64[:, 9]), "each slot drew its own variates"
    assert torch.equal(env.state.i32[_abi.I32.KEY_LO, dst], env.state.i32[_abi.I32.KEY_LO, src])


def test_subset_restore_with_permuted_columns_and_into_other_slots():
    env, act = _prepared("all")
    snap = env.snapshot([2, 5, 7, 9])
    assert snap.count == 4 and snap.env_ids.tolist() == [2, 5, 7, 9]
    at_snapshot = everything(env)
    _window(env, act)
    stepped = everything(env)
    env.restore(snap, env_ids=[9, 2], columns=[3, 0])
    got = everything(env)
    assert_same(got, at_snapshot, "restored", cols_got=[9, 2], cols_want=[9, 2])
    rest = [e for e in range(N) if e not in (9, 2)]
    assert_same(got, stepped, "the others", cols_got=rest, cols_want=rest)
    env.restore(snap, columns=torch.tensor([1, 2]))          # back where they came from: environments 5 and 7
    env.restore(snap, env_ids=np.array([0]), columns=[2])    # environment 7's state into slot 0
    got = everything(env)
    assert_same(got, at_snapshot, "defaults and another slot", cols_got=[5, 7, 0], cols_want=[5, 7, 7])
    env.restore(snap, env_ids=(3, 4))                        # columns default to 0 .. len(env_ids) - 1
    assert_same(everything(env), at_snapshot, cols_got=[3, 4], cols_want=[2, 5])


def test_a_snapshot_can_be_stored_and_loaded_with_weights_only():
    env, act = _prepared("all")
    snap = env.snapshot([1, 3])
    at_snapshot = everything(env)
    buf = io.BytesIO()
    torch.save(snap.to("cpu").state_dict(), buf)
    buf.seek(0)
    loaded = EnvSnapshot.from_state_dict(torch.load(buf, map_location="cpu", weights_only=True))
    _window(env, act)
    env.restore(loaded)
    assert_same(everything(env), at_snapshot, cols_got=[1, 3], cols_want=[1, 3])


def test_indices_are_refused_before_anything_is_copied():
    env, _ = _prepared("plain")
    before = everything(env)
    snap = env.snapshot([0, 1, 2])
    for call, match in (
            (lambda: env.fork([0, 1], [1, 2]), "both a source and a destination"),
            (lambda: env.fork([0, 1], [5, 5]), "must be distinct"),
            (lambda: env.fork([0], [N]), "out of range"),
            (lambda: env.fork([-1], [3]), "out of range"),
            (lambda: env.fork([0, 1], [3, 4, 5]), "2 sources for 3 destinations"),
            (lambda: env.fork([0.5], [3]), "must be integers"),
            (lambda: env.snapshot([N]), "out of range"),
            (lambda: env.restore(snap, env_ids=[4, 4], columns=[0, 1]), "must be distinct"),
            (lambda: env.restore(snap, env_ids=[4], columns=[3]), "snapshot column 3 out of range"),
            (lambda: env.restore(snap, env_ids=[N], columns=[0]), "out of range"),
            (lambda: env.restore(snap, env_ids=[1, 2], columns=[0]), "2 environments for 1 snapshot columns")):
        with pytest.raises(ValueError, match=match):
            call()
    with pytest.raises(TypeError):
        env.restore(env.state_dict())
    assert_same(everything(env), before, "nothing was copied")
    env.check_errors()   # host indices leave the device status word alone


def test_snapshots_of_another_environment_are_refused():
    env, _ = _prepared("plain")
    snap = env.snapshot()
    for other, match in (
            (make("cpu", N, "plain", geometry="s13"), "different shape: n_segments 128 against 13"),
            (make("cpu", N, "crater"), "different shape: crater_log_capacity 0 against 8"),
            (make("cpu", N, "pulse"), "different shape: obs_dim 8 against 11"),
            (make("cpu", N, "envp"), "optional blocks differ"),
            (make("cpu", N, "plain", ignition_params=IgnitionModuleParameters(hard_short_gap=1.5)), "different physics"),
            (make("cpu", N, "plain", env_id_offset=64), "different physics")):
        with pytest.raises(ValueError, match=match):
            other.restore(snap)
    stale = EnvSnapshot(dict(snap.meta, abi_version=3), snap.blocks, snap.env_ids)
    with pytest.raises(ValueError, match="state layout ABI 3"):
        env.restore(stale)
    wmat = make("cpu", N, "wmat")
    wsnap = wmat.snapshot()
    swapped = make("cpu", N, "wmat", wire_material=[(COPPER, BRASS)[k % 2] for k in range(N)])
    with pytest.raises(ValueError, match="material table differs"):
        swapped.restore(wsnap)
    with pytest.raises(ValueError, match="optional blocks differ"):
        env.restore(wsnap)
    # ... while another batch size of the same physics is the same kind of environment
    small = make("cpu", 5, "plain")
    scenario(small)
    small.restore(snap, env_ids=[4, 0], columns=[7, 11])
    assert_same(everything(small), everything(env), cols_got=[4, 0], cols_want=[7, 11])


def test_geometry_belongs_to_the_slot():
    """Per-environment geometry: a copy between slots of equal (height, diameter) passes, one between differing slots is
    refused, for fork and for restore."""
    h = np.array([10.0, 10.0, 20.0, 20.0, 10.0, 20.0])
    d = np.array([0.25, 0.25, 0.25, 0.2, 0.25, 0.2])
    env = WireEDMEnv(num_envs=6, device="cpu", backend=OracleBackend, workpiece_height=h, wire_diameter=d)
    act = scenario(env)
    env.step_many(act, 150)
    snap = env.snapshot([0, 3])
    assert snap.geometry.tolist() == [[10.0, 20.0], [0.25, 0.2]]
    before = everything(env)
    env.fork([0, 3], [4, 5])
    env.restore(snap, env_ids=[1, 5])
    assert_same(everything(env), before, cols_got=[4, 5, 1, 5], cols_want=[0, 3, 0, 3])
    for call in (lambda: env.fork([0], [2]), lambda: env.fork([2], [3]), lambda: env.restore(snap, env_ids=[2], columns=[0]),
                 lambda: env.restore(snap, env_ids=[2], columns=[1])):
        with pytest.raises(ValueError, match="geometry belongs to the slot"):
            call()
    same = WireEDMEnv(num_envs=6, device="cpu", backend=OracleBackend, workpiece_height=np.full(6, 12.0))
    assert same._geom_hd is None   # per-environment rows, one geometry: nothing to hold copies to
    same.fork([0], [5])


def test_vector_env_fork_copies_the_adapters_own_flags():
    env = make("cpu", N, "plain")
    vec = WireEDMVectorEnv(env)
    vec.reset(seed=3)
    vec._need_reset[torch.tensor([0, 2])] = True
    blocks = env.state.clone_blocks()
    vec.fork([0, 1], [5, 6])
    vec.fork(2, torch.tensor([7, 8]))
    assert vec._need_reset.tolist() == [e in (0, 2, 5, 7, 8) for e in range(N)]
    want = copy_columns_numpy(blocks, [0, 1, 2, 2], [5, 6, 7, 8])
    assert_same(env.state.clone_blocks(), want)


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_plane_struct_mirror_matches_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wedm_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(wedm_copy_plane));']
    for field, _ in _abi.CopyPlane._fields_:
        lines.append(f'  printf("{field} %zu\\n", offsetof(wedm_copy_plane, {field}));')
    lines += ['  printf("max_planes %d abi %d\\n", WEDM_COPY_MAX_PLANES, WEDM_ABI_VERSION);', "  return 0;", "}"]
    src = tmp_path / "plane.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "plane"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                   check=True)
    out = dict(row.split(" ", 1) for row in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("size")) == C.sizeof(_abi.CopyPlane) == 48
    assert out.pop("max_planes") == f"{_abi.COPY_MAX_PLANES} abi {_abi.ABI_VERSION}" and _abi.ABI_VERSION == 4
    assert {k: int(v) for k, v in out.items()} == {f: getattr(_abi.CopyPlane, f).offset for f, _ in _abi.CopyPlane._fields_}


def test_the_call_is_exported_and_refuses_bad_arguments_without_a_device():
    assert "wedm_copy_columns" in _lib.EXPORTS
    L = _lib.load()
    A = 0x10000   # never dereferenced: every call below returns before a launch

    def plane(**kw):
        f = dict(src=A, dst=A + 0x1000, rows=3, elem_bytes=8, src_stride=64, dst_stride=128, src_cols=64, dst_cols=70)
        f.update(kw)
        return _abi.CopyPlane(**f)

    def call(planes, n_planes=None, count=1, src=A, dst=A):
        arr = (_abi.CopyPlane * max(len(planes), 1))(*planes)
        return L.wedm_copy_columns(arr, len(planes) if n_planes is None else n_planes, src, dst, count, None, None)

    assert call([plane()], count=0) == _abi.OK
    assert call([plane(elem_bytes=w, rows=0) for w in (1, 4, 8, 16)], count=5) == _abi.OK   # no rows: nothing to launch
    assert call([plane()] * 16, count=0) == _abi.OK
    assert L.wedm_copy_columns(None, 1, A, A, 1, None, None) == _abi.ERR_BAD_ARG
    for bad in (dict(n_planes=0), dict(n_planes=17), dict(n_planes=-1), dict(count=-1), dict(src=None), dict(dst=None)):
        assert call([plane()], **bad) == _abi.ERR_BAD_ARG, bad
    for bad in (dict(elem_bytes=2), dict(elem_bytes=0), dict(elem_bytes=32), dict(src=A + 4), dict(dst=A + 1),
                dict(elem_bytes=16, src=A + 8), dict(elem_bytes=4, dst=A + 2), dict(src=None), dict(dst=None), dict(rows=-1),
                dict(src_stride=63), dict(dst_stride=69), dict(src_cols=-1), dict(dst_cols=-1)):
        assert call([plane(), plane(**bad)]) == _abi.ERR_BAD_ARG, bad
        assert call([plane(**bad)], count=0) == _abi.ERR_BAD_ARG, bad
        assert b"wedm_copy_columns" in L.wedm_last_error(None)
    assert call([plane(elem_bytes=1, src=A + 3, dst=A + 5)], count=0) == _abi.OK
