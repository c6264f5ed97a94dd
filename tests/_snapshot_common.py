"""What tests/test_snapshot_host.py (CPU oracle backend, the torch path) and tests/test_snapshot.py (MI355X, the kernel)
share: the environments of every binding that adds state, the scenario, and byte-for-byte comparison of everything a
snapshot, restore or fork has to move.  TEST SEAM ONLY."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from sparc_amd import EnvironmentConfig, WireEDMEnv, WireModuleParameters
from tests._oracle_backend import OracleBackend
from tests._signal_oracle import SignalOracleBackend
from tests._wmat_draw import BRASS, COPPER

# segments of the wire: 128 (32 whole quads) and 13 (the fourth quad holds one cell and three of padding)
GEOMETRY = {"s128": dict(wire_params=WireModuleParameters(segment_len=0.625)),
            "s13": dict(wire_params=WireModuleParameters(segment_len=6.1))}
WINDOW = (100, 1, 199)   # the 300 us of the round-trip and replay tests, as three launches (an autoreset needs a second one)


def binding_kw(binding: str, n: int) -> dict:
    """Constructor keywords of every binding that adds state to an environment."""
    rng = np.random.default_rng(3)
    envp = dict(hard_short_gap=rng.uniform(0.5, 3.0, n), plasma_efficiency=rng.uniform(0.05, 0.2, n),
                dielectric_temperature=rng.uniform(290.0, 310.0, n), max_speed=rng.uniform(2.0e4, 4.0e4, n))
    mats = [(BRASS, COPPER)[k % 2] for k in range(n)]
    return {"plain": {}, "pulse": dict(pulse_stats=True), "signal": dict(signal_stats=True), "envp": dict(env_params=envp),
            "wmat": dict(wire_material=mats), "crater": dict(crater_log_capacity=8),
            "autoreset": dict(autoreset=True, reward="progress"),
            "all": dict(pulse_stats=True, signal_stats=True, env_params=envp, wire_material=mats, crater_log_capacity=8)}[binding]


def make(device: str, n: int, binding: str = "plain", geometry: str = "s128", **kw) -> WireEDMEnv:
    kw = {**GEOMETRY[geometry], **binding_kw(binding, n), **kw}
    kw.setdefault("config", EnvironmentConfig(target_cutting_distance=5000.0))
    if device == "cpu":
        kw["backend"] = OracleBackend if binding in ("plain", "crater", "autoreset") else SignalOracleBackend
    return WireEDMEnv(num_envs=n, device=device, **kw)


def scenario(env, seed: int = 77):
    """The scenario of tests/test_signal_stats.py at any batch size: gaps from a hard short to an idle 15 um, so the batch
    sparks; every tenth environment has reached its target at its first step, every tenth collides with the workpiece at
    its first step (a wire break), every tenth reaches a target 0.02 um away after some sparks, in mid-interval."""
    n, dev = env.num_envs, env.device
    env.reset(seed=seed)
    idx = torch.arange(n, device=dev)
    wp = torch.linspace(10.4, 25.0, n, dtype=torch.float64, device=dev)
    x = torch.full((n,), 10.0, dtype=torch.float64, device=dev)
    target = torch.full((n,), 5000.0, dtype=torch.float64, device=dev)
    target[idx % 10 == 3] = wp[idx % 10 == 3]
    target[idx % 10 == 7] = wp[idx % 10 == 7] + 0.02
    x[idx % 10 == 5] = wp[idx % 10 == 5] + 101.0
    env.state.workpiece_position = wp
    env.state.wire_position = x
    env.state.target_position = target
    return env.make_action(0.0, 80.0, 9, 3.0, 30.0)


def everything(env) -> Dict[str, torch.Tensor]:
    """Host copies of every block and row that is an environment's state or follows from it: `clone_blocks()` plus the
    env-param values and rows, the material index, and the material and geometry rows selected by it."""
    out = dict(env.state.clone_blocks())
    for name in ("_envp_src", "_envp_rows", "_wmat_index", "_wmat_rows"):
        t = getattr(env, name, None)
        if t is not None:
            out[name] = t.detach().cpu().clone().reshape(-1, t.shape[-1])
    if getattr(env, "_wmat_rows", None) is not None:
        out["_geom_f64"] = env._geom_f64.detach().cpu().clone()
    return out


def _bytes(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.uint8)


def diffs(got: Dict[str, torch.Tensor], want: Dict[str, torch.Tensor], cols_got=None, cols_want=None):
    """Names of the blocks that differ in any BYTE (so NaN payloads and signed zeros count) over the given columns (an
    index list per side; default: every column, padding included)."""
    assert set(got) == set(want), (sorted(got), sorted(want))
    out = []
    for k in got:
        a = got[k] if cols_got is None else got[k][:, cols_got]
        b = want[k] if cols_want is None else want[k][:, cols_want]
        if a.shape != b.shape or not torch.equal(_bytes(a), _bytes(b)):
            rows = [r for r in range(a.shape[0]) if a.shape != b.shape or not torch.equal(_bytes(a[r]), _bytes(b[r]))]
            out.append(f"{k}: rows {rows[:8]}")
    return out


def assert_same(got, want, where="", **kw) -> None:
    bad = diffs(got, want, **kw)
    assert not bad, (where, bad)


def copy_columns_numpy(blocks: Dict[str, torch.Tensor], src, dst) -> Dict[str, torch.Tensor]:
    """Column src[i] of every block into column dst[i], written independently of the package (NumPy fancy indexing on
    the raw bytes): what a fork has to produce."""
    out = {}
    for k, t in blocks.items():
        a = t.contiguous().numpy().copy()
        raw = a.view(np.uint8).reshape(a.shape[0], a.shape[1], -1)
        raw[:, list(dst)] = raw[:, list(src)]
        out[k] = torch.from_numpy(a)
    return out
