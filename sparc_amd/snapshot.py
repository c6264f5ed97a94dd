"""Snapshot, restore and fork of environment subsets, on the device.

Every block of the C-ABI is ``[rows][stride]`` with the environment as the column (the quad-interleaved ``T`` block is
``[quads][stride]`` of 16-byte words), so the state of an environment is one column of every block and moving it is one
operation: `wedm_copy_columns` (include/wedm_hip.h), one launch over a list of *planes* -- one per block -- with no
temporaries.  `WireEDMEnv.snapshot`, `restore` and `fork` are thin callers of the functions below.

What is copied (`env_blocks`): ``f64``, ``i32``, ``i8``, ``T``, ``obs``, ``stats``, ``reward`` and, where present,
``crater_log``, ``pulse``, ``signal``; with ``env_params=`` the user-facing values and the derived device rows; with
``wire_material=`` the material index (the material and geometry rows are then selected from the fixed per-material tables,
as `WireEDMEnv.set_wire_material` does).  What is not: the trace ring (a recording of a window of slots), the
injected-variate table (an input keyed by step since the reset, not by state), the host-side ``steps_since_reset``, and
the geometry rows -- height and diameter belong to the slot, so a copy between slots whose ``(height, diameter)`` differ is
refused.  An environment built with ``dynamic_geometry=`` is the exception: there the two geometry blocks, the height row and
the diameter-index row are state, join the planes and travel with the copy (`sparc_amd.geometry`).

Without a backend ``copy_columns`` (the CPU oracle backend of the tests) the same plane list is served by plain torch:
``index_select`` then ``index_copy_`` block by block, ``T`` through its ``[stride]``-wide 16-byte view.  That path needs
host indices (device tensors are read back) and is what the kernel is checked against.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _abi

STATE_BLOCKS = ("f64", "i32", "i8", "T", "obs", "stats", "reward", "crater_log", "pulse", "signal")
# bit 0: the kernel met an index outside its plane; bit 1: the device-side check found a duplicate destination or a source
# among the destinations
STATUS_RANGE, STATUS_OVERLAP = 1, 2


def env_blocks(env) -> Dict[str, torch.Tensor]:
    """Every block that is part of an environment's state, by name, as the tensors the kernels are bound to."""
    st = env.state
    out = {k: getattr(st, k) for k in STATE_BLOCKS if getattr(st, k) is not None}
    if env._envp_rows is not None:
        out["envp_src"], out["envp_rows"] = env._envp_src, env._envp_rows
    if env._wmat_rows is not None:
        out["wmat_index"] = env._wmat_index.view(1, -1)
    dyn = getattr(env, "_dyn", None)
    if dyn is not None:  # dynamic geometry: the rows, the height and the diameter index are state and travel with the copy
        out["geom_f64"], out["geom_i32"] = env._geom_f64, env._geom_i32
        out["geom_height"], out["geom_diameter_index"] = dyn.height.view(1, -1), dyn.dia.view(1, -1)
    return out


def _wide(t: torch.Tensor) -> torch.Tensor:
    """``[rows][stride]`` face of a block: the T block's 16-byte words as one element each."""
    return t.view(torch.complex128)[..., 0] if t.dim() == 3 else t


def torch_copy_columns(pairs, src_idx: torch.Tensor, dst_idx: torch.Tensor) -> None:
    """The plain-torch form of `wedm_copy_columns`: for every ``(src, dst)`` block pair, columns ``src_idx`` of ``src`` into
    columns ``dst_idx`` of ``dst`` (int64 index tensors on the blocks' device, in range, destinations distinct)."""
    for src, dst in pairs:
        _wide(dst).index_copy_(1, dst_idx, _wide(src).index_select(1, src_idx))


def _plane(src: torch.Tensor, dst: torch.Tensor, src_cols: int, dst_cols: int) -> _abi.CopyPlane:
    assert src.dtype == dst.dtype and src.shape[0] == dst.shape[0] and src.dim() == dst.dim()
    quad = 4 if src.dim() == 3 else 1
    assert src.stride(-1) == 1 and dst.stride(-1) == 1 and (quad == 1 or (src.stride(1) == 4 and dst.stride(1) == 4))
    return _abi.CopyPlane(src.data_ptr(), dst.data_ptr(), src.shape[0], src.element_size() * quad, src.stride(0) // quad,
                          dst.stride(0) // quad, src_cols, dst_cols)


# ------------------------------------------------------------------------------------------------ indices
def _is_device(x) -> bool:
    return torch.is_tensor(x) and x.device.type != "cpu"


def _host_index(x, what: str) -> np.ndarray:
    a = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{what} must be integers, got {a.dtype}")
    return a.reshape(-1).astype(np.int64)


def _device_index(x: torch.Tensor, device) -> torch.Tensor:
    """int32 on the device without reading it; what does not fit int32 becomes -1 (out of every range)."""
    t = x.detach().to(device).reshape(-1)
    if t.is_floating_point() or t.dtype == torch.bool:
        raise ValueError(f"environment indices must be integers, got {t.dtype}")
    if t.dtype == torch.int32:
        return t.contiguous()
    t = t.to(torch.int64)
    return torch.where((t >= 0) & (t < 2**31), t, torch.full_like(t, -1)).to(torch.int32)


def _check_range(a: np.ndarray, n: int, what: str) -> None:
    bad = a[(a < 0) | (a >= n)]
    if bad.size:
        raise ValueError(f"{what} {int(bad[0])} out of range [0, {n})")


def _check_distinct(a: np.ndarray, what: str) -> None:
    u, c = np.unique(a, return_counts=True)
    if (c > 1).any():
        raise ValueError(f"{what} must be distinct: {int(u[c > 1][0])} is named {int(c[c > 1][0])} times "
                         f"(two copies into one environment have no defined result)")


def _upload(a: np.ndarray, device) -> torch.Tensor:
    return torch.from_numpy(a.astype(np.int32)).to(device)


def _device_checks(env, dst: torch.Tensor, src: Optional[torch.Tensor]) -> None:
    """Duplicate destinations (and, for a fork, sources among the destinations) of device-resident index lists, found on
    the device and ORed into the environment's status word: a few stream-ordered ops, nothing read back."""
    n, dev = env.num_envs, env.device
    ok = (dst >= 0) & (dst < n)
    hits = torch.zeros(env.state.stride, dtype=torch.int32, device=dev)
    hits.scatter_add_(0, dst.clamp(0, n - 1).to(torch.int64), ok.to(torch.int32))
    bad = (hits > 1).any()
    if src is not None:
        oks = (src >= 0) & (src < n)
        marks = torch.zeros(env.state.stride, dtype=torch.int32, device=dev)
        marks.scatter_add_(0, src.clamp(0, n - 1).to(torch.int64), oks.to(torch.int32))
        bad = bad | ((hits > 0) & (marks > 0)).any()
    env._copy_status.bitwise_or_(bad.to(torch.int32) * STATUS_OVERLAP)


def _launch(env, pairs, src_cols: int, dst_cols: int, src, dst, count: int) -> None:
    """`src` / `dst`: host int64 arrays (validated) or int32 device tensors."""
    if count == 0:
        return
    backend = env._backend
    if hasattr(backend, "copy_columns"):
        dev = env.device
        s = src if torch.is_tensor(src) else _upload(src, dev)
        d = dst if torch.is_tensor(dst) else _upload(dst, dev)
        planes = [_plane(a, b, src_cols, dst_cols) for a, b in pairs]
        for k in range(0, len(planes), _abi.COPY_MAX_PLANES):
            backend.copy_columns(planes[k: k + _abi.COPY_MAX_PLANES], s.data_ptr(), d.data_ptr(), count,
                                 env._copy_status.data_ptr())
        env._copy_keep = (s, d, pairs)  # the launch is asynchronous: its inputs live until the next one replaces them
    else:
        dev = pairs[0][0].device
        torch_copy_columns(pairs, torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev))


def _needs_host(env, *others) -> bool:
    """Device-resident indices have to be read back: on the torch path, and where slots differ in geometry (the
    ``(height, diameter)`` check runs on the host: one synchronisation per call in that configuration)."""
    return not hasattr(env._backend, "copy_columns") or env._geom_hd is not None or any(o is not None for o in others)


def _same_geometry(a: np.ndarray, b: np.ndarray, ia: np.ndarray, ib: np.ndarray, what: str) -> None:
    differ = np.flatnonzero((a[:, ia] != b[:, ib]).any(axis=0))
    if differ.size:
        k = int(differ[0])
        raise ValueError(f"{what}: environment {int(ib[k])} has (height, diameter) = {tuple(b[:, ib[k]])}, the state to be "
                         f"copied into it belongs to {tuple(a[:, ia[k]])}: geometry belongs to the slot and is not copied, so "
                         f"the copy would continue the state on another workpiece / wire")


# ------------------------------------------------------------------------------------------------ the snapshot
class EnvSnapshot:
    """Compact device copies of some environments' columns of every state block (`env_blocks`), at a stride of its own
    (``count`` rounded up to 64), plus what a restore must check.  ``env_ids`` are the environments the columns came from
    (where `restore` puts them back by default).  `to` moves it (``snap.to("cpu")`` to store it), `state_dict` /
    `from_state_dict` give a form of tensors, ints and strings that ``torch.load(..., weights_only=True)`` accepts."""

    def __init__(self, meta: Dict[str, Any], blocks: Dict[str, torch.Tensor], env_ids: torch.Tensor,
                 geometry: Optional[torch.Tensor] = None):
        self.meta, self.blocks, self.env_ids, self.geometry = dict(meta), dict(blocks), env_ids, geometry

    @property
    def count(self) -> int:
        return int(self.meta["count"])

    @property
    def stride(self) -> int:
        return int(self.blocks["f64"].shape[1])

    @property
    def device(self) -> torch.device:
        return self.blocks["f64"].device

    def to(self, device) -> "EnvSnapshot":
        device = torch.device(device)
        if device == self.device:
            return self
        return EnvSnapshot(self.meta, {k: v.to(device) for k, v in self.blocks.items()}, self.env_ids.to(device),
                           None if self.geometry is None else self.geometry.to(device))

    def state_dict(self) -> Dict[str, Any]:
        return {"meta": dict(self.meta), "blocks": {k: v.detach().cpu().clone() for k, v in self.blocks.items()},
                "env_ids": self.env_ids.detach().cpu().clone(),
                "geometry": None if self.geometry is None else self.geometry.detach().cpu().clone()}

    @classmethod
    def from_state_dict(cls, sd: Dict[str, Any], device=None) -> "EnvSnapshot":
        snap = cls(sd["meta"], sd["blocks"], sd["env_ids"], sd.get("geometry"))
        return snap if device is None else snap.to(device)


def _meta(env) -> Dict[str, Any]:
    """What must agree between the environment a snapshot was taken from and the one it is restored into."""
    log = env.state.crater_log
    return {"abi_version": _abi.ABI_VERSION, "n_segments": env.n_segments, "obs_dim": env.obs_dim,
            "crater_log_capacity": 0 if log is None else int(log.shape[0]), "blocks": sorted(env_blocks(env)),
            "physics": env._physics_fingerprint(),
            "env_param_names": list(env.env_param_names) if env._envp_rows is not None else None,
            "wire_materials": [m.name for m in env.wire_materials] if env._wmat_rows is not None else None,
            "wire_material_table": env._wire_material_fingerprint() if env._wmat_rows is not None else None}


def _check_meta(env, snap: EnvSnapshot) -> None:
    mine, theirs = _meta(env), snap.meta
    if theirs.get("abi_version") != mine["abi_version"]:
        raise ValueError(f"snapshot was taken with state layout ABI {theirs.get('abi_version')}, this build is ABI "
                         f"{mine['abi_version']}: it cannot be restored here")
    shape = ("n_segments", "obs_dim", "crater_log_capacity")
    if any(theirs.get(k) != mine[k] for k in shape):
        raise ValueError("snapshot was taken from an environment of a different shape: "
                         + ", ".join(f"{k} {theirs.get(k)} against {mine[k]}" for k in shape if theirs.get(k) != mine[k]))
    if list(theirs.get("blocks", ())) != mine["blocks"] or theirs.get("env_param_names") != mine["env_param_names"]:
        raise ValueError(f"snapshot holds the blocks {theirs.get('blocks')} (per-environment physics parameters "
                         f"{theirs.get('env_param_names')}), this environment has {mine['blocks']} "
                         f"({mine['env_param_names']}): the optional blocks differ")
    if theirs.get("wire_materials") != mine["wire_materials"] or theirs.get("wire_material_table") != mine["wire_material_table"]:
        raise ValueError(f"snapshot was taken with per-environment wire materials {theirs.get('wire_materials')}, this "
                         f"environment has {mine['wire_materials']}"
                         + (" (same names, different constants or geometry)"
                            if theirs.get("wire_materials") == mine["wire_materials"] else "") + ": the material table differs")
    if theirs.get("physics") != mine["physics"]:
        raise ValueError("snapshot was taken with different physics (configuration, module parameters, control mode or "
                         "per-environment geometry): restoring it would silently change the trajectory")


def snapshot(env, env_ids=None) -> EnvSnapshot:
    n = env.num_envs
    if env_ids is None:
        env_ids = np.arange(n)
    if _is_device(env_ids) and not _needs_host(env):
        ids = _device_index(env_ids, env.device)  # range: the kernel's check; a source may be named more than once
        count, keep = int(ids.numel()), ids
    else:
        ids = _host_index(env_ids, "snapshot: environment index")
        _check_range(ids, n, "snapshot: environment index")
        count, keep = int(ids.size), _upload(ids, env.device)
    stride = (count + 63) // 64 * 64
    src = env_blocks(env)
    blocks = {k: torch.zeros((t.shape[0], stride) + tuple(t.shape[2:]), dtype=t.dtype, device=t.device) for k, t in src.items()}
    meta = dict(_meta(env), count=count)
    geometry = None if env._geom_hd is None else torch.from_numpy(env._geom_hd[:, ids].copy())
    dst = np.arange(count) if not torch.is_tensor(ids) else torch.arange(count, dtype=torch.int32, device=env.device)
    _launch(env, [(src[k], blocks[k]) for k in src], n, count, ids, dst, count)
    return EnvSnapshot(meta, blocks, keep, geometry)


def restore(env, snap: EnvSnapshot, env_ids=None, columns=None) -> None:
    if not isinstance(snap, EnvSnapshot):
        raise TypeError("restore needs an EnvSnapshot (env.snapshot(), EnvSnapshot.from_state_dict())")
    _check_meta(env, snap)
    snap = snap.to(env.device)
    n, count = env.num_envs, snap.count
    on_device = (_is_device(env_ids) or _is_device(columns) or (env_ids is None and _is_device(snap.env_ids))) \
        and not _needs_host(env, snap.geometry)
    if on_device:
        dev = env.device
        ids = None if env_ids is None else _device_index(torch.as_tensor(env_ids), dev)
        if columns is None:
            cols = torch.arange(count if ids is None else int(ids.numel()), dtype=torch.int32, device=dev)
        else:
            cols = _device_index(torch.as_tensor(columns), dev)
        if ids is None:   # back where the columns came from
            ok = (cols >= 0) & (cols < count)
            back = snap.env_ids.to(torch.int32).index_select(0, cols.clamp(0, max(count - 1, 0)).to(torch.int64))
            ids = torch.where(ok, back, torch.full_like(back, -1))
        if ids.numel() != cols.numel():
            raise ValueError(f"restore: {ids.numel()} environments for {cols.numel()} snapshot columns")
        _device_checks(env, ids, None)
        m = int(ids.numel())
    else:
        cols = None if columns is None else _host_index(columns, "restore: snapshot column")
        if env_ids is None:
            if cols is None:
                cols = np.arange(count)
            _check_range(cols, count, "restore: snapshot column")
            ids = _host_index(snap.env_ids, "restore: environment index")[cols]
        else:
            ids = _host_index(env_ids, "restore: environment index")
            if cols is None:
                cols = np.arange(ids.size)
        if ids.size != cols.size:
            raise ValueError(f"restore: {ids.size} environments for {cols.size} snapshot columns")
        _check_range(cols, count, "restore: snapshot column")
        _check_range(ids, n, "restore: environment index")
        _check_distinct(ids, "restore: destination environments")
        if env._geom_hd is not None:
            _same_geometry(snap.geometry.cpu().numpy(), env._geom_hd, cols, ids, "restore")
        m = int(ids.size)
    dst = env_blocks(env)
    _launch(env, [(snap.blocks[k], dst[k]) for k in dst], count, n, cols, ids, m)
    if env._wmat_rows is not None:
        env._select_wire_material_rows()


def fork(env, src_ids, dst_ids) -> None:
    n = env.num_envs
    on_device = (_is_device(src_ids) or _is_device(dst_ids)) and not _needs_host(env)
    if on_device:
        dev = env.device
        d = _device_index(torch.as_tensor(dst_ids), dev)
        s = _device_index(torch.as_tensor(src_ids), dev)
        if s.numel() == 1 and d.numel() != 1:
            s = s.expand(d.numel()).contiguous()
        if s.numel() != d.numel():
            raise ValueError(f"fork: {s.numel()} sources for {d.numel()} destinations (one source per destination, or one for all)")
        _device_checks(env, d, s)
        m = int(d.numel())
    else:
        d = _host_index(dst_ids, "fork: destination environment")
        s = _host_index(src_ids, "fork: source environment")
        if s.size == 1 and d.size != 1:
            s = np.broadcast_to(s, d.shape).copy()
        if s.size != d.size:
            raise ValueError(f"fork: {s.size} sources for {d.size} destinations (one source per destination, or one for all)")
        _check_range(s, n, "fork: source environment")
        _check_range(d, n, "fork: destination environment")
        _check_distinct(d, "fork: destination environments")
        both = np.intersect1d(s, d)
        if both.size:
            raise ValueError(f"fork: environment {int(both[0])} is both a source and a destination (the copy runs in place, "
                             f"in one launch: a source must not be overwritten by it)")
        if env._geom_hd is not None:
            _same_geometry(env._geom_hd, env._geom_hd, s, d, "fork")
        m = int(d.size)
    blocks = env_blocks(env)
    _launch(env, [(t, t) for t in blocks.values()], n, n, s, d, m)
    if env._wmat_rows is not None:
        env._select_wire_material_rows()


def fork_rows(rows: torch.Tensor, src_ids, dst_ids) -> None:
    """The same copy for a per-environment 1-D tensor that lives outside the environment (an adapter's own flags), in
    torch; pairs with an index out of range are skipped, as the kernel skips them."""
    n, dev = rows.numel(), rows.device
    d = (_device_index(torch.as_tensor(dst_ids), dev) if _is_device(dst_ids) else
         torch.from_numpy(_host_index(dst_ids, "fork: destination environment")).to(dev)).to(torch.int64)
    s = (_device_index(torch.as_tensor(src_ids), dev) if _is_device(src_ids) else
         torch.from_numpy(_host_index(src_ids, "fork: source environment")).to(dev)).to(torch.int64)
    if s.numel() == 1 and d.numel() != 1:
        s = s.expand(d.numel())
    ok = (s >= 0) & (s < n) & (d >= 0) & (d < n)
    ext = torch.cat([rows, rows[:1]])  # (a skipped pair writes the spare element)
    ext.scatter_(0, torch.where(ok, d, torch.full_like(d, n)), rows.index_select(0, s.clamp(0, n - 1)))
    rows.copy_(ext[:n])
