"""The wire's temperature profile per environment, reduced on the device.

The wire is the largest piece of an environment's state and the thing a policy must keep from breaking; the observation
carries one scalar of it.  `wire_profile` gives, for any geometry -- uniform, per-environment height / diameter, per-environment
material -- the mean over the workpiece zone, the wire's mean, maximum and hottest cell, and the wire pooled into ``bins``
bins (maximum and mean of each), by one launch of `wedm_wire_profile` (include/wedm_hip.h, which holds the definition) with
no temporaries.  `WireEDMEnv.wire_profile`, `WireEDMEnv.zone_mean_temperature` (per-environment geometry) and
`WireEDMVectorEnv(wire_profile_bins=)` are thin callers.

The profile is derived from ``T``: it is not state, and `snapshot` / `restore` / `fork` and `state_dict` do not carry it.

Without a backend ``wire_profile`` (the CPU oracle backends of the tests) `torch_wire_profile` computes the same definition
on the host, environment by environment; that path is what the kernel is checked against.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _abi
from .snapshot import _check_range, _device_index, _host_index, _is_device, _upload

# bits of the status word: the kernel met an environment index outside [0, num_envs) / a geometry row whose n_seg is outside
# [1, n_seg_max]; the column was left unwritten
STATUS_RANGE, STATUS_GEOMETRY = 1, 2
FIXED_NAMES = ("zone_mean", "wire_mean", "wire_max", "hot_cell")


def profile_names(bins: int):
    """Names of the rows of a profile with ``bins`` bins, in order (the observation columns `WireEDMVectorEnv` appends)."""
    return ("wire_zone_mean", "wire_mean", "wire_max", "wire_hot_cell") + tuple(f"wire_bin_max_{b}" for b in range(bins)) + \
        tuple(f"wire_bin_mean_{b}" for b in range(bins))


def _check_bins(bins) -> int:
    if isinstance(bins, bool) or int(bins) != bins or not 0 <= int(bins) <= _abi.PROFILE_MAX_BINS:
        raise ValueError(f"bins must be an integer in [0, {_abi.PROFILE_MAX_BINS}], got {bins!r}")
    return int(bins)


def _mean32(cells: np.ndarray) -> np.float32:
    """The float64 sum of float32 cells, divided in float64, rounded once to float32."""
    return np.float32(np.sum(cells, dtype=np.float64) / np.float64(cells.size))


def torch_wire_profile(T, num_envs: int, n_seg, az_start, az_end, bins: int = 8, env_ids=None) -> torch.Tensor:
    """The definition of `wedm_wire_profile` on host data: ``T`` is the ``[quads, stride, 4]`` wire block (a tensor on any
    device or an array), ``n_seg`` / ``az_start`` / ``az_end`` are integers (uniform geometry) or one value per
    environment, ``env_ids`` host indices in range (default: all).  Returns float32 ``[4 + 2 * bins, count]`` on the CPU."""
    bins = _check_bins(bins)
    block = T.detach().cpu().numpy() if torch.is_tensor(T) else np.asarray(T)
    assert block.dtype == np.float32 and block.ndim == 3 and block.shape[2] == 4
    ids = np.arange(num_envs) if env_ids is None else _host_index(env_ids, "wire_profile: environment index")
    _check_range(ids, num_envs, "wire_profile: environment index")
    n_all, zs_all, ze_all = (np.broadcast_to(np.asarray(x, dtype=np.int64), (num_envs,)) for x in (n_seg, az_start, az_end))
    out = np.zeros((_abi.profile_rows(bins), ids.size), dtype=np.float32)
    for col, e in enumerate(ids):
        n, zs, ze = int(n_all[e]), int(zs_all[e]), int(ze_all[e])
        if not 1 <= n <= block.shape[0] * 4:
            raise ValueError(f"wire_profile: environment {int(e)} has n_seg {n}, outside [1, {block.shape[0] * 4}]")
        t = block[:, e, :].reshape(-1)[:n]
        zone = t[zs:ze] if 0 <= zs < ze <= n else t
        out[_abi.PR.ZONE_MEAN, col] = _mean32(zone)
        out[_abi.PR.WIRE_MEAN, col] = _mean32(t)
        out[_abi.PR.WIRE_MAX, col] = t.max()
        out[_abi.PR.HOT_CELL, col] = np.float32(int(np.argmax(t)))  # the first of equals
        for b in range(bins):
            lo = b * n // bins
            hi = max(lo + 1, (b + 1) * n // bins)
            out[_abi.PR_FIXED + b, col] = t[lo:hi].max()
            out[_abi.PR_FIXED + bins + b, col] = _mean32(t[lo:hi])
    return torch.from_numpy(out)


def _geometry(env):
    """(n_seg, az_start, az_end): integers with uniform geometry, host int64 arrays per environment otherwise."""
    if env.geometry is not None:
        g = env.geometry
        return int(g.n_seg), int(g.az_start), int(g.az_end)
    gi = env._geom_i32.detach().cpu().numpy()[:, : env.num_envs].astype(np.int64)
    return gi[_abi.GI32.N_SEG], gi[_abi.GI32.AZ_START], gi[_abi.GI32.AZ_END]


def _as_dict(rows: torch.Tensor, bins: int) -> Dict[str, torch.Tensor]:
    out = {name: rows[k] for k, name in enumerate(FIXED_NAMES)}
    out["bin_max"] = rows[_abi.PR_FIXED: _abi.PR_FIXED + bins]
    out["bin_mean"] = rows[_abi.PR_FIXED + bins: _abi.PR_FIXED + 2 * bins]
    out["rows"] = rows
    return out


def wire_profile(env, bins: int = 8, env_ids=None) -> Dict[str, torch.Tensor]:
    """The wire profile of the environments ``env_ids`` (default: all, in order) as float32 tensors on the environment's
    device: ``zone_mean``, ``wire_mean``, ``wire_max``, ``hot_cell`` of shape ``[count]``, ``bin_max`` and ``bin_mean`` of
    shape ``[bins, count]``, and ``rows``, the ``[4 + 2 * bins, count]`` block all of them are views of (rows in the order
    of `profile_names`).  Column ``i`` describes environment ``env_ids[i]``; an environment may be named more than once.

    THE TENSORS ARE VALID UNTIL THE NEXT CALL with the same ``(bins, count)``: the output block is cached per
    ``(bins, count)`` on the environment and reused, so that a call allocates nothing.  Clone what must outlive it.

    ``env_ids``: a sequence, a NumPy array, a CPU tensor or a device tensor.  Host indices are checked here and raise
    ``ValueError`` before anything is launched.  A device tensor is never read back: the kernel skips an index outside
    ``[0, num_envs)`` (that column keeps what it held) and sets a flag that `WireEDMEnv.check_errors` raises for."""
    bins = _check_bins(bins)
    n = env.num_envs
    native = hasattr(env._backend, "wire_profile")
    ids = None
    if env_ids is None:
        count = n
    elif _is_device(env_ids) and native:
        ids = _device_index(env_ids, env.device)
        count = int(ids.numel())
    else:
        ids = _host_index(env_ids, "wire_profile: environment index")
        _check_range(ids, n, "wire_profile: environment index")
        count = int(ids.size)
    if not native:
        n_seg, zs, ze = _geometry(env)
        return _as_dict(torch_wire_profile(env.state.T, n, n_seg, zs, ze, bins, ids).to(env.device), bins)
    rows = _abi.profile_rows(bins)
    cache = env._profile_out
    block = cache.get((bins, count))
    if block is None:
        if len(cache) >= 8:  # callers with ever-changing counts do not pile up blocks
            cache.clear()
        block = cache[(bins, count)] = torch.zeros((rows, max((count + 63) // 64 * 64, 64)), dtype=torch.float32,
                                                   device=env.device)
    if count:
        if ids is not None and not torch.is_tensor(ids):
            ids = _upload(ids, env.device)
        st = env.state
        g = env.geometry
        desc = _abi.ProfileDesc(
            T=st.T.data_ptr(), stride=st.stride, num_envs=n, n_seg_max=env.n_segments,
            n_seg=g.n_seg if g is not None else 0, az_start=g.az_start if g is not None else 0,
            az_end=g.az_end if g is not None else 0, geom_i32=None if g is not None else env._geom_i32.data_ptr(),
            bins=bins, out=block.data_ptr(), out_stride=block.shape[1], out_cols=count)
        env._backend.wire_profile(desc, None if ids is None else ids.data_ptr(), count, env._profile_status.data_ptr())
        env._profile_keep = ids  # the launch is asynchronous: its index list lives until the next one replaces it
    return _as_dict(block[:, :count], bins)


def status_text(status: int) -> Optional[str]:
    """What `check_errors` says about a non-zero status word of `wire_profile`."""
    what = [text for bit, text in ((STATUS_RANGE, "an environment index out of range"),
                                   (STATUS_GEOMETRY, "a geometry row whose n_seg lies outside [1, n_segments]"))
            if status & bit]
    if not what:
        return None
    return ("wire_profile with indices in a device tensor: " + "; ".join(what) + " (those columns of the profile were not "
            "written).  The indices were not read back when the profile was launched; this check reports and clears the flag")
