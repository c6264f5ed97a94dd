"""Loader of ``libwedm_hip.so`` — the only compute path of this package.

There is deliberately no fallback: if the HIP library is missing or no gfx950
device is visible, construction fails with an explicit error instead of silently
running something else."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import torch

from . import _abi

# WEDM_HIP_LIB lets the profiling scripts load an instrumented build of the SAME library;
# it never selects a different implementation.
import os

LIB_PATH = Path(os.environ.get("WEDM_HIP_LIB") or (Path(__file__).resolve().parent / "libwedm_hip.so"))


class WedmError(RuntimeError):
    def __init__(self, code: int, text: str):
        super().__init__(f"{_abi.STATUS_NAMES.get(code, code)}: {text}")
        self.code = code


_lib = None

_ctx, _p, _i32, _i64, _to = C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.POINTER  # (_p: a device address, a stream)
_form_out = (_to(C.c_int32), _to(C.c_int32), _to(C.c_uint32))
# every entry point of include/wedm_hip.h: its result type, then its argument types
_SIGNATURES = {
    "wedm_abi_version": (_i32,),
    "wedm_sizeof_params": (_i64,),
    "wedm_create": (_i32, _to(_abi.Params), _i32, _i32, _to(_ctx)),
    "wedm_destroy": (_i32, _ctx),
    "wedm_bind_state": (_i32, _ctx, _to(_abi.StatePtrs)),
    "wedm_bind_geometry": (_i32, _ctx, _to(_abi.GeomPtrs)),
    "wedm_reset": (_i32, _ctx, _p, C.c_uint64, _i32, _p),
    "wedm_step": (_i32, _ctx, _i32, _to(_abi.ActionPtrs), _p),
    "wedm_bind_trace": (_i32, _ctx, _to(_abi.TraceDesc)),
    "wedm_bind_rng_replay": (_i32, _ctx, _p, _i64),
    "wedm_bind_pulse_stats": (_i32, _ctx, _p),
    "wedm_bind_signal_stats": (_i32, _ctx, _p),
    "wedm_bind_env_params": (_i32, _ctx, _p),
    "wedm_bind_wire_material": (_i32, _ctx, _p),
    "wedm_trace_samples": (_i64, _ctx),
    "wedm_set_kernel": (_i32, _ctx, _i32),
    "wedm_set_lanes": (_i32, _ctx, _i32),
    "wedm_last_error": (C.c_char_p, _ctx),
    "wedm_last_kernel": (C.c_char_p, _ctx),
    "wedm_last_occupancy": (_i32, _ctx),
    "wedm_debug_math": (_i32, _i32, _p, _p, _p, _i32, _p),
    "wedm_debug_poison_lds": (_i32, C.c_float, _p),
    "wedm_debug_registry": (_i32, _i32, *_form_out),
    "wedm_debug_last_form": (_i32, _ctx, *_form_out),
    "wedm_debug_form_name": (C.c_char_p, _i32),
    "wedm_copy_columns": (_i32, _to(_abi.CopyPlane), _i32, _p, _p, _i32, _p, _p),
    "wedm_wire_profile": (_i32, _to(_abi.ProfileDesc), _p, _i32, _p, _p),
    "wedm_derive_geometry": (_i32, _to(_abi.GeomDeriveDesc), _p, _p, _p, _p, _p, _p),
    "wedm_draw_episode": (_i32, _to(_abi.DrawDesc), _p, _p, _p),
    "wedm_normalize": (_i32, _to(_abi.NormDesc), _p),
    "wedm_gae": (_i32, _to(_abi.GaeDesc), _p),
    "wedm_policy_head": (_i32, _to(_abi.HeadDesc), _p),
    "wedm_ppo_loss": (_i32, _to(_abi.PpoDesc), _p),
    "wedm_policy_net": (_i32, _to(_abi.NetDesc), _p),
    "wedm_adam": (_i32, _to(_abi.OptDesc), _p),
    "wedm_minibatch_index": (_i32, _to(_abi.MbDesc), _p),
    "wedm_episode_log": (_i32, _to(_abi.ElogDesc), _p),
    "wedm_reward": (_i32, _to(_abi.RewardDesc), _p),
    "wedm_sensor": (_i32, _to(_abi.SensorDesc), _p),
    "wedm_build_id": (C.c_char_p,),
}
EXPORTS = tuple(_SIGNATURES)


def _declare(L: C.CDLL, name: str) -> None:
    fn = getattr(L, name)
    fn.restype, *fn.argtypes = _SIGNATURES[name]


def load() -> C.CDLL:
    """dlopen the library and declare every entry point of include/wedm_hip.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  sparc_amd has no CPU or PyTorch fallback."
        )
    L = C.CDLL(str(LIB_PATH))
    for name in ("wedm_abi_version", "wedm_sizeof_params"):
        _declare(L, name)
    if L.wedm_abi_version() != _abi.ABI_VERSION:
        raise ImportError(f"libwedm_hip.so has ABI {L.wedm_abi_version()}, python expects {_abi.ABI_VERSION}")
    if L.wedm_sizeof_params() != C.sizeof(_abi.Params):
        raise ImportError("struct wedm_params layout mismatch between libwedm_hip.so and sparc_amd._abi")
    for name in EXPORTS:
        _declare(L, name)
    _lib = L
    return L


def registry() -> list:
    """Every compiled instantiation of a step kernel as (kernel, lanes, forms), in the library's order
    (`wedm_debug_registry`); needs no device."""
    L = load()
    k, lanes, forms = C.c_int32(), C.c_int32(), C.c_uint32()
    rc = L.wedm_debug_registry(-1, C.byref(k), None, None)
    if rc != _abi.OK:
        raise WedmError(rc, "wedm_debug_registry(-1)")
    out = []
    for i in range(k.value):
        rc = L.wedm_debug_registry(i, C.byref(k), C.byref(lanes), C.byref(forms))
        if rc != _abi.OK:
            raise WedmError(rc, f"wedm_debug_registry({i})")
        out.append((k.value, lanes.value, forms.value))
    return out


def build_id() -> str:
    """`wedm_build_id()` of the loaded library: the fingerprint measurement records are bound to (include/wedm_hip.h)."""
    return load().wedm_build_id().decode()


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def call_stateless(fn, device: torch.device, *args) -> None:
    """A call of ``fn``, an entry point that takes no handle and a stream last, on ``device`` and torch's current stream
    there: the device is made current for the call when it is not (an index of None is the current device), the stream goes
    as its raw handle (no Stream object is built where the accessor exists), and a refusal raises `WedmError` with the
    library's text."""
    current, index = torch.cuda.current_device(), device.index
    if index is None:
        index = current
    with _NO_GUARD if index == current else torch.cuda.device(index):
        stream = _RAW_STREAM(index) if _RAW_STREAM is not None else torch.cuda.current_stream(index).cuda_stream
        rc = fn(*args, C.c_void_p(stream))
    if rc != _abi.OK:
        raise WedmError(rc, (load().wedm_last_error(None) or b"").decode())


class HipBackend:
    """Thin owner of one ``wedm_ctx``.  All memory stays with the caller (torch)."""

    name = "hip"

    def __init__(self, params: _abi.Params, num_envs: int, n_seg_max: int, device):
        import torch

        if device.type != "cuda":
            raise RuntimeError(
                f"sparc_amd runs on an AMD GPU only (device={device}); there is no CPU path. "
                "Use device='cuda' on an MI355X."
            )
        self._L = load()
        self._torch = torch
        self.device = device
        self._raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        self._ctx = C.c_void_p()
        with torch.cuda.device(device):
            rc = self._L.wedm_create(C.byref(params), num_envs, n_seg_max, C.byref(self._ctx))
        if rc != _abi.OK:
            raise WedmError(rc, (self._L.wedm_last_error(None) or b"").decode())

    def _check(self, rc: int) -> None:
        if rc != _abi.OK:
            raise WedmError(rc, (self._L.wedm_last_error(self._ctx) or b"").decode())

    def _stream(self):
        # raw handle of torch's current stream on this device (the public accessor builds a
        # Stream object per call: several microseconds on the per-microsecond stepping path)
        raw = self._raw_stream
        if raw is not None:
            return C.c_void_p(raw(self.device.index))
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def bind_state(self, ptrs: _abi.StatePtrs) -> None:
        self._check(self._L.wedm_bind_state(self._ctx, C.byref(ptrs)))

    def bind_geometry(self, ptrs: _abi.GeomPtrs) -> None:
        self._check(self._L.wedm_bind_geometry(self._ctx, C.byref(ptrs)))

    def _on_device(self):
        """The library launches on whatever device is current and refuses a handle of another one
        (wedm_step / wedm_reset return WEDM_ERR_BAD_ARG): make this environment's device current
        for the call when it is not (an environment on cuda:1 in a process whose current device is
        cuda:0).  The common case — already current — costs one integer compare."""
        torch = self._torch
        if torch.cuda.current_device() == self.device.index:
            return _NO_GUARD
        return torch.cuda.device(self.device)

    def reset(self, mask_ptr, seed: int, reseed: bool, fresh: bool = False) -> None:
        """`fresh`: WEDM_RESET_FRESH -- module-private state too, whatever `reset_semantics` (a handle's first reset)."""
        with self._on_device():
            flags = (1 if reseed else 0) | (2 if fresh else 0)
            self._check(self._L.wedm_reset(self._ctx, mask_ptr, seed & (2**64 - 1), flags, self._stream()))

    def step(self, n_substeps: int, action: _abi.ActionPtrs) -> None:
        with self._on_device():
            self._check(self._L.wedm_step(self._ctx, n_substeps, C.byref(action), self._stream()))

    def bind_trace(self, desc) -> None:
        """`desc` is an `_abi.TraceDesc` or None (unbind)."""
        self._check(self._L.wedm_bind_trace(self._ctx, C.byref(desc) if desc is not None else None))

    def bind_rng_replay(self, table_ptr, n_steps: int) -> None:
        self._check(self._L.wedm_bind_rng_replay(self._ctx, table_ptr, int(n_steps)))

    def bind_pulse_stats(self, rows_ptr) -> None:
        """`rows_ptr`: device address of an int32 [PULSE_COUNT][stride] block, or None (unbind)."""
        self._check(self._L.wedm_bind_pulse_stats(self._ctx, rows_ptr))

    def bind_signal_stats(self, rows_ptr) -> None:
        """`rows_ptr`: device address of a float64 [SIG_COUNT][stride] block, or None (unbind).  After `bind_state`."""
        self._check(self._L.wedm_bind_signal_stats(self._ctx, rows_ptr))

    def bind_env_params(self, rows_ptr) -> None:
        """`rows_ptr`: device address of a float64 [ENVP_COUNT][stride] block, or None (unbind)."""
        self._check(self._L.wedm_bind_env_params(self._ctx, rows_ptr))

    def bind_wire_material(self, rows_ptr) -> None:
        """`rows_ptr`: device address of a float64 [WMAT_COUNT][stride] block, or None (unbind).  Needs bound
        per-environment geometry."""
        self._check(self._L.wedm_bind_wire_material(self._ctx, rows_ptr))

    def copy_columns(self, planes, src_idx_ptr, dst_idx_ptr, count: int, status_ptr=None) -> None:
        """`wedm_copy_columns` on this backend's device and torch's current stream: `planes` is a sequence of
        `_abi.CopyPlane` (at most `_abi.COPY_MAX_PLANES`), the index lists are device addresses of int32[count], `status_ptr`
        the device address of an int32 word or None."""
        arr = (_abi.CopyPlane * len(planes))(*planes)
        call_stateless(self._L.wedm_copy_columns, self.device, arr, len(planes), src_idx_ptr, dst_idx_ptr, int(count), status_ptr)

    def wire_profile(self, desc: "_abi.ProfileDesc", env_idx_ptr, count: int, status_ptr=None) -> None:
        """`wedm_wire_profile` on this backend's device and torch's current stream: ``env_idx_ptr`` is the device address of
        int32[count] or None (environments ``0 .. count - 1``), ``status_ptr`` the device address of an int32 word or None."""
        call_stateless(self._L.wedm_wire_profile, self.device, C.byref(desc), env_idx_ptr, int(count), status_ptr)

    def derive_geometry(self, desc: "_abi.GeomDeriveDesc", height_ptr, diameter_idx_ptr, material_idx_ptr=None, mask_ptr=None,
                        status_ptr=None) -> None:
        """`wedm_derive_geometry` on this backend's device and torch's current stream: device addresses of float64[num_envs]
        heights, int32[num_envs] diameter indices, int32[num_envs] material indices or None (material 0), a uint8[num_envs]
        mask or None (every environment) and an int32 status word or None."""
        call_stateless(self._L.wedm_derive_geometry, self.device, C.byref(desc), height_ptr, diameter_idx_ptr, material_idx_ptr,
                       mask_ptr, status_ptr)

    def draw_episode(self, desc: "_abi.DrawDesc", mask_ptr, draw_count_ptr) -> None:
        """`wedm_draw_episode` on this backend's device and torch's current stream: device addresses of a uint8[num_envs] mask
        or None (every environment) and of the sampler's int32[stride] draw counts."""
        call_stateless(self._L.wedm_draw_episode, self.device, C.byref(desc), mask_ptr, draw_count_ptr)

    def normalize(self, desc: "_abi.NormDesc") -> None:
        """`wedm_normalize` on this backend's device and torch's current stream (at most three launches, no synchronisation)."""
        call_stateless(self._L.wedm_normalize, self.device, C.byref(desc))

    def gae(self, desc: "_abi.GaeDesc") -> None:
        """`wedm_gae` on this backend's device and torch's current stream (at most three launches, no synchronisation)."""
        call_stateless(self._L.wedm_gae, self.device, C.byref(desc))

    def policy_head(self, desc: "_abi.HeadDesc") -> None:
        """`wedm_policy_head` on this backend's device and torch's current stream (one launch, no synchronisation)."""
        call_stateless(self._L.wedm_policy_head, self.device, C.byref(desc))

    def ppo_loss(self, desc: "_abi.PpoDesc") -> None:
        """`wedm_ppo_loss` on this backend's device and torch's current stream (at most four launches, no synchronisation)."""
        call_stateless(self._L.wedm_ppo_loss, self.device, C.byref(desc))

    def policy_net(self, desc: "_abi.NetDesc") -> None:
        """`wedm_policy_net` on this backend's device and torch's current stream (at most three launches, no synchronisation)."""
        call_stateless(self._L.wedm_policy_net, self.device, C.byref(desc))

    def adam(self, desc: "_abi.OptDesc") -> None:
        """`wedm_adam` on this backend's device and torch's current stream (one launch or at most three, no synchronisation)."""
        call_stateless(self._L.wedm_adam, self.device, C.byref(desc))

    def minibatch_index(self, desc: "_abi.MbDesc") -> None:
        """`wedm_minibatch_index` on this backend's device and torch's current stream (at most three launches, no synchronisation)."""
        call_stateless(self._L.wedm_minibatch_index, self.device, C.byref(desc))

    def episode_log(self, desc: "_abi.ElogDesc") -> None:
        """`wedm_episode_log` on this backend's device and torch's current stream (at most three launches, no synchronisation)."""
        call_stateless(self._L.wedm_episode_log, self.device, C.byref(desc))

    def reward(self, desc: "_abi.RewardDesc") -> None:
        """`wedm_reward` on this backend's device and torch's current stream (one launch, no synchronisation)."""
        call_stateless(self._L.wedm_reward, self.device, C.byref(desc))

    def sensor(self, desc: "_abi.SensorDesc") -> None:
        """`wedm_sensor` on this backend's device and torch's current stream (one launch, no synchronisation)."""
        call_stateless(self._L.wedm_sensor, self.device, C.byref(desc))

    def trace_samples(self) -> int:
        return int(self._L.wedm_trace_samples(self._ctx))

    def set_kernel(self, variant: int) -> None:
        self._check(self._L.wedm_set_kernel(self._ctx, variant))

    def set_lanes(self, lanes: int) -> None:
        self._check(self._L.wedm_set_lanes(self._ctx, lanes))

    def last_kernel(self) -> str:
        return (self._L.wedm_last_kernel(self._ctx) or b"").decode()

    def last_form(self) -> tuple:
        """(kernel, lanes, forms) of the instantiation the last launch ran (`_abi.KERNEL`, lanes per environment,
        `_abi.FORM` bits): `wedm_debug_last_form`."""
        k, lanes, forms = C.c_int32(), C.c_int32(), C.c_uint32()
        self._check(self._L.wedm_debug_last_form(self._ctx, C.byref(k), C.byref(lanes), C.byref(forms)))
        return k.value, lanes.value, forms.value

    def last_occupancy(self) -> int:
        """Blocks per CU the occupancy API admits for the last launch's kernel, block size and LDS (diagnostic)."""
        return int(self._L.wedm_last_occupancy(self._ctx))

    def build_id(self) -> str:
        return build_id()

    def close(self) -> None:
        if self._ctx:
            self._L.wedm_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
