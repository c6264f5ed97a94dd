"""Guard arenas for the memory contract of the C-ABI (include/wedm_hip.h, "What a launch writes").

TEST SEAM ONLY.  `guarded(env)` moves every caller-owned block of an existing ``WireEDMEnv`` into a larger arena of the
same dtype, with a guard band before and after the block, everything pre-filled with the byte 0xA5, and binds the new
addresses through the backend's own calls.  `Guard.snapshot()` returns every arena as bytes and
`Guard.assert_only_owned_changed(before, after)` asserts that two snapshots differ only in the bytes the ABI gives the
library: columns ``[0, num_envs)`` of the rows of the state blocks (and of the pulse block), and the whole of a bound
trace ring.  The padding columns ``[num_envs, stride)``, both bands and every byte of the geometry, env-param and
wire-material rows must be unchanged.

With ``stride=`` the blocks are re-laid to another row stride (any ``stride >= num_envs``: the header allows it, the
Python layer itself only ever uses multiples of 64).  The environment's setters that write whole rows (`set_env_params`,
`set_wire_material`) assume the default stride: call them before `guarded`.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from sparc_amd import _abi

FILL = 0xA5
MIN_BAND_BYTES = 4096
STATE_BLOCKS = ("f64", "i32", "i8", "T", "obs", "stats", "reward", "crater_log", "pulse")   # written: columns [0, num_envs)
CONST_BLOCKS = ("_geom_f64", "_geom_i32", "_envp_rows", "_wmat_rows")                     # never written
REGIONS = ("before-band", "padding column", "after-band", "read-only column")


class Arena:
    """One block inside its arena: ``[rows][width][inner]`` elements of ``dtype`` starting ``lead`` elements into
    ``full``; the library owns columns ``[0, owned)`` of every row."""

    def __init__(self, name: str, like: torch.Tensor, width: int, owned: int, live: Optional[int] = None):
        shape = tuple(like.shape)
        self.name, self.rows, self.width, self.owned = name, shape[0], int(width), int(owned)
        self.live = self.owned if live is None else int(live)   # columns that hold an environment (a read-only block owns none)
        self.inner = int(np.prod(shape[2:])) if len(shape) > 2 else 1
        self.itemsize = like.element_size()
        row = self.width * self.inner
        band = max(2 * row, -(-MIN_BAND_BYTES // self.itemsize))
        self.lead = -(-band // 16) * 16          # (the block keeps the 16-byte alignment the T words need)
        self.count = self.rows * row
        raw = torch.full(((2 * self.lead + self.count) * self.itemsize,), FILL, dtype=torch.uint8, device=like.device)
        self.raw = raw
        self.full = raw.view(like.dtype)
        self.view = self.full[self.lead: self.lead + self.count].view((self.rows, self.width) + shape[2:])
        assert self.view.data_ptr() % 16 == 0

    def owned_mask(self) -> np.ndarray:
        """bool per BYTE of the arena: what a launch may change."""
        m = np.zeros((self.rows, self.width, self.inner * self.itemsize), dtype=bool)
        m[:, : self.owned] = True
        out = np.zeros(self.raw.numel(), dtype=bool)
        lo = self.lead * self.itemsize
        out[lo: lo + m.size] = m.reshape(-1)
        return out

    def locate(self, byte: int):
        """(region, row, column) of a byte of the arena; rows count from the block's first row (negative: before it)."""
        rel = byte // self.itemsize - self.lead
        row_elems = self.width * self.inner
        row, col = rel // row_elems, (rel % row_elems) // self.inner
        if rel < 0:
            return "before-band", row, col
        if rel >= self.count:
            return "after-band", row, col
        return ("padding column" if col >= self.live else "read-only column"), row, col


def _relaid(arena: Arena, old: torch.Tensor) -> None:
    """The block's current contents into the arena: all of its columns where the stride stays, else what fits (the
    columns past the old block repeat its last one, as the host lays out its padding)."""
    w = min(arena.width, old.shape[1])
    arena.view[:, :w] = old[:, :w]
    if arena.width > w:
        arena.view[:, w:] = old[:, w - 1: w]


class Guard:
    def __init__(self, env, stride: Optional[int] = None):
        st = env.state
        n = env.num_envs
        stride = int(st.stride if stride is None else stride)
        if stride < n:
            raise ValueError("stride < num_envs")
        self.env, self.num_envs, self.stride = env, n, stride
        self.arenas: Dict[str, Arena] = {}
        for name in STATE_BLOCKS:
            old = getattr(st, name)
            if old is None:
                continue
            a = self.arenas[name] = Arena(name, old, stride, n)
            _relaid(a, old)
            object.__setattr__(st, name, a.view)
        for name in CONST_BLOCKS:
            old = getattr(env, name, None)
            if old is None:
                continue
            a = self.arenas[name] = Arena(name, old, stride, 0, live=n)
            _relaid(a, old)
            setattr(env, name, a.view)
        object.__setattr__(st, "b", st.i8.view(torch.bool))
        object.__setattr__(st, "stride", stride)
        st.__dict__["_views"].clear()
        env._reward = st.reward[0, :n]
        env._step_out = None
        be = env._backend
        be.bind_state(st.pointers(with_obs=True))
        if env.per_env_geometry:
            be.bind_geometry(_abi.GeomPtrs(env._geom_f64.data_ptr(), env._geom_i32.data_ptr()))
        if st.pulse is not None:
            be.bind_pulse_stats(st.pulse.data_ptr())
        if env._envp_rows is not None:
            be.bind_env_params(env._envp_rows.data_ptr())
        if env._wmat_rows is not None:
            be.bind_wire_material(env._wmat_rows.data_ptr())

    def guard_trace(self, trace) -> None:
        """Move the rings of a trace just bound with ``env.bind_trace`` into arenas and bind the descriptor again (which
        restarts its sample counter at zero, where it still is).  A ring is dense -- ``[capacity][rows][env_count]`` is
        exactly the slots and the environment window its descriptor names --, so all of it is the library's."""
        assert self.env._trace is trace and trace.count == 0
        for key in ("f64", "i32", "i8"):
            old = trace._buf[key]
            if old is not None:
                a = self.arenas[f"trace.{key}"] = Arena(f"trace.{key}", old, old.shape[1], old.shape[1])
                a.view.copy_(old)
                trace._buf[key] = a.view
        if trace._T is not None:
            a = self.arenas["trace.T"] = Arena("trace.T", trace._T, trace._T.shape[1], trace._T.shape[1])
            a.view.copy_(trace._T)
            trace._T = a.view
        d = trace.desc
        ptr = lambda t: t.data_ptr() if t is not None else None
        trace.desc = _abi.TraceDesc(ptr(trace._buf["f64"]), ptr(trace._buf["i32"]), ptr(trace._buf["i8"]), ptr(trace._T),
                                    d.f64_mask, d.i32_mask, d.i8_mask, d.env_lo, d.env_count, d.every, d.capacity, 0)
        self.env._backend.bind_trace(trace.desc)

    def snapshot(self) -> Dict[str, np.ndarray]:
        """Every arena, bands included, as bytes (host copies)."""
        if self.env.device.type == "cuda":
            torch.cuda.synchronize(self.env.device)
        return {name: a.raw.cpu().numpy().copy() for name, a in self.arenas.items()}

    def violations(self, before, after) -> List[str]:
        kernel = self.env._backend.last_kernel()
        out = []
        for name, a in self.arenas.items():
            bad = (before[name] != after[name]) & ~a.owned_mask()
            if not bad.any():
                continue
            idx = np.flatnonzero(bad)
            seen = set()
            for byte in idx:   # the first byte of every region that was hit
                region, row, col = a.locate(int(byte))
                if region in seen:
                    continue
                seen.add(region)
                cnt = sum(1 for b in idx if a.locate(int(b))[0] == region) if idx.size <= 4096 else idx.size
                out.append(f"{name}: {region} written: row {row} column {col} (byte {int(byte)} of the arena, "
                           f"0x{int(before[name][byte]):02x} -> 0x{int(after[name][byte]):02x}; {cnt} bytes"
                           f"{'' if idx.size <= 4096 else ' in all regions'}); kernel {kernel}")
        return out

    def assert_only_owned_changed(self, before, after) -> None:
        bad = self.violations(before, after)
        assert not bad, "\n".join(bad[:20])


def guarded(env, stride: Optional[int] = None) -> Guard:
    return Guard(env, stride)


# ---- read-only inputs that need no arena: clone before the launch, compare every byte after it
def clone_inputs(*tensors):
    return [t.detach().clone() for t in tensors]


def assert_inputs_unchanged(names, tensors, clones, kernel="") -> None:
    for name, t, c in zip(names, tensors, clones):
        same = torch.equal(t.contiguous().view(torch.uint8), c.contiguous().view(torch.uint8))
        assert same, f"{name}: read-only input written; kernel {kernel}"


def action_leaves(act):
    names = ("servo", "target_voltage", "on_time", "off_time", "current_mode")
    return [f"action.{k}" for k in names], [getattr(act, k) for k in names]
