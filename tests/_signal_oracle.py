"""The expected values of the signal-statistics block (include/wedm_hip.h, enum wedm_sig_field), formed from
microsecond-by-microsecond runs of the CPU oracle as it stands.

TEST SEAM ONLY, like ``tests/_oracle_backend.py``.  `SignalOracleBackend` is `OracleBackendRows` with ``bind_signal_stats``:
a launch of ``n`` physics steps is run as ``n`` oracle launches of one step, and after each of them the bound rows are
updated in NumPy float64, elementwise over the batch -- one addition per sample, so the order of the summation is the
kernels' (never ``np.sum`` over time).  What a fused launch does once per launch is kept per launch here: the next-step
autoreset (only the first of the single steps may perform it) and the progress reward (formed from the launch's first
and last workpiece position).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from sparc_amd import _abi
from tests._oracle_backend import OracleBackendRows

S = _abi.SIG
_ACC = slice(int(S.SAMPLES_ACC), int(S.TMAX_PEAK_ACC) + 1)
_LAST = slice(int(S.SAMPLES_LAST), int(S.TMAX_PEAK_LAST) + 1)
IDENTITIES = np.array([0.0, 0.0, 0.0, 0.0, np.inf, -np.inf])


class SignalOracleBackend(OracleBackendRows):
    name = "oracle-signal"
    n_threads = 1   # launches of one step on test-sized batches: a thread team per call costs more than it saves

    def __init__(self, params, num_envs, n_seg_max, device):
        super().__init__(params, num_envs, n_seg_max, device)
        self._sig = None
        self._launch_open = False   # a launch is under way and its first single step has run

    def bind_signal_stats(self, rows_ptr):
        self._sig = rows_ptr

    # ------------------------------------------------------------------ views of the caller's blocks
    def _sig_rows(self):
        return np.ctypeslib.as_array(C.cast(self._sig, C.POINTER(C.c_double)), shape=(_abi.SIG_COUNT, self.state.stride))

    def _f64(self):
        return self._block(self.state.f64, C.c_double, _abi.F64_COUNT)[:, : self.num_envs]

    def _i8(self):
        return self._block(self.state.i8, C.c_int8, _abi.I8_COUNT)[:, : self.num_envs]

    def _reset_rows(self, m):
        """The reset rule for the environments of the bool mask `m`: accumulators to their identities, published rows to 0."""
        rows = self._sig_rows()[:, : self.num_envs]
        rows[_ACC, m] = IDENTITIES[:, None]
        rows[_LAST, m] = 0.0

    # ------------------------------------------------------------------ the backend's calls
    def reset(self, mask_ptr, seed, reseed, fresh=False):
        super().reset(mask_ptr, seed, reseed, fresh)
        if self._sig is None:
            return
        if mask_ptr is None:
            m = np.ones(self.num_envs, dtype=bool)
        else:
            m = np.ctypeslib.as_array(C.cast(mask_ptr, C.POINTER(C.c_uint8)), shape=(self.num_envs,)).astype(bool)
        self._reset_rows(m)

    def step(self, n_substeps, action):
        if n_substeps <= 0:
            return super().step(n_substeps, action)
        p = self.params
        done0 = self._i8()[_abi.I8.DONE] != 0
        reset0 = done0 & bool(p.autoreset)
        frozen0 = done0 & (not p.autoreset) & (not p.keep_stepping_terminated)
        wp0 = np.where(reset0, p.initial_gap, self._f64()[_abi.F64.WORKPIECE_POS])
        autoreset = p.autoreset
        self._launch_open = False
        try:
            super().step(n_substeps, action)
        finally:
            p.autoreset = autoreset
            self._launch_open = False
        if p.reward_mode and self.state.reward:  # the launch's reward, as wedm_step writes it
            reward = np.ctypeslib.as_array(C.cast(self.state.reward, C.POINTER(C.c_float)), shape=(self.state.stride,))
            broken = self._i8()[_abi.I8.WIRE_BROKEN] != 0
            r = (self._f64()[_abi.F64.WORKPIECE_POS] - wp0).astype(np.float32) - \
                np.float32(p.reward_break_penalty) * broken.astype(np.float32)
            reward[: self.num_envs] = np.where(frozen0, np.float32(0.0), r)

    def _run(self, n_substeps, action):
        p = self.params
        for _ in range(n_substeps):
            if self._launch_open:
                p.autoreset = 0      # a fused launch resets terminated environments when it begins, and only then
            done = self._i8()[_abi.I8.DONE] != 0
            reset_now = done & bool(p.autoreset)
            ran = ~done | reset_now | bool(p.keep_stepping_terminated)
            super()._run(1, action)
            self._launch_open = True
            if self._sig is not None:
                if reset_now.any():
                    self._reset_rows(reset_now)
                self._tally(ran)

    def _tally(self, ran):
        """One sample of every environment of `ran`: the state after the step it just ran."""
        n = self.num_envs
        f64, i8 = self._f64(), self._i8()
        rows = self._sig_rows()[:, :n]
        V, I = f64[_abi.F64.VOLTAGE], f64[_abi.F64.CURRENT]
        gap = f64[_abi.F64.WORKPIECE_POS] - f64[_abi.F64.WIRE_POS]
        tmax = f64[_abi.F64.TMAX]
        energy = V * I   # rounded to float64 before it is added
        acc = rows[_ACC].copy()
        acc[0] = acc[0] + 1.0
        acc[1] = acc[1] + I
        acc[2] = acc[2] + energy
        acc[3] = acc[3] + gap
        acc[4] = np.minimum(acc[4], gap)
        acc[5] = np.maximum(acc[5], tmax)
        rows[_ACC] = np.where(ran, acc, rows[_ACC])
        pub = ran & (i8[_abi.I8.CTRL_STEP] != 0)
        if not pub.any():
            return
        rows[_LAST] = np.where(pub, rows[_ACC], rows[_LAST])
        rows[_ACC] = np.where(pub, IDENTITIES[:, None], rows[_ACC])
        base = _abi.OBS_DIM + (len(_abi.PULSE_OBS_NAMES) if self._pulse is not None else 0)
        if self.state.obs and int(self.params.obs_dim) >= base + len(_abi.SIGNAL_OBS_NAMES):
            obs = np.ctypeslib.as_array(C.cast(self.state.obs, C.POINTER(C.c_float)),
                                        shape=(self.params.obs_dim, self.state.stride))[:, :n]
            last = rows[_LAST]
            for k in range(5):   # current sum, energy sum, gap sum, gap minimum, peak temperature: rows 1 .. 5 of the six
                obs[base + k] = np.where(pub, last[1 + k].astype(np.float32), obs[base + k])

    def last_kernel(self):
        return super().last_kernel() + ("[sig]" if self._sig is not None else "")


def signal_rows(env):
    """``float64 [SIG_COUNT, num_envs]`` host copy of an environment's signal block."""
    return env.state.signal[:, : env.num_envs].detach().cpu().numpy().copy()
