"""What tests/test_policy_net_host.py (CPU oracle backends, the NumPy definition), tests/test_policy_net.py and
tests/test_policy_net_shapes.py (MI355X, the kernels) share: synthetic calls of `wedm_policy_net` with their expected blocks,
a mirror of the kernels' LDS plan, and the training stacks of tests/_resume_common.py with a `PolicyNet` as the network
(DESIGN.md section 4.22).  TEST SEAM ONLY."""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from sparc_amd import PolicyNet
from sparc_amd.policy_net import layout, policy_net_reference
from tests import _resume_common as rc

EXTRA = 37   # entries of a store beyond the call's rows
OUTSIDE = (-1, -2 ** 63, 2 ** 40, 2 ** 63 - 1)   # and n_src itself: indices that name no entry


def draw_call(rows: int, D: int, hidden, M: int, index: Optional[str], seed: int, obs_pad: int = 0, grad_pad: int = 0) -> dict:
    """Host blocks of one call: asymmetric random ``theta``, a store of observations (``rows + EXTRA`` entries with an index,
    NaN in its padding columns), ``index`` (None, "perm": distinct entries, "repeats": repeats and entries outside the
    store), ``grad_params`` (NaN in its padding columns) and ``grad_value``."""
    rng = np.random.default_rng(seed)
    P = 8 + M
    n_theta = layout(D, hidden, M)["n_theta"][0]
    n_src = rows + EXTRA if index else rows
    obs = np.full((n_src, D + obs_pad), np.nan, dtype=np.float32)
    obs[:, :D] = rng.normal(size=(n_src, D))
    gp = np.full((rows, P + grad_pad), np.nan, dtype=np.float32)
    gp[:, :P] = rng.normal(size=(rows, P))
    idx = None
    if index == "perm":
        idx = rng.permutation(n_src)[:rows].astype(np.int64)
    elif index == "repeats":
        idx = rng.integers(0, n_src, size=rows).astype(np.int64)
        idx[:: 3] = idx[0]
        outside = OUTSIDE + (n_src,)
        where = rng.permutation(rows)[: max(1, rows // 7)]
        idx[where] = [outside[i % len(outside)] for i in range(len(where))]
    return {"theta": (0.3 * rng.normal(size=n_theta)).astype(np.float32), "obs": obs, "index": idx, "grad_params": gp,
            "grad_value": rng.normal(size=rows).astype(np.float32), "D": D, "hidden": tuple(hidden), "M": M, "rows": rows}


def define(call: dict, activation: str) -> dict:
    """`policy_net_reference` on a `draw_call`."""
    D = call["D"]
    return policy_net_reference(call["theta"], np.ascontiguousarray(call["obs"][:, :D]), hidden=call["hidden"], n_modes=call["M"],
                                activation=activation, index=call["index"], grad_params=call["grad_params"], grad_value=call["grad_value"])


def lds_plan(D: int, H1: int, H2: int, O: int, backward: bool):
    """`net_make_shape` of sparc_amd/csrc/wedm_policy_net.h, in floats against its 160 KiB: (the parked node lies in LDS,
    ``theta`` is staged in LDS).  The forward parks nothing."""
    limit = 160 * 1024 // 4
    at = 2 * 128 + 128 * (H1 + 4) + 128 * (H2 + 4) + (128 * 36 if backward else 0)   # src, act1, act2, go
    n_theta = (D + 1) * H1 + (H1 + 1) * H2 + (H2 + 1) * O
    park = backward and at + n_theta <= limit
    at += n_theta if park else 0
    staged = (D + 1) * (H1 + 4) + (H1 + 1) * (H2 + 4) + (H2 + 1) * (O + 4)   # rows of N + 4
    return bool(park), at + staged <= limit


# ------------------------------------------------------------------------------------------------ the stack
NET_HIDDEN = (32, 16)


class NetStack(rc.Stack):
    """A stack of tests/_resume_common.py whose network is a `PolicyNet` on the stack's device: ``leaves`` is
    ``[net.theta]``, so the loop's fixed step, the checkpoints and `everything` carry it."""

    def __init__(self, variant: str, device: str, seeds: dict, net_device: Optional[str] = None):
        super().__init__(variant, device, seeds, net_device)
        self.pnet = PolicyNet(self.vec, self.head, hidden=NET_HIDDEN, activation="tanh", seed=seeds["net"])
        self.leaves = [self.pnet.theta]

    def net(self, obs: torch.Tensor):
        """(params, value): with a graph inside an epoch, without one in the loop's own no-grad calls."""
        obs = obs if self.norm is not None else obs * self.scale
        params, value = self.pnet(obs) if torch.is_grad_enabled() else self.pnet.forward(obs)
        return params.clone(), value.clone()


def run_whole(variant: str, device: str):
    """The uninterrupted run of ``K`` control steps: (steps, calls, everything at the end)."""
    st = NetStack(variant, device, rc.RUN_SEEDS)
    steps, calls = [], []
    try:
        rc.run(st, rc.K, steps, calls)
        return steps, calls, rc.everything(st)
    finally:
        st.close()


def check_resume_at_every_cut(variant: str, device: str, folder) -> None:
    """The stack is cut after every control step, saved, loaded into a fresh stack built with other seeds, and continued:
    everything it hands out and holds afterwards equals the uninterrupted run's on every byte."""
    st = NetStack(variant, device, rc.RUN_SEEDS)
    steps: List[dict] = []
    calls: List[dict] = []
    paths = []
    for k in rc.CUTS:
        rc.run(st, k, steps, calls)
        paths.append(folder / f"net-{variant}-{k}.pt")
        rc.save(st, paths[-1])
    rc.run(st, rc.K, steps, calls)
    end = rc.everything(st)
    st.close()
    assert len(calls) == 4 and all(bool(c["stats"].isfinite().all()) for c in calls)
    assert any(bool((a["grad"] != 0).any()) for a in calls)
    for k in rc.CUTS:
        other = NetStack(variant, device, rc.OTHER_SEEDS)
        try:
            rc.run(other, 2, [], [])
            rc.load(other, paths[k])
            got_steps, got_calls = [], []
            rc.run(other, rc.K, got_steps, got_calls)
            for i, (got, want) in enumerate(zip(got_steps, steps[k:])):
                rc.assert_equal(got, want, f"{variant}, cut {k}: what control step {k + i + 1} handed out")
            want_calls = [c for c in calls if c["step"] >= k]
            assert [(c["step"], c["part"]) for c in got_calls] == [(c["step"], c["part"]) for c in want_calls]
            for got, want in zip(got_calls, want_calls):
                rc.assert_equal({n: got[n] for n in ("grad", "stats")}, {n: want[n] for n in ("grad", "stats")}, f"{variant}, cut {k}")
            rc.assert_equal(rc.everything(other), end, f"{variant}, cut {k}: everything after control step {rc.K}")
        finally:
            other.close()
