"""What tests/test_optimizer_host.py (CPU oracle backends, the NumPy definition) and tests/test_optimizer.py (MI355X, the
kernels) share: synthetic calls of `wedm_adam` with their expected blocks, and the training stacks of
tests/_policy_net_common.py with an `Adam` in place of the loop's fixed step.  TEST SEAM ONLY."""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from sparc_amd import Adam, _abi
from sparc_amd.optimizer import FRESH_STATE, adam_reference
from tests import _policy_net_common as pc
from tests import _resume_common as rc

HYPER = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-5)
MAX_NORM, WEIGHT_DECAY = 0.5, 0.01
PHASES = _abi.OPT_NORM | _abi.OPT_DECIDE | _abi.OPT_APPLY
FORMS = {"one": (0,), "phased": (PHASES,), "separate": (_abi.OPT_NORM, _abi.OPT_DECIDE, _abi.OPT_APPLY)}
KL_AT = _abi.PPO_STAT_NAMES.index("approx_kl")


def draw_start(n: int, seed: int) -> Dict[str, np.ndarray]:
    """Host blocks before the first call: random ``theta``, moments as some earlier steps left them, the state after three
    applied steps, and a stats block of a PPO loss whose ``approx_kl`` is 0.01."""
    rng = np.random.default_rng(seed)
    state = np.array(FRESH_STATE)
    state[:3] = HYPER["betas"][0] ** 3, HYPER["betas"][1] ** 3, 3.0
    stats = rng.normal(size=_abi.PPO_STATS)
    stats[KL_AT] = 0.01
    return {"theta": rng.normal(size=n).astype(np.float32), "m": (0.01 * rng.normal(size=n)).astype(np.float32),
            "v": (1e-4 * rng.random(n)).astype(np.float32), "state": state, "stats": stats}


def draw_grads(n: int, seed: int, steps: int = 3) -> List[np.ndarray]:
    """Gradients whose norms are about 0.3, 2 and 0.45: under, over and under a ``max_norm`` of 0.5."""
    rng = np.random.default_rng(seed + 1)
    return [(f * rng.normal(size=n) / np.sqrt(n)).astype(np.float32) for f in (0.3, 2.0, 0.45, 1.0, 0.2)[:steps]]


def reference_step(host: Dict[str, np.ndarray], grad: np.ndarray, *, clip: bool, decay: bool, kl_limit: Optional[float] = None,
                   new_update: bool = False, **hyper) -> Dict[str, np.ndarray]:
    """`adam_reference` on copies: every block as the call has to leave it."""
    out = {k: v.copy() for k, v in host.items()}
    out["info"], out["partials"] = adam_reference(
        out["theta"], out["m"], out["v"], grad, out["state"], **{**HYPER, **hyper}, weight_decay=WEIGHT_DECAY if decay else 0.0,
        max_norm=MAX_NORM if clip else None, kl=out["stats"][KL_AT], kl_limit=kl_limit, new_update=new_update)
    out["grad"] = grad.copy()
    return out


# ------------------------------------------------------------------------------------------------ the stack
KL_LIMIT_SCALE = 0.5   # the gate's limit, as a part of the first non-zero approximate KL of the run without a gate


class OptStack(pc.NetStack):
    """A `NetStack` whose network is moved by an `Adam` with clipping and a KL gate."""

    def __init__(self, variant: str, device: str, seeds: dict, kl_limit: Optional[float], lr=None):
        super().__init__(variant, device, seeds)
        # (a stack built with other seeds gets other hyperparameters too: a load has to bring the run's)
        other = seeds is not rc.RUN_SEEDS
        self.opt = Adam(self.pnet, lr=lr if lr is not None else (lambda k: 1e-2 / (1 + k)), betas=(0.8, 0.9) if other else (0.9, 0.999),
                        max_grad_norm=0.7 if other else 0.5, kl_limit=kl_limit if not other or kl_limit is None else 2 * kl_limit + 1.0)


def _host(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().clone()


def epoch(st: OptStack, calls: List[dict]) -> None:
    """`tests._resume_common.epoch` with ``opt.begin_update()`` before the minibatches and ``opt.step(stats)`` as the step."""
    flat = st.buf.flat()
    rows, P = rc.T * st.vec.num_envs, st.head.param_dim
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(1000 + st.steps)).to(st.device)
    st.opt.begin_update()
    for part, idx in enumerate(torch.tensor_split(perm, 2)):
        st.opt.zero_grad()
        params, value = st.net(flat["obs"][idx])
        stats = st.ppo.backward(params, value, rollout=st.buf, index=idx)
        st.opt.step(stats if st.opt.kl_limit is not None else None)
        B = idx.shape[0]
        calls.append({"step": st.steps, "part": part, "grad": _host(st.ppo._grad[: B * (P + 1)]), "stats": _host(stats.tensor),
                      "info": _host(st.opt.info)})
    st.opt.zero_grad()


def control_step(st: OptStack, steps: List[dict], calls: List[dict]) -> None:
    """`tests._resume_common.control_step` around this module's `epoch`."""
    if st.pending:
        epoch(st, calls)
        st.pending = False
    with torch.no_grad():
        params, value = st.net(st.obs)
        out = st.head.sample(params)
        nxt, reward, term, trunc, info = st.vec.step(out.action)
        st.buf.add(st.obs, st.head.stored(out), value, reward, term, trunc, log_prob=out.log_prob)
        rec = {"obs": _host(nxt), "reward": _host(reward), "terminated": _host(term), "truncated": _host(trunc),
               "episode": _host(info["episode"])}
        if st.norm is not None:
            rec.update({f"episode_stats.{k}": _host(v) for k, v in info["episode_stats"].items()})
            rec.update(raw_observation=_host(info["raw_observation"]), raw_reward=_host(info["raw_reward"]))
        steps.append(rec)
        st.obs = nxt.clone()
        st.steps += 1
        if st.steps % rc.T == 0:
            st.buf.finish(st.net(st.obs)[1])
            st.pending = True


def run(st: OptStack, upto: int, steps: List[dict], calls: List[dict]) -> None:
    while st.steps < upto:
        control_step(st, steps, calls)
    st.env.check_errors()


def everything(st: OptStack) -> Dict[str, torch.Tensor]:
    out = rc.everything(st)
    out.update({"opt.m": _host(st.opt.m), "opt.v": _host(st.opt.v), "opt.state": _host(st.opt.state),
                "opt.calls": torch.tensor([st.opt.calls])})
    return out


def save(st: OptStack, path) -> None:
    rc.save(st, path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    ck["opt"] = st.opt.state_dict()
    torch.save(ck, path)


def load(st: OptStack, path) -> None:
    rc.load(st, path)
    st.opt.load_state_dict(torch.load(path, map_location="cpu", weights_only=True)["opt"])


_LIMITS: dict = {}


def kl_limit_of(variant: str) -> float:
    """`KL_LIMIT_SCALE` times the first non-zero approximate KL of the run without a gate on the oracle backend, computed
    once per variant: the first minibatch of an epoch has a KL of exactly 0 (the ratios are 1) and is applied, the
    second one's KL is that value, over the limit, and is skipped."""
    if variant not in _LIMITS:
        st = OptStack(variant, "cpu", rc.RUN_SEEDS, None)
        calls: List[dict] = []
        try:
            run(st, rc.T + 1, [], calls)
        finally:
            st.close()
        kls = [float(c["stats"][KL_AT]) for c in calls]
        assert len(kls) == 2 and kls[0] == 0.0 and kls[1] > 0.0 and np.isfinite(kls[1]), kls
        _LIMITS[variant] = KL_LIMIT_SCALE * kls[1]
    return _LIMITS[variant]


def run_whole(variant: str, device: str):
    """The uninterrupted run of ``K`` control steps with the gate: (steps, calls, everything at the end)."""
    st = OptStack(variant, device, rc.RUN_SEEDS, kl_limit_of(variant))
    steps, calls = [], []
    try:
        run(st, rc.K, steps, calls)
        return steps, calls, everything(st)
    finally:
        st.close()


def assert_gate_worked(calls: List[dict]) -> None:
    applied = [float(c["info"][4]) for c in calls]
    assert len(calls) == 4 and 0.0 in applied and 1.0 in applied, applied
    assert all(bool(c["stats"].isfinite().all()) for c in calls) and any(bool((c["grad"] != 0).any()) for c in calls)


def check_resume_at_every_cut(variant: str, device: str, folder) -> None:
    """`tests._policy_net_common.check_resume_at_every_cut` with the `Adam`'s dict among the checkpoint's and its blocks
    among `everything`."""
    limit = kl_limit_of(variant)
    st = OptStack(variant, device, rc.RUN_SEEDS, limit)
    steps: List[dict] = []
    calls: List[dict] = []
    paths = []
    for k in rc.CUTS:
        run(st, k, steps, calls)
        paths.append(folder / f"opt-{variant}-{k}.pt")
        save(st, paths[-1])
    run(st, rc.K, steps, calls)
    end = everything(st)
    st.close()
    assert_gate_worked(calls)
    for k in rc.CUTS:
        other = OptStack(variant, device, rc.OTHER_SEEDS, limit)
        try:
            run(other, 2, [], [])
            load(other, paths[k])
            got_steps, got_calls = [], []
            run(other, rc.K, got_steps, got_calls)
            for i, (got, want) in enumerate(zip(got_steps, steps[k:])):
                rc.assert_equal(got, want, f"{variant}, cut {k}: what control step {k + i + 1} handed out")
            want_calls = [c for c in calls if c["step"] >= k]
            assert [(c["step"], c["part"]) for c in got_calls] == [(c["step"], c["part"]) for c in want_calls]
            for got, want in zip(got_calls, want_calls):
                rc.assert_equal({n: got[n] for n in ("grad", "stats", "info")}, {n: want[n] for n in ("grad", "stats", "info")},
                                f"{variant}, cut {k}")
            rc.assert_equal(everything(other), end, f"{variant}, cut {k}: everything after control step {rc.K}")
        finally:
            other.close()
