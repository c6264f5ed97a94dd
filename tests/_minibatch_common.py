"""What tests/test_minibatch_host.py (CPU oracle backends, the NumPy definition) and tests/test_minibatch.py (MI355X, the
kernels) share: masks of live rows, the properties every drawn index has, and the training stacks of
tests/_optimizer_common.py with a `MinibatchSampler` in place of the loop's ``randperm``.
TEST SEAM ONLY."""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from sparc_amd import MinibatchSampler
from sparc_amd.minibatch import part_bounds
from tests import _optimizer_common as oc
from tests import _resume_common as rc

KL_AT = oc.KL_AT


# ------------------------------------------------------------------------------------------------ masks and properties
def masks(R: int, seed: int) -> Dict[str, Optional[np.ndarray]]:
    """The ``valid`` blocks of a size by name: None (every row live), all live, all dead, only the first row, only the last
    row, about 90 % live with non-zero bytes other than 1, and exactly V live rows for V the largest power of two and the
    largest power of two plus one that fit.  Masks that would repeat an earlier one are left out."""
    rng = np.random.default_rng(seed)
    out: Dict[str, Optional[np.ndarray]] = {"null": None, "all live": np.ones(R, dtype=np.uint8), "all dead": np.zeros(R, dtype=np.uint8)}

    def exactly(V: int) -> np.ndarray:
        m = np.zeros(R, dtype=np.uint8)
        m[rng.permutation(R)[:V]] = rng.choice(np.array([1, 2, 0xFF], dtype=np.uint8), size=V)
        return m

    if R > 1:
        first, last = np.zeros(R, dtype=np.uint8), np.zeros(R, dtype=np.uint8)
        first[0], last[-1] = 1, 0x80
        out.update({"first": first, "last": last})
    if R > 2:
        most = rng.choice(np.array([1, 2, 0xFF], dtype=np.uint8), size=R)
        most[rng.random(R) < 0.1] = 0
        out["most"] = most
        pow2 = 1 << ((R - 1).bit_length() - 1)   # the largest power of two below R
        out["power of two"] = exactly(pow2)
        if pow2 + 1 < R:
            out["power of two plus one"] = exactly(pow2 + 1)
    return out


def check_placement(index: np.ndarray, valid: Optional[np.ndarray], n: int) -> None:
    """The consequences the header names: a permutation of ``[0, R)``; in every part of the sizes of ``tensor_split`` the
    live rows come first; part p holds ``ceil((V - p) / n)`` of them."""
    R = index.shape[0]
    live = np.ones(R, dtype=bool) if valid is None else np.asarray(valid).reshape(-1) != 0
    V = int(live.sum())
    assert index.dtype == np.int64 and np.array_equal(np.sort(index), np.arange(R))
    off, cnt = part_bounds(R, n)
    assert [int(c) for c in cnt] == [t.shape[0] for t in torch.tensor_split(torch.arange(R), n)] and int(off[-1] + cnt[-1]) == R
    for p in range(n):
        part = live[index[off[p]: off[p] + cnt[p]]]
        want = max(0, -(-(V - p) // n))
        assert int(part.sum()) == want and bool(part[:want].all()), (p, want)


# ------------------------------------------------------------------------------------------------ the stack
N_PARTS = 2


class MbStack(oc.OptStack):
    """An `OptStack` whose epochs take their minibatches from a `MinibatchSampler`."""

    def __init__(self, variant: str, device: str, seeds: dict, kl_limit: Optional[float]):
        super().__init__(variant, device, seeds, kl_limit)
        # (a stack built with other seeds gets another number of parts too: a load has to bring the run's)
        other = seeds is not rc.RUN_SEEDS
        self.mb = MinibatchSampler(self.buf, 3 if other else N_PARTS, seed=seeds["sampler"] ^ (0xFFFF << 48 if other else 0))


def _host(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().clone()


def epoch(st: MbStack, calls: List[dict]) -> None:
    """`tests._optimizer_common.epoch` with ``st.mb.draw()`` where that one makes a permutation on the host: nothing the host
    made enters the epoch."""
    flat = st.buf.flat()
    P = st.head.param_dim
    st.opt.begin_update()
    for part, idx in enumerate(st.mb.draw()):
        st.opt.zero_grad()
        params, value = st.net(flat["obs"][idx])
        stats = st.ppo.backward(params, value, rollout=st.buf, index=idx)
        st.opt.step(stats if st.opt.kl_limit is not None else None)
        B = idx.shape[0]
        calls.append({"step": st.steps, "part": part, "index": _host(idx), "grad": _host(st.ppo._grad[: B * (P + 1)]),
                      "stats": _host(stats.tensor), "info": _host(st.opt.info)})
    st.opt.zero_grad()


def control_step(st: MbStack, steps: List[dict], calls: List[dict]) -> None:
    """`tests._optimizer_common.control_step` around this module's `epoch`."""
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


def run(st: MbStack, upto: int, steps: List[dict], calls: List[dict]) -> None:
    while st.steps < upto:
        control_step(st, steps, calls)
    st.env.check_errors()


def everything(st: MbStack) -> Dict[str, torch.Tensor]:
    out = oc.everything(st)
    out.update({"mb.index": _host(st.mb.index), "mb.count": _host(st.mb.count),
                "mb.seed_parts_draws": torch.from_numpy(np.array([st.mb.seed, st.mb.n_parts, st.mb.draws], dtype=np.uint64).view(np.int64).copy())})
    return out


def save(st: MbStack, path) -> None:
    oc.save(st, path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    ck["mb"] = st.mb.state_dict()
    torch.save(ck, path)


def load(st: MbStack, path) -> None:
    oc.load(st, path)
    st.mb.load_state_dict(torch.load(path, map_location="cpu", weights_only=True)["mb"])


_LIMITS: dict = {}


def kl_limit_of(variant: str) -> float:
    """`tests._optimizer_common.kl_limit_of` for this module's minibatches: `KL_LIMIT_SCALE` times the first non-zero
    approximate KL of the run without a gate on the oracle backend, once per variant."""
    if variant not in _LIMITS:
        st = MbStack(variant, "cpu", rc.RUN_SEEDS, None)
        calls: List[dict] = []
        try:
            run(st, rc.T + 1, [], calls)
        finally:
            st.close()
        kls = [float(c["stats"][KL_AT]) for c in calls]
        assert len(kls) == 2 and kls[0] == 0.0 and kls[1] > 0.0 and np.isfinite(kls[1]), kls
        _LIMITS[variant] = oc.KL_LIMIT_SCALE * kls[1]
    return _LIMITS[variant]


CALL_BLOCKS = ("index", "grad", "stats", "info")


def assert_calls_equal(got_calls: List[dict], want_calls: List[dict], where: str) -> None:
    assert [(c["step"], c["part"]) for c in got_calls] == [(c["step"], c["part"]) for c in want_calls]
    for got, want in zip(got_calls, want_calls):
        rc.assert_equal({n: got[n] for n in CALL_BLOCKS}, {n: want[n] for n in CALL_BLOCKS}, f"{where}: call after step {want['step']}")


def check_drawn(st_valid: torch.Tensor, calls: List[dict]) -> None:
    """The parts a run recorded are what the definition deals: an epoch's parts together are a permutation."""
    R = st_valid.numel()
    for a, b in zip(calls[::N_PARTS], calls[1::N_PARTS]):
        both = torch.cat([a["index"], b["index"]]).numpy()
        assert np.array_equal(np.sort(both), np.arange(R))


def run_whole(variant: str, device: str):
    """The uninterrupted run of ``K`` control steps with the gate: (steps, calls, everything at the end)."""
    st = MbStack(variant, device, rc.RUN_SEEDS, kl_limit_of(variant))
    steps, calls = [], []
    try:
        run(st, rc.K, steps, calls)
        check_drawn(st.buf.computed["valid"], calls)
        return steps, calls, everything(st)
    finally:
        st.close()


def check_resume_at_every_cut(variant: str, device: str, folder) -> None:
    """`tests._optimizer_common.check_resume_at_every_cut` with the sampler's dict among the checkpoint's, its blocks among
    `everything` and every drawn index among the recorded calls."""
    limit = kl_limit_of(variant)
    st = MbStack(variant, device, rc.RUN_SEEDS, limit)
    steps: List[dict] = []
    calls: List[dict] = []
    paths = []
    for k in rc.CUTS:
        run(st, k, steps, calls)
        paths.append(folder / f"mb-{variant}-{k}.pt")
        save(st, paths[-1])
    run(st, rc.K, steps, calls)
    end = everything(st)
    check_drawn(st.buf.computed["valid"], calls)
    st.close()
    oc.assert_gate_worked(calls)
    assert st.mb.draws == 2
    for k in rc.CUTS:
        other = MbStack(variant, device, rc.OTHER_SEEDS, limit)
        try:
            run(other, 2, [], [])
            load(other, paths[k])
            got_steps, got_calls = [], []
            run(other, rc.K, got_steps, got_calls)
            for i, (got, want) in enumerate(zip(got_steps, steps[k:])):
                rc.assert_equal(got, want, f"{variant}, cut {k}: what control step {k + i + 1} handed out")
            assert_calls_equal(got_calls, [c for c in calls if c["step"] >= k], f"{variant}, cut {k}")
            rc.assert_equal(everything(other), end, f"{variant}, cut {k}: everything after control step {rc.K}")
        finally:
            other.close()
