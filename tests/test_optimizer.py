"""Adam with clipping and a KL gate on the MI355X (sparc_amd/csrc/wedm_adam.h, sparc_amd/optimizer.py, DESIGN.md section
4.23): `wedm_adam` against `adam_reference` on every byte of one arena per block -- guard bands, the gradient and the KL
left alone, ``partials``, ``state``, ``info`` -- at the wave, tile and block edges and on either side of the one-block
threshold, in the one-block form, the phased form and the phases in three calls, and up to the cap of 1 048 576; hostile
values; the gate; repeats; an update without a host synchronisation or an allocation; the call on a side stream behind a
gate; and a whole training run on the GPU against the same run on the oracle backend."""
from __future__ import annotations

import ctypes as C
import gc
import itertools
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sparc_amd import Adam, _abi, _lib
from sparc_amd.optimizer import APPLIED, LATCH, MAX_N, SCALE, SKIPPED_KL, SKIPPED_NONFINITE, SUMSQ, T
from tests import _optimizer_common as oc
from tests import _resume_common as rc
from tests._arena import FILL, Arena
from tests._normalize_common import same_bits
from tests._stream_gate import Gate, check_control, gated, seconds_on
from tests.test_policy_net import _stack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent
ONE = _abi.OPT_ONE_BLOCK_MAX
SIZES = (1, 63, 64, 255, 256, 257, 1025, 6418, ONE, ONE + 1, 65537)
# 2049 tiles (half of DECIDE's tree is padding), 4096 tiles with a last tile of one element, and the cap, where the tree's
# 4096 doubles are full to the last word; the call accepts them in the phased form and the phases in three calls
LARGE = (524_289, 1_048_321, MAX_N)
EVERY_BYTE = [(n, form) for form in oc.FORMS for n in SIZES + LARGE if n not in LARGE or form != "one"]
BLOCKS = ("theta", "m", "v", "grad", "partials", "state", "info", "stats")


def device_adam(desc) -> None:
    _lib.call_stateless(_lib.load().wedm_adam, torch.device(DEV), C.byref(desc))


class Problem:
    """The blocks of one optimiser on the device, each inside an arena of 0xA5 bytes (tests/_arena.py) and ``shift`` bytes past
    a 16-byte boundary (the float64 blocks: 8 bytes where ``shift`` is 12); ``host`` is what every block has to hold."""

    def __init__(self, n: int, seed: int, shift: int = 0):
        self.n, self.tiles = n, -(-n // 256)
        start = oc.draw_start(n, seed)
        host = dict(start, grad=np.zeros(n, dtype=np.float32))
        for name, count in (("partials", self.tiles), ("info", _abi.OPT_INFO)):
            host[name] = np.empty(count, dtype=np.float64)
            host[name].view(np.uint8)[:] = FILL
        self.host, self.arena, self.view, self.lead = host, {}, {}, {}
        for name in BLOCKS:
            a = host[name]
            lead = shift // 4 if a.dtype == np.float32 else (1 if shift == 12 else 0)
            like = torch.empty((1, lead + a.shape[0]), dtype=torch.from_numpy(a).dtype, device=DEV)
            self.arena[name] = arena = Arena(name, like, like.shape[1], like.shape[1])
            self.lead[name], self.view[name] = lead, arena.view[0, lead:]
            self.view[name].copy_(torch.from_numpy(a))
        torch.cuda.synchronize()
        self.image = {name: self.arena[name].raw.cpu().numpy().copy() for name in BLOCKS}   # every byte, bands included

    def put(self, name: str, host: np.ndarray) -> None:
        """An input block as the test sets it (the expected image follows)."""
        self.host[name] = host.copy()
        self.view[name].copy_(torch.from_numpy(host))
        self._into_image(name)

    def _into_image(self, name: str) -> None:
        a, arena = self.host[name], self.arena[name]
        at = (arena.lead + self.lead[name]) * arena.itemsize
        self.image[name][at: at + a.nbytes] = a.view(np.uint8)

    def desc(self, flags: int, *, clip: bool, decay: bool, kl_limit=None, new_update=False, **hyper):
        v, h = self.view, {**oc.HYPER, **hyper}
        flags |= (_abi.OPT_CLIP if clip else 0) | (_abi.OPT_KL_GATE if kl_limit is not None else 0) | (_abi.OPT_NEW_UPDATE if new_update else 0)
        return _abi.OptDesc(theta=v["theta"].data_ptr(), m=v["m"].data_ptr(), v=v["v"].data_ptr(), grad=v["grad"].data_ptr(),
                            partials=v["partials"].data_ptr(), state=v["state"].data_ptr(), info=v["info"].data_ptr(),
                            kl=v["stats"].data_ptr() + 8 * oc.KL_AT, lr=h["lr"], beta1=h["betas"][0], beta2=h["betas"][1], eps=h["eps"],
                            weight_decay=oc.WEIGHT_DECAY if decay else 0.0, max_norm=oc.MAX_NORM if clip else 0.0,
                            kl_limit=0.0 if kl_limit is None else kl_limit, n=self.n, flags=flags)

    def step(self, grad: np.ndarray, form: str, **kw) -> list:
        """One step in ``form``; returns the names of the arenas that differ from the definition in any byte."""
        self.put("grad", grad)
        self.host = oc.reference_step(self.host, grad, **kw)
        for name in BLOCKS:
            self._into_image(name)
        for flags in oc.FORMS[form]:
            device_adam(self.desc(flags, **kw))
        torch.cuda.synchronize()
        return [name for name in BLOCKS if not np.array_equal(self.arena[name].raw.cpu().numpy(), self.image[name])]


@pytest.mark.parametrize("n,form", EVERY_BYTE)
def test_three_steps_are_the_definition_on_every_byte(n, form):
    """`SIZES` in every form, `LARGE` in the phased form and the phases apart; at the large sizes a fourth call whose gradient
    is not finite in its last element -- the last tile, the last word of DECIDE's tree -- which is skipped and counted."""
    grads = oc.draw_grads(n, seed=n)
    shifts = itertools.cycle((0, 4, 12))
    for clip, decay in itertools.product((True, False), repeat=2):
        p = Problem(n, seed=n, shift=next(shifts))
        scales = []
        for k, g in enumerate(grads):
            assert p.step(g, form, clip=clip, decay=decay) == [], (n, form, clip, decay, k)
            assert p.host["info"][APPLIED] == 1.0
            scales.append(float(p.host["info"][SCALE]))
        assert p.host["state"][T] == 6.0 and (np.abs(p.host["m"]).sum() > 0)
        if n >= 63:   # the second gradient's norm lies over max_norm, the others' under it
            assert scales[1] < 1.0 and scales[0] == scales[2] == 1.0 if clip else scales == [1.0] * 3
        if n in LARGE:
            assert p.tiles == (n + 255) // 256 > 2048
            bad = grads[0].copy()
            bad[n - 1] = np.nan if clip else -np.inf
            held = {k: p.host[k].copy() for k in ("theta", "m", "v")}
            assert p.step(bad, form, clip=clip, decay=decay) == [], (n, form, clip, decay, "not finite")
            assert all(same_bits(p.host[k], held[k]) for k in held) and p.host["info"][APPLIED] == 0.0
            assert p.host["state"][SKIPPED_NONFINITE] == 1.0 and p.host["state"][T] == 6.0


@pytest.mark.parametrize("form", tuple(oc.FORMS))
@pytest.mark.parametrize("n", (257, 1025))
def test_hostile_values(n, form):
    """Subnormal and signed-zero gradients and parameters; gradients of 1e38 (the sum of squares stays finite, v becomes +inf
    and theta stands still there); one NaN, one -inf (no byte of theta, m, v is written); a NaN already in theta."""
    rng = np.random.default_rng(n)
    p = Problem(n, seed=n + 1, shift=4)
    theta = p.host["theta"].copy()
    theta[0:20:2], theta[1:20:2], theta[20:30], theta[30] = 0.0, -0.0, np.float32(1e-41), np.float32(-3e-39)
    p.put("theta", theta)
    g = (rng.normal(size=n) * 1e-3).astype(np.float32)
    g[0:40:4], g[1:40:4], g[2:40:4], g[3:40:4] = 0.0, -0.0, np.float32(1e-41), np.float32(-2e-45)
    assert p.step(g, form, clip=True, decay=True) == []
    huge = g.copy()
    huge[100:110] = np.float32(1e38)
    huge[110:120] = np.float32(-1e38)
    before = p.host["theta"].copy()
    assert p.step(huge, form, clip=False, decay=False) == []
    assert np.isfinite(p.host["info"][SUMSQ]) and np.isinf(p.host["v"][100:120]).all() and same_bits(p.host["theta"][100:120], before[100:120])
    assert p.host["info"][APPLIED] == 1.0
    for poison in (np.nan, -np.inf):
        bad = g.copy()
        bad[n - 1] = poison
        held = {k: p.host[k].copy() for k in ("theta", "m", "v")}
        skipped = p.host["state"][SKIPPED_NONFINITE]
        assert p.step(bad, form, clip=True, decay=True) == []
        assert all(same_bits(p.host[k], held[k]) for k in held) and p.host["state"][SKIPPED_NONFINITE] == skipped + 1
    theta = p.host["theta"].copy()
    theta[7] = np.nan
    p.put("theta", theta)
    assert p.step(g, form, clip=True, decay=True) == []
    assert np.isnan(p.host["theta"][7]) and np.isfinite(np.delete(p.host["theta"], np.r_[7, 100:120])).all()


@pytest.mark.parametrize("form", tuple(oc.FORMS))
def test_the_gate_latches_until_a_new_update_with_kl_in_a_ppo_stats_tensor(form):
    """``kl`` points into the stats tensor of a real `PPOLoss` (its own device tensor, which the loss has written)."""
    vec, head, ppo, buf, net = _stack(T=2, hidden=(16, 16))
    idx = torch.arange(64, device=DEV)
    params, value = net(rollout=buf, index=idx)
    stats = ppo.backward(params, value, rollout=buf, index=idx)
    torch.cuda.synchronize()
    assert np.isfinite(float(stats.approx_kl))
    n = 1025
    p = Problem(n, seed=5)
    kl_ptr = stats.tensor.data_ptr() + 8 * oc.KL_AT

    def step(kl, want_applied, **kw):
        stats.tensor[oc.KL_AT] = kl
        host_stats = p.host["stats"].copy()
        host_stats[oc.KL_AT] = kl
        p.host["stats"] = host_stats
        g = oc.draw_grads(n, seed=int(p.host["state"][T] + p.host["state"][SKIPPED_KL]), steps=1)[0]
        p.put("grad", g)
        p.host = oc.reference_step(p.host, g, clip=True, decay=False, kl_limit=0.02, **kw)
        for name in BLOCKS:
            p._into_image(name)
        for flags in oc.FORMS[form]:
            d = p.desc(flags, clip=True, decay=False, kl_limit=0.02, **kw)
            d.kl = kl_ptr
            device_adam(d)
        torch.cuda.synchronize()
        p.image["stats"] = p.arena["stats"].raw.cpu().numpy().copy()   # (this problem's own stats block is not the call's)
        assert [name for name in BLOCKS if not np.array_equal(p.arena[name].raw.cpu().numpy(), p.image[name])] == []
        assert p.host["info"][APPLIED] == want_applied

    step(0.01, 1.0)
    step(0.05, 0.0)
    assert p.host["state"][LATCH] == 1.0
    step(0.0, 0.0)                       # still latched
    step(0.0, 1.0, new_update=True)
    step(float("nan"), 0.0)              # a NaN closes the gate too
    step(0.0, 0.0)
    step(0.03, 0.0, new_update=True)     # a new update whose first minibatch is over the limit
    assert p.host["state"][SKIPPED_KL] == 5.0 and p.host["state"][T] == 5.0
    vec.close()


def test_the_same_call_twice_from_the_same_start_gives_the_same_bits():
    for n in (6418, ONE + 1):
        g = oc.draw_grads(n, seed=3, steps=1)[0]
        outs = []
        for _ in range(2):
            p = Problem(n, seed=9)
            assert p.step(g, "one", clip=True, decay=True) == []
            outs.append({k: p.view[k].clone() for k in BLOCKS})
        assert all(same_bits(outs[0][k], outs[1][k]) for k in BLOCKS)


def test_an_update_neither_synchronises_nor_allocates():
    vec, head, ppo, buf, net = _stack()
    opt = Adam(net, lr=lambda k: 1e-3 / (1 + k), max_grad_norm=0.5, kl_limit=0.02)
    assert opt._native is not None
    parts = torch.tensor_split(torch.randperm(buf.flat()["obs"].shape[0], generator=torch.Generator().manual_seed(2)).to(DEV), 2)

    def update():
        opt.begin_update()
        for idx in parts:
            opt.zero_grad()
            params, value = net(rollout=buf, index=idx)
            stats = ppo.backward(params, value, rollout=buf, index=idx)
            opt.step(stats)
            del params, value, stats

    update()   # buffers grow to their sizes
    torch.cuda.synchronize()
    assert float(opt.state[T]) >= 1.0
    theta = net.theta.detach().clone()
    gc.collect()
    gc.disable()
    torch.cuda.set_sync_debug_mode("error")
    try:
        before = torch.cuda.memory_allocated()
        update()
        after = torch.cuda.memory_allocated()
        assert after == before, (before, after)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        gc.enable()
    torch.cuda.synchronize()
    assert not same_bits(theta, net.theta) and float(opt.state[T] + opt.state[SKIPPED_KL]) == 4.0
    with pytest.raises(RuntimeError, match="grad is None"):
        opt.zero_grad()
        opt.step(ppo.stats)
    vec.close()


GATE_SIZES = (1025, 6418)   # the one-block form and the phased form


def gate_case(n: int) -> None:
    """The call on a side stream behind a gate, as tests/_stream_gate.py describes it; the gradient is the gated input."""
    ga, gb = oc.draw_grads(n, seed=11, steps=2)
    kw = dict(clip=True, decay=True)
    p, control = Problem(n, seed=4), Problem(n, seed=4)
    start = {k: v.copy() for k, v in p.host.items()}
    want_a, want_b = oc.reference_step(start, ga, **kw), oc.reference_step(start, gb, **kw)
    warm = Problem(n, seed=4)
    device_adam(warm.desc(0, **kw))   # warm-up: the code is loaded
    gate = Gate(seconds_on(torch.cuda.current_stream(), lambda: device_adam(warm.desc(0, **kw))))
    p.put("grad", ga)
    gb_dev = torch.from_numpy(gb).to(DEV)
    cdesc = control.desc(0, **kw)
    cdesc.grad = p.desc(0, **kw).grad   # the control reads the same gradient buffer
    gated(gate, lambda: p.view["grad"].copy_(gb_dev, non_blocking=True), lambda: device_adam(p.desc(0, **kw)), lambda: device_adam(cdesc))
    names = ("theta", "m", "v", "partials", "state", "info")
    got = {k: control.view[k] for k in names}
    check_control(all(same_bits(got[k], want_a[k]) for k in names), all(same_bits(got[k], want_b[k]) for k in names), gate, "wedm_adam")
    assert all(same_bits(p.view[k], want_b[k]) for k in names)


def test_the_call_runs_on_the_current_stream_behind_a_gate():
    """Both forms, in a process of its own (`python -m tests.test_optimizer`).  A gate needs a side stream, and the runtime
    deals its few hardware queues to the streams of a process as they are first used: a stream taken here would move every
    later module's gate to another queue, and the one that comes to share the default stream's cannot hold its control
    back.  The child's two side streams are the first two of their process and get a queue each."""
    run = subprocess.run([sys.executable, "-m", "tests.test_optimizer"], cwd=str(ROOT), capture_output=True, text=True)
    assert run.returncode == 0 and f"gate cases ok: {len(GATE_SIZES)}" in run.stdout, (run.stdout[-3000:], run.stderr[-3000:])


def test_a_training_run_on_the_gpu_is_the_oracle_backends_run_on_every_byte():
    """The 64 x 13 in-kernel stack with `PolicyNet` and `Adam` (clipping and the KL gate on) on the GPU, nine control steps and
    two epochs, against the same stack on the oracle backend: every observation, reward and flag it hands out, every PPO
    gradient, ``stats`` and ``info``, and ``theta``, ``m``, ``v`` and ``state`` at the end."""
    want_steps, want_calls, want_end = oc.run_whole("in-kernel", "cpu")
    got_steps, got_calls, got_end = oc.run_whole("in-kernel", DEV)
    assert len(got_steps) == len(want_steps) == rc.K
    oc.assert_gate_worked(want_calls)
    for i, (got, want) in enumerate(zip(got_steps, want_steps)):
        rc.assert_equal(got, want, f"what control step {i + 1} handed out")
    for got, want in zip(got_calls, want_calls):
        rc.assert_equal({n: got[n] for n in ("grad", "stats", "info")}, {n: want[n] for n in ("grad", "stats", "info")},
                        f"PPO call after step {want['step']}")
    names = ("net.0", "opt.m", "opt.v", "opt.state", "opt.calls")
    rc.assert_equal({n: got_end[n] for n in names}, {n: want_end[n] for n in names}, "theta, m, v and state at the end")


if __name__ == "__main__":
    for size in GATE_SIZES:
        gate_case(size)
    print(f"gate cases ok: {len(GATE_SIZES)}")
