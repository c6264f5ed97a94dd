"""The actor-critic network on the MI355X (sparc_amd/csrc/wedm_policy_net.h, sparc_amd/policy_net.py, DESIGN.md section
4.22): `wedm_policy_net` against `policy_net_reference` on every byte of everything it may write -- the head's rows with
their padding columns, the values, the tile partials, the gradient, each between guard bands -- at samples of the chunk,
pass and tile edges and of the paddings of the MFMA's k-step (D % 4 in {0, 1, 3}, O % 4 in {0, 2}), through an index with
repeats and entries outside the store; hostile values; the phases apart, repeats and `ACCUMULATE`; `PolicyNet` under `PPOLoss`
without a host synchronisation or an allocation; the call on a side stream behind a gate; and a whole training run on the
GPU against the same run on the oracle backend.  The sweeps -- every pair of hidden widths, every mode count and k-padding,
every LDS placement, the remaining pass edges and the fold past eight tiles -- are in tests/test_policy_net_shapes.py."""
from __future__ import annotations

import ctypes as C
import gc

import numpy as np
import pytest
import torch

from sparc_amd import PolicyHead, PolicyNet, PPOLoss, RolloutBuffer, WireEDMVectorEnv, _abi, _lib
from sparc_amd.policy_net import ACTIVATIONS, layout, policy_net_reference
from tests import _policy_net_common as pc
from tests import _resume_common as rc
from tests._normalize_common import same_bits
from tests._snapshot_common import make
from tests._stream_gate import Gate, check_control, gated, seconds_on
from tests.test_rollout import DEV, Banded, poisoned

pytestmark = pytest.mark.gpu
ALL = _abi.NET_FORWARD | _abi.NET_BACKWARD | _abi.NET_FOLD


def device_policy_net(desc) -> None:
    _lib.call_stateless(_lib.load().wedm_policy_net, torch.device(DEV), C.byref(desc))


class Problem:
    """A `draw_call` on the device, every block between guard bands (``shift``: every base that many bytes past a 16-byte
    boundary), the outputs poisoned; `expect` builds every output block as the call has to leave it."""

    def __init__(self, call: dict, activation: str, param_pad: int = 0, shift: int = 0):
        self.call, self.activation, self.param_pad = call, activation, param_pad
        rows, M = call["rows"], call["M"]
        self.P = P = 8 + M
        self.n_theta = call["theta"].shape[0]
        self.tiles = -(-rows // 256)
        host_in = {k: call[k] for k in ("theta", "obs", "grad_params", "grad_value")}
        if call["index"] is not None:
            host_in["index"] = call["index"]
        host_out = {"params": poisoned((rows, P + param_pad), np.float32), "value": poisoned((rows,), np.float32),
                    "partials": poisoned((self.tiles, self.n_theta), np.float32), "grad_theta": poisoned((self.n_theta,), np.float32)}
        self.host_in, self.host_out = host_in, host_out
        lead = shift // 4   # (index is int64: it keeps its alignment)
        self.inputs = {k: self._place(v, 0 if k == "index" else lead) for k, v in host_in.items()}
        self.outputs = {k: self._place(v, lead) for k, v in host_out.items()}

    @staticmethod
    def _place(host: np.ndarray, lead: int):
        flat = np.concatenate([np.zeros(lead, dtype=host.dtype), host.reshape(-1)])
        b = Banded(flat)
        b.view = b.t[lead:].view(host.shape)
        return b

    def desc(self, flags: int):
        c, i, o = self.call, self.inputs, self.outputs
        return _abi.NetDesc(theta=i["theta"].view.data_ptr(), obs=i["obs"].view.data_ptr(),
                            index=i["index"].view.data_ptr() if "index" in i else None, params=o["params"].view.data_ptr(),
                            value=o["value"].view.data_ptr(), grad_params=i["grad_params"].view.data_ptr(),
                            grad_value=i["grad_value"].view.data_ptr(), partials=o["partials"].view.data_ptr(),
                            grad_theta=o["grad_theta"].view.data_ptr(), obs_stride=c["obs"].shape[1], param_stride=self.P + self.param_pad,
                            grad_stride=c["grad_params"].shape[1], n_src=c["obs"].shape[0], obs_dim=c["D"], hidden1=c["hidden"][0],
                            hidden2=c["hidden"][1], n_modes=c["M"], activation=ACTIVATIONS.index(self.activation), rows=c["rows"], flags=flags)

    def expect(self, flags: int = ALL) -> dict:
        res = self.res = pc.define(self.call, self.activation)
        want = {k: v.copy() for k, v in self.host_out.items()}
        if flags & _abi.NET_FORWARD:
            want["params"][:, : self.P] = res["params"]
            want["value"][:] = res["value"]
        if flags & _abi.NET_BACKWARD:
            want["partials"][:] = res["partials"]
        if flags & _abi.NET_FOLD:
            want["grad_theta"][:] = res["grad_theta"]
        return want

    def differences(self, want: dict):
        torch.cuda.synchronize()
        bad = [k for k, b in self.outputs.items() if not same_bits(b.view, want[k])]
        bad += [f"input {k}" for k, b in self.inputs.items() if not same_bits(b.view, self.host_in[k])]
        return bad + [f"band of {k}" for k, b in {**self.inputs, **self.outputs}.items() if not b.bands_intact()]


# rows, D, hidden, M, activation, stride padding, index: every value of every axis occurs
CASES = [
    (1, 1, (16, 16), 1, "relu", 0, None),
    (63, 3, (16, 64), 9, "tanh", 3, "perm"),
    (64, 4, (64, 64), 19, "relu", 0, "repeats"),
    (65, 13, (128, 32), 1, "tanh", 3, None),
    (255, 148, (16, 16), 9, "relu", 0, "perm"),
    (256, 16, (64, 64), 19, "tanh", 3, "repeats"),
    (257, 17, (128, 32), 9, "tanh", 0, "repeats"),
    (1000, 13, (16, 64), 1, "relu", 3, "perm"),
    (5 * 256 + 1, 16, (128, 128), 19, "tanh", 3, None),
]


@pytest.mark.parametrize("rows,D,hidden,M,activation,pad,index", CASES)
def test_forward_and_backward_are_the_definition_on_every_byte(rows, D, hidden, M, activation, pad, index):
    p = Problem(pc.draw_call(rows, D, hidden, M, index, seed=rows + D, obs_pad=pad and 2, grad_pad=pad), activation, param_pad=pad)
    want = p.expect()
    device_policy_net(p.desc(ALL))
    assert p.differences(want) == []
    assert np.isfinite(p.res["grad_theta"]).all() and np.abs(p.res["grad_theta"]).sum() > 0


@pytest.mark.parametrize("activation", ACTIVATIONS)
def test_hostile_values_at_257_rows(activation):
    """NaN and infinities in the observations, -0.0 biases over negative weights under all-zero rows (the first layer's
    pre-activation is -0.0 there, behind a D padded from 5 to 8), subnormal weights and gradients, gradients of 1e-30 whose
    products underflow to -0.0, gradients of 1e30."""
    rows, D, hidden, M = 257, 5, (16, 32), 9
    call = pc.draw_call(rows, D, hidden, M, "repeats", seed=7)
    lay = layout(D, hidden, M)
    th, obs, gp, gv = call["theta"], call["obs"], call["grad_params"], call["grad_value"]
    obs[3, 0], obs[4, 1], obs[5, 2], obs[6, :] = np.nan, np.inf, -np.inf, np.nan
    obs[10:40, :] = 0.0
    for name in ("b1", "b2", "b3"):
        at, shape = lay[name]
        th[at: at + shape[0]: 2] = -0.0
    at, shape = lay["W1"]   # negative weights into the columns with a -0.0 bias: a zero row's products there are all -0.0
    w1 = th[at: at + shape[0] * shape[1]].reshape(shape)
    w1[:, ::2] = -np.abs(w1[:, ::2]) - np.float32(0.1)
    at, shape = lay["W2"]
    th[at: at + 40] = np.float32(1e-41)
    th[at + 40: at + 80] = np.float32(-3e-39)
    gp[0:50, :] = np.float32(1e-41)
    gp[50:120, :] = np.where(np.arange(gp.shape[1]) % 2 == 0, np.float32(1e-30), np.float32(-1e-30))
    gv[50:120] = np.float32(-1e-30)
    gp[120:150, :] = np.float32(1e30)
    gv[120:150] = np.float32(-1e30)
    call["index"][3:7] = np.arange(3, 7)         # the NaN, the infinities and the zero rows are reached
    call["index"][10:40] = np.arange(10, 40)
    call["index"][50:150] = np.arange(50, 150)
    p = Problem(call, activation)
    want = p.expect()
    device_policy_net(p.desc(ALL))
    assert p.differences(want) == []
    a1 = p.res["a1"][10:40, ::2]
    assert (np.signbit(a1) & (a1 == 0)).all() and (np.abs(p.res["x"]) == np.finfo(np.float32).max).any()


def test_repeats_phases_accumulate_and_bases_off_a_16_byte_boundary():
    call = pc.draw_call(700, 13, (64, 32), 9, "perm", seed=3, obs_pad=1, grad_pad=3)
    p = Problem(call, "tanh", param_pad=3, shift=4)
    want = p.expect()
    for _ in range(2):   # the same call twice: the same bits
        device_policy_net(p.desc(ALL))
        assert p.differences(want) == []
    q = Problem(call, "tanh", param_pad=3, shift=12)   # the phases apart
    for flags in (_abi.NET_FORWARD, _abi.NET_BACKWARD, _abi.NET_FOLD):
        device_policy_net(q.desc(flags))
    assert q.differences(want) == []
    # ACCUMULATE: the fold plus one float32 addition per element
    before = np.random.default_rng(1).normal(size=q.n_theta).astype(np.float32)
    before[::5] = -0.0
    q.outputs["grad_theta"].view.copy_(torch.from_numpy(before))
    device_policy_net(q.desc(_abi.NET_FOLD | _abi.NET_ACCUMULATE))
    want["grad_theta"] = (before + p.res["grad_theta"]).astype(np.float32)
    assert q.differences(want) == []


def _stack(n=64, T=4, hidden=(64, 64)):
    vec = WireEDMVectorEnv(make(DEV, n, "autoreset", "s13"), max_episode_steps=3000)
    head = PolicyHead(vec, modes=(5, 9, 13), bounds=rc.BOUNDS, seed=111)
    ppo = PPOLoss(head, clip=0.2, vf_coef=0.5, ent_coef=0.01, clip_value=0.3)
    buf = RolloutBuffer(vec, T, gamma=0.95, extras={"log_prob": torch.float32})
    net = PolicyNet(vec, head, hidden=hidden, seed=5)
    obs, _ = vec.reset(seed=33)
    buf.reset()
    with torch.no_grad():
        for _ in range(T):
            params, value = net.forward(obs * 1e-3)
            out = head.sample(params)
            nxt, reward, term, trunc, _ = vec.step(out.action)
            buf.add(obs * 1e-3, head.stored(out), value, reward, term, trunc, log_prob=out.log_prob)
            obs = nxt.clone()
        buf.finish(net.forward(obs * 1e-3)[1])
    return vec, head, ppo, buf, net


def test_an_update_neither_synchronises_nor_allocates_and_is_the_definition():
    vec, head, ppo, buf, net = _stack()
    assert net._native is not None
    flat = buf.flat()
    parts = torch.tensor_split(torch.randperm(flat["obs"].shape[0], generator=torch.Generator().manual_seed(2)).to(DEV), 2)
    opt = torch.optim.SGD([net.theta], lr=0.1)
    for idx in parts:   # the first epoch: against the definition
        theta = net.theta.detach().cpu().numpy().copy()
        params, value = net(rollout=buf, index=idx)
        ppo.backward(params, value, rollout=buf, index=idx)
        B, P = idx.shape[0], head.param_dim
        g = ppo._grad[: B * (P + 1)].cpu().numpy()
        want = policy_net_reference(theta, flat["obs"].cpu().numpy(), hidden=net.hidden, n_modes=net.n_modes, activation="tanh",
                                    index=idx.cpu().numpy(), grad_params=g[: B * P].reshape(B, P), grad_value=g[B * P:])
        assert same_bits(params, want["params"]) and same_bits(value, want["value"]) and same_bits(net.theta.grad, want["grad_theta"])
        assert float(np.abs(want["grad_theta"]).sum()) > 0
        opt.step()
        net.theta.grad = None
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for idx in parts:
            before = torch.cuda.memory_allocated()
            params, value = net(rollout=buf, index=idx)
            ppo.backward(params, value, rollout=buf, index=idx)
            del params, value
            after = torch.cuda.memory_allocated()
            assert after == before, (before, after)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        gc.enable()
    # PPOLoss.loss(...).backward(): the same gradient, scaled by what is upstream
    net.theta.grad = None
    params, value = net(rollout=buf, index=parts[0])
    (2.0 * ppo.loss(params, value, rollout=buf, index=parts[0])).backward()
    twice = net.theta.grad.clone()
    net.theta.grad = None
    params, value = net(rollout=buf, index=parts[0])
    ppo.backward(params, value, rollout=buf, index=parts[0])
    assert float(twice.abs().sum()) > 0 and torch.allclose(twice, 2.0 * net.theta.grad, rtol=1e-4, atol=1e-7)
    vec.close()


def test_the_call_runs_on_the_current_stream_behind_a_gate():
    rows, D, hidden, M = 257, 13, (64, 64), 9
    a = pc.draw_call(rows, D, hidden, M, "repeats", seed=11)
    b = pc.draw_call(rows, D, hidden, M, "repeats", seed=12)
    b["index"] = a["index"]
    p, control = Problem(a, "tanh"), Problem(a, "tanh")
    want_a, want_b = p.expect(), Problem(b, "tanh").expect()
    b_dev = {k: torch.from_numpy(b[k]).to(DEV) for k in ("theta", "obs", "grad_params", "grad_value")}
    device_policy_net(p.desc(ALL))   # warm-up: the code is loaded
    gate = Gate(seconds_on(torch.cuda.current_stream(), lambda: device_policy_net(p.desc(ALL))))
    cdesc = control.desc(ALL)
    for name in ("theta", "obs", "index", "grad_params", "grad_value"):   # the control reads the same input buffers
        setattr(cdesc, name, getattr(p.desc(ALL), name))

    def write_b():
        for k, t in b_dev.items():
            p.inputs[k].view.copy_(t, non_blocking=True)

    gated(gate, write_b, lambda: device_policy_net(p.desc(ALL)), lambda: device_policy_net(cdesc))
    got = {k: blk.view for k, blk in control.outputs.items()}
    check_control(all(same_bits(got[k], want_a[k]) for k in got), all(same_bits(got[k], want_b[k]) for k in got), gate, "wedm_policy_net")
    assert all(same_bits(blk.view, want_b[k]) for k, blk in p.outputs.items())


def test_a_training_run_on_the_gpu_is_the_oracle_backends_run_on_every_byte():
    """The 64 x 13 in-kernel stack with the `PolicyNet` on the GPU, nine control steps and two epochs, against the same
    stack on the oracle backend: every observation, reward and flag it hands out, every PPO gradient and `stats`, and
    everything it holds at the end, ``theta`` included."""
    want_steps, want_calls, want_end = pc.run_whole("in-kernel", "cpu")
    got_steps, got_calls, got_end = pc.run_whole("in-kernel", DEV)
    assert len(got_steps) == len(want_steps) == rc.K and len(got_calls) == len(want_calls) == 4
    for i, (got, want) in enumerate(zip(got_steps, want_steps)):
        rc.assert_equal(got, want, f"what control step {i + 1} handed out")
    for got, want in zip(got_calls, want_calls):
        rc.assert_equal({n: got[n] for n in ("grad", "stats")}, {n: want[n] for n in ("grad", "stats")}, f"PPO call after step {want['step']}")
    rc.assert_equal({"theta": got_end["net.0"]}, {"theta": want_end["net.0"]}, "theta at the end")
    assert any(bool((c["grad"] != 0).any()) for c in want_calls)
