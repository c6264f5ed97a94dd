"""The policy action head on the MI355X (sparc_amd/csrc/wedm_head.h, sparc_amd/policy_head.py):
`wedm_policy_head` against `policy_head_definition` on every byte of everything it writes -- the action leaves, the mode, the
stored pre-squash values and mode index, log-probability, entropy and the gradient -- at the wave and block edges, through
LDS and directly, with its blocks in guard bands; every mode count from 1 to 19; a wide regime of parameters and stored
values (zero probabilities, a saturated tanh, infinities, NaN, subnormals); a draw evaluated again; shards against the
whole batch; hostile rows; and `PolicyHead` through `WireEDMVectorEnv` and `RolloutBuffer`, without a host synchronisation
or an allocation per step."""
from __future__ import annotations

import gc

import numpy as np
import pytest
import torch

from sparc_amd import PolicyHead, RolloutBuffer, WireEDMVectorEnv, _abi
from sparc_amd.policy_head import BACKWARD, EVALUATE, SAMPLE, device_policy_head, policy_head_definition
from tests._gae_common import is_subnormal
from tests._normalize_common import same_bits
from tests._policy_head_common import (ALL_M, CONSTS, MODES, desc_consts, make_hostile, random_params, random_stored, wide_params,
                                       wide_stored, zero_probability_rows)
from tests._snapshot_common import make
from tests.test_rollout import DEV, FILL, Banded, poisoned

pytestmark = pytest.mark.gpu
LEAF_BLOCKS = ("action0", "action1", "action2", "action3")
SAMPLED = ("u", "mode_index", "current_mode", "log_prob", "entropy") + LEAF_BLOCKS


class Problem:
    """``rows`` parameter rows of ``M`` modes on the device and the host: params ``[rows, P + pad_in]`` with NaN in the
    padding columns, stored actions, upstream gradients, and every output block as 0xA5 bytes (grad_params ``[rows, P +
    pad_out]``), each between guard bands.  `call` runs `wedm_policy_head`; `differences` names every block -- outputs, and
    inputs, which nothing may change -- that is not what ``want`` (default: what it was) says, on every byte."""

    def __init__(self, rows, M, seed, pad_in=0, pad_out=0, hostile=False, mode_index=None, wide=False):
        self.rows, self.M, self.P, self.si, self.so = rows, M, 8 + M, 8 + M + pad_in, 8 + M + pad_out
        rng = np.random.default_rng(seed)
        h = self.host = {}
        if wide:   # the wide regime's rows, and stored values that saturate the tanh, are huge, infinite, NaN or subnormal
            h["params"] = wide_params(rng, rows, M, pad_in)
            h["u"], h["mode_index"] = wide_stored(rng, h["params"], M)
        else:
            h["params"] = random_params(rng, rows, M, pad_in)
            if hostile:
                h["params"] = make_hostile(rng, h["params"], M)
            h["u"], h["mode_index"] = random_stored(rng, np.nan_to_num(h["params"], posinf=1.0, neginf=-1.0).clip(-3, 3), M)
        if mode_index is not None:
            h["mode_index"] = np.resize(np.asarray(mode_index, dtype=np.int32), rows)
        h["g_log_prob"], h["g_entropy"] = rng.normal(size=rows).astype(np.float32), rng.normal(size=rows).astype(np.float32)
        for name in LEAF_BLOCKS:
            h[name] = poisoned((rows,), np.float64)
        h["current_mode"] = poisoned((rows,), np.int32)
        h["log_prob"], h["entropy"] = poisoned((rows,), np.float32), poisoned((rows,), np.float32)
        h["grad_params"] = poisoned((rows, self.so), np.float32)
        self.blocks = {name: Banded(a) for name, a in h.items()}

    def poison(self, *names):
        for name in names:
            self.host[name].view(np.uint8)[...] = FILL
            self.blocks[name].t.copy_(torch.from_numpy(self.host[name]))

    def put(self, name, a):
        """Other contents for an input block, on the host and the device."""
        self.host[name] = np.ascontiguousarray(a, dtype=self.host[name].dtype)
        self.blocks[name].t.copy_(torch.from_numpy(self.host[name]))

    def desc(self, op, lo=0, count=None, g_entropy=True, **kw):
        """The descriptor of rows [lo, lo + count): a shard is the same blocks entered ``lo`` rows further on."""
        b = self.blocks
        at = lambda name, per_row: b[name].t.data_ptr() + lo * per_row   # noqa: E731
        d = desc_consts(_abi.HeadDesc(
            params=at("params", 4 * self.si), u=at("u", 16), mode_index=at("mode_index", 4), current_mode=at("current_mode", 4),
            log_prob=at("log_prob", 4), entropy=at("entropy", 4), g_log_prob=at("g_log_prob", 4),
            g_entropy=at("g_entropy", 4) if g_entropy else None, grad_params=at("grad_params", 4 * self.so),
            param_stride=self.si, grad_stride=self.so, rows=self.rows - lo if count is None else count, op=op, **kw), self.M)
        d.action[:] = [at(name, 8) for name in LEAF_BLOCKS]
        return d

    def call(self, op, **kw):
        device_policy_head(self.desc(op, **kw), DEV)

    def definition(self, op, **kw):
        h = self.host
        return policy_head_definition(op, h["params"], modes=MODES[self.M], u=h["u"], mode_index=h["mode_index"],
                                      g_log_prob=h["g_log_prob"], **CONSTS, **kw)

    def expect(self, out):
        """The host's blocks with the definition's outputs ``out`` in their places (the gradient's padding stays 0xA5)."""
        want = {}
        for name, a in out.items():
            if name == "action":
                want.update({leaf: a[:, i].copy() for i, leaf in enumerate(LEAF_BLOCKS)})
            elif name == "grad_params":
                want[name] = poisoned((self.rows, self.so), np.float32)
                want[name][:, : self.P] = a
            elif name in self.host:
                want[name] = a
        return want

    def differences(self, want=None):
        torch.cuda.synchronize()
        ref = {**self.host, **(want or {})}
        bad = [name for name, b in self.blocks.items() if not same_bits(b.t, ref[name])]
        return bad + [f"band of {name}" for name, b in self.blocks.items() if not b.bands_intact()]

    def adopt(self, want):
        """The host's copies follow the device's: a later call's inputs are what this one wrote."""
        self.host.update(want)


# ------------------------------------------------------------------------------------------------ 6. the three ops
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_the_call_equals_the_definition_on_every_byte(rows):
    """The wave (64) and block (256) edges by M in {1, 2, 9} (P = 9, 10, 17: odd and even LDS rows) by the staged and the
    direct path of params (stride P and P + 3) and, for BACKWARD, of grad_params; SAMPLE drawn and DETERMINISTIC, EVALUATE,
    BACKWARD with g_entropy given and NULL.  The blocks lie in guard bands, outputs start as 0xA5 bytes, the padding columns
    hold NaN (params) and must come out as they were (grad_params), and no input may change."""
    drawn_modes = set()
    for M in (1, 2, 9):
        for pad_in in (0, 3):
            p = Problem(rows, M, seed=1000 * rows + 10 * M + pad_in, pad_in=pad_in)
            want = p.expect(p.definition(EVALUATE))
            p.call(EVALUATE)
            assert p.differences(want) == [], ("EVALUATE", rows, M, pad_in)
            for deterministic in (True, False):
                p.poison(*SAMPLED)
                kw = dict(seed=0x123456789ABCDEF, t=2 ** 32 + 5, env_id_offset=2 ** 32 - 7)
                want = p.expect(p.definition(SAMPLE, deterministic=deterministic, **kw))
                p.call(SAMPLE, flags=_abi.HEAD_DETERMINISTIC if deterministic else 0, **kw)
                assert p.differences(want) == [], ("SAMPLE", rows, M, pad_in, deterministic)
                p.adopt(want)
            drawn_modes |= set(p.host["mode_index"].tolist())
            for pad_out in (0, 3):
                q = Problem(rows, M, seed=2000 * rows + 10 * M + pad_in, pad_in=pad_in, pad_out=pad_out)
                for g_entropy in (True, False):
                    q.poison("grad_params")
                    want = q.expect(q.definition(BACKWARD, g_entropy=q.host["g_entropy"] if g_entropy else None))
                    q.call(BACKWARD, g_entropy=g_entropy)
                    assert q.differences(want) == [], ("BACKWARD", rows, M, pad_in, pad_out, g_entropy)
    assert rows == 1 or len(drawn_modes) > 1, "more than one mode index is drawn"


def test_params_and_grad_params_off_16_bytes_take_the_direct_path():
    """Stride P with the blocks entered one row further on (P = 9 floats: 36 bytes), so neither base is 16-byte aligned."""
    p = Problem(301, 1, seed=7)
    sub = {k: v[1:] for k, v in p.host.items()}
    kw = dict(modes=MODES[1], u=sub["u"], mode_index=sub["mode_index"], **CONSTS)
    want = {}
    for name, a in policy_head_definition(EVALUATE, sub["params"], **kw).items():
        if name in p.host:
            want[name] = np.concatenate([p.host[name][:1], a])
    grad = policy_head_definition(BACKWARD, sub["params"], g_log_prob=sub["g_log_prob"], g_entropy=sub["g_entropy"], **kw)["grad_params"]
    want["grad_params"] = np.concatenate([p.host["grad_params"][:1], grad])
    assert p.blocks["params"].t[1:].data_ptr() % 16 != 0
    p.call(EVALUATE, lo=1)
    p.call(BACKWARD, lo=1)
    assert p.differences(want) == []


# ------------------------------------------------------------------------------------------------ 6b. every mode count
SAMPLE_KW = dict(seed=0x123456789ABCDEF, t=2 ** 32 + 5, env_id_offset=2 ** 32 - 7)


@pytest.mark.parametrize("M", ALL_M)
def test_every_mode_count_equals_the_definition_on_every_byte(M):
    """Every M the header promises (P = 9..27: odd and even LDS rows, and P divisible by 4 at M = 4, 8, 12, 16, where a
    float4 never straddles a row) by a lone row, a partial tail block and a full block followed by a one-row block (rows 1,
    255, 257) by param_stride P (staged), P + 1 and P + 3 (direct) and, for BACKWARD, the same three grad_strides: EVALUATE,
    SAMPLE drawn and DETERMINISTIC, BACKWARD with g_entropy given and NULL, bands, 0xA5 outputs and NaN padding as in the
    test above.  The mode lists are `MODES[M]`, in which no entry is its index or its index + 1.  Over the sweep every
    index in [0, M) is drawn and every listed mode is handed out: at M = 19 that is entries 9..18 of the kept array, of
    the select chain and of ``modes[19]``."""
    drawn, handed_out = set(), set()
    for rows in (1, 255, 257):
        for pad_in in (0, 1, 3):
            p = Problem(rows, M, seed=5000 * rows + 10 * M + pad_in, pad_in=pad_in)
            want = p.expect(p.definition(EVALUATE))
            p.call(EVALUATE)
            assert p.differences(want) == [], ("EVALUATE", rows, M, pad_in)
            for deterministic in (True, False):
                p.poison(*SAMPLED)
                want = p.expect(p.definition(SAMPLE, deterministic=deterministic, **SAMPLE_KW))
                p.call(SAMPLE, flags=_abi.HEAD_DETERMINISTIC if deterministic else 0, **SAMPLE_KW)
                assert p.differences(want) == [], ("SAMPLE", rows, M, pad_in, deterministic)
                p.adopt(want)
            drawn |= set(want["mode_index"].tolist())
            handed_out |= set(want["current_mode"].tolist())
            for pad_out in (0, 1, 3):
                q = Problem(rows, M, seed=6000 * rows + 10 * M + pad_in, pad_in=pad_in, pad_out=pad_out)
                for g_entropy in (True, False):
                    q.poison("grad_params")
                    want = q.expect(q.definition(BACKWARD, g_entropy=q.host["g_entropy"] if g_entropy else None))
                    q.call(BACKWARD, g_entropy=g_entropy)
                    assert q.differences(want) == [], ("BACKWARD", rows, M, pad_in, pad_out, g_entropy)
    assert drawn == set(range(M)), "every mode index is drawn"
    assert handed_out == set(MODES[M]), "every listed mode is handed out"


@pytest.mark.parametrize("M", ALL_M)
def test_deterministic_takes_the_last_logit_when_it_is_the_largest_and_the_first_of_a_tie(M):
    """257 rows, staged and direct: the largest logit planted at index M - 1 in the even rows, and in the odd rows an exact
    tie between index 0 and index M - 1, where the first wins."""
    for pad_in in (0, 3):
        p = Problem(257, M, seed=7000 + 10 * M + pad_in, pad_in=pad_in)
        params = p.host["params"].copy()
        params[:, 8 + M - 1] = 6.0   # (the others lie in [-5, 5])
        params[1::2, 8] = 6.0
        p.put("params", params)
        p.poison(*SAMPLED)
        want = p.expect(p.definition(SAMPLE, deterministic=True))
        k = np.where(np.arange(257) % 2 == 1, 0, M - 1).astype(np.int32)
        assert np.array_equal(want["mode_index"], k) and np.array_equal(want["current_mode"], np.asarray(MODES[M], dtype=np.int32)[k])
        p.call(SAMPLE, flags=_abi.HEAD_DETERMINISTIC)
        assert p.differences(want) == [], (M, pad_in)


# ------------------------------------------------------------------------------------------------ 6c. the wide regime
@pytest.mark.parametrize("M", [3, 8, 19])
def test_the_wide_regime_equals_the_definition_on_every_byte(M):
    """257 rows of `wide_params` (log_std in [-6, 2]; logit spreads of up to 1588, so that w_j = exp(l_j - m) is exactly 0
    and p_j (log p_j + H) is 0 times a large finite number) with a stored ``u`` of `wide_stored`: draws at the parameters,
    +-20 and +-400 (e underflows, the action clamps to a bound), +-1e30, +-inf, NaN and float32 subnormals.  Every output
    equals the definition's on every byte (a NaN is 0x7FC00000 in both); what SAMPLE emits stays a listed mode with leaves
    within bounds."""
    rows = 257
    for pad in (0, 3):
        p = Problem(rows, M, seed=8000 + 10 * M + pad, pad_in=pad, pad_out=pad, wide=True)
        zero_p = zero_probability_rows(p.host["params"], M)
        assert zero_p.sum() >= 5 and np.isnan(p.host["u"]).any() and np.isinf(p.host["u"]).any() and is_subnormal(p.host["u"]).any()
        want = p.expect(p.definition(EVALUATE))
        want.update(p.expect(p.definition(BACKWARD, g_entropy=p.host["g_entropy"])))
        p.call(EVALUATE)
        p.call(BACKWARD)
        assert p.differences(want) == [], (M, pad)
        lp, grad = want["log_prob"], want["grad_params"][:, : p.P]
        assert np.isnan(lp).any() and np.isfinite(lp).any() and np.isfinite(lp[zero_p]).any()
        assert np.isnan(grad).any() and np.isfinite(grad[zero_p]).all(1).any() and np.isfinite(want["entropy"]).all()
        p.adopt(want)
        for deterministic in (False, True):
            p.poison(*SAMPLED)
            want = p.expect(p.definition(SAMPLE, seed=92, t=1, deterministic=deterministic))
            p.call(SAMPLE, seed=92, t=1, flags=_abi.HEAD_DETERMINISTIC if deterministic else 0)
            assert p.differences(want) == [], (M, pad, deterministic)
            torch.cuda.synchronize()
            k, mode = p.blocks["mode_index"].t.cpu().numpy(), p.blocks["current_mode"].t.cpu().numpy()
            assert k.min() >= 0 and k.max() < M and np.array_equal(mode, np.asarray(MODES[M], dtype=np.int32)[k])
            for i, name in enumerate(LEAF_BLOCKS):
                leaf = p.blocks[name].t.cpu().numpy()
                assert np.all(leaf >= CONSTS["lo"][i]) and np.all(leaf <= CONSTS["hi"][i]), name
            assert np.isfinite(want["log_prob"]).all()
            p.adopt(want)


# ------------------------------------------------------------------------------------------------ 7. a draw, evaluated again
@pytest.mark.parametrize("pad_in", [0, 3])
def test_sample_then_evaluate_gives_the_same_bits(pad_in):
    p = Problem(1000, 9, seed=70 + pad_in, pad_in=pad_in)
    p.call(SAMPLE, seed=71, t=3)
    torch.cuda.synchronize()
    drawn = {name: p.blocks[name].t.clone() for name in ("log_prob", "entropy", "u", "mode_index")}
    p.blocks["log_prob"].t.fill_(0.0)
    p.blocks["entropy"].t.fill_(0.0)
    p.call(EVALUATE)
    torch.cuda.synchronize()
    assert all(same_bits(p.blocks[name].t, drawn[name]) for name in drawn)
    assert bool(drawn["log_prob"].isfinite().all()) and float(drawn["log_prob"].std()) > 0


# ------------------------------------------------------------------------------------------------ 8. shards
def test_shards_in_turn_equal_the_whole_batch_and_the_definition():
    kw = dict(seed=81, t=9, env_id_offset=5000)
    whole, parts = Problem(300, 9, seed=80), Problem(300, 9, seed=80)
    want = whole.expect(whole.definition(SAMPLE, **kw))
    whole.poison(*SAMPLED)
    parts.poison(*SAMPLED)
    whole.call(SAMPLE, **kw)
    assert whole.differences(want) == []
    parts.call(SAMPLE, lo=0, count=128, **kw)
    parts.call(SAMPLE, lo=128, count=172, **{**kw, "env_id_offset": 5128})
    assert parts.differences(want) == []
    assert all(same_bits(parts.blocks[k].raw, whole.blocks[k].raw) for k in whole.blocks)


# ------------------------------------------------------------------------------------------------ 9. hostile rows
@pytest.mark.parametrize("pad_in", [0, 3])
def test_hostile_rows_reach_numbers_only(pad_in):
    """NaN, +-inf and +-1e30 scattered into the means, log-stds and logits, and stored mode indices outside [0, M): the bands
    are intact, what SAMPLE emits is a mode index in [0, M), a listed mode and leaves within their bounds, and every output
    equals the definition's on every byte (a NaN is stored as 0x7FC00000 by both).  Nothing here provokes a fault: it pins
    that data never forms an address."""
    M, rows = 9, 600
    outside = [-1, M, M + 1, -7, 2 ** 31 - 1, -2 ** 31, 1 << 20, 3]
    p = Problem(rows, M, seed=90 + pad_in, pad_in=pad_in, pad_out=pad_in, hostile=True, mode_index=outside)
    assert np.isnan(p.host["params"][:, : p.P]).any() and np.isinf(p.host["params"][:, : p.P]).any()
    want = p.expect(p.definition(EVALUATE))
    want.update(p.expect(p.definition(BACKWARD, g_entropy=p.host["g_entropy"])))
    p.call(EVALUATE)
    p.call(BACKWARD)
    assert p.differences(want) == []
    assert np.isnan(want["log_prob"]).any() and np.isfinite(want["log_prob"]).any() and np.isnan(want["grad_params"][:, : p.P]).any()
    p.adopt(want)
    for deterministic in (False, True):
        p.poison(*SAMPLED)
        want = p.expect(p.definition(SAMPLE, seed=91, t=1, deterministic=deterministic))
        p.call(SAMPLE, seed=91, t=1, flags=_abi.HEAD_DETERMINISTIC if deterministic else 0)
        assert p.differences(want) == [], deterministic
        torch.cuda.synchronize()
        k, mode = p.blocks["mode_index"].t.cpu().numpy(), p.blocks["current_mode"].t.cpu().numpy()
        assert k.min() >= 0 and k.max() < M and set(mode.tolist()) <= set(MODES[M])
        for i, name in enumerate(LEAF_BLOCKS):
            leaf = p.blocks[name].t.cpu().numpy()
            assert np.all(leaf >= CONSTS["lo"][i]) and np.all(leaf <= CONSTS["hi"][i]), name
        p.adopt(want)


# ------------------------------------------------------------------------------------------------ 10. through the stack
def test_policy_head_through_the_vector_env_and_the_rollout_buffer():
    """64 environments x 13 segments with in-kernel autoreset, four control steps driven by sampled actions: the stored
    actions and log-probabilities come back from `flat`, a PPO-shaped loss through `evaluate` puts the definition's BACKWARD
    (fed the upstream gradients read back from torch) into the leaf, and from the second `sample` on nothing synchronises
    with the host or allocates."""
    n, T = 64, 4
    vec = WireEDMVectorEnv(make(DEV, n, "autoreset", "s13"), max_episode_steps=3000)
    modes = (5, 9, 13)
    head = PolicyHead(vec, modes=modes, bounds={"servo": (-0.2, 0.4), "ON_time": (1.0, 4.0), "OFF_time": (20.0, 60.0)}, seed=101)
    assert head._native is not None
    buf = RolloutBuffer(vec, T, extras={"log_prob": torch.float32})
    gen = torch.Generator(device=DEV).manual_seed(4)
    params = torch.randn(T, n, head.param_dim, generator=gen, device=DEV)
    values = torch.randn(T + 1, n, generator=gen, device=DEV)
    obs, _ = vec.reset(seed=31)
    vec.env.state.workpiece_position = torch.linspace(10.4, 25.0, n, dtype=torch.float64, device=DEV)
    vec.env.state.wire_position = 10.0
    kept = []

    def step(t):
        nonlocal obs
        out = head.sample(params[t])
        kept.append(out)
        nxt, reward, term, trunc, _ = vec.step(out.action)
        buf.add(obs, head.stored(out), values[t], reward, term, trunc, log_prob=out.log_prob)
        obs = nxt

    step(0)
    torch.cuda.synchronize()
    gc.collect()   # `memory_allocated` counts the whole process: earlier tests' environments are collected first
    gc.disable()
    torch.cuda.set_sync_debug_mode("error")
    try:
        before = torch.cuda.memory_allocated()
        for t in range(1, T):
            step(t)
        after = torch.cuda.memory_allocated()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        gc.enable()
    assert after == before, (before, after)
    assert all(out is kept[0] for out in kept) and head.t == T
    buf.finish(values[T])
    vec.env.check_errors()
    flat = buf.flat()
    flat_params = params.reshape(T * n, head.param_dim)
    kw = dict(modes=modes, lo=head._lo, hi=head._hi, log_span=head._log_span)
    for t in range(T):   # the stored rows are the definition's draw at step t
        want = policy_head_definition(SAMPLE, params[t], seed=101, t=t, **kw)
        rows = slice(t * n, (t + 1) * n)
        assert same_bits(flat["action.u"][rows], want["u"]) and same_bits(flat["action.mode_index"][rows], want["mode_index"])
        assert same_bits(flat["log_prob"][rows], want["log_prob"])
    leaf = flat_params.clone().requires_grad_(True)
    lp, ent = head.evaluate(leaf, flat["action.u"], flat["action.mode_index"])
    assert same_bits(lp, flat["log_prob"])
    lp.retain_grad()
    ent.retain_grad()
    loss = -(torch.exp(lp - flat["log_prob"]) * flat["advantage_norm"] * flat["valid"]).mean() - 0.01 * ent.mean()
    loss.backward()
    want = policy_head_definition(BACKWARD, flat_params, u=flat["action.u"], mode_index=flat["action.mode_index"],
                                  g_log_prob=lp.grad, g_entropy=ent.grad, **kw)
    assert same_bits(leaf.grad, want["grad_params"])
    assert float(leaf.grad.abs().sum()) > 0 and bool(leaf.grad.isfinite().all())
    strided = torch.zeros(T * n, head.param_dim + 5, device=DEV)[:, 2: 2 + head.param_dim].copy_(flat_params)
    assert not strided.is_contiguous() and same_bits(head.evaluate(strided, flat["action.u"], flat["action.mode_index"])[0], lp)
