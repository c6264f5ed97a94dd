"""The policy action head (sparc_amd/policy_head.py) on the host side: the ABI mirror of
``wedm_head_desc`` and the export with its refusals (no device is needed), the NumPy portable math and polar normal against
the CPU oracle's, `policy_head_definition` against ``torch.distributions`` in float64 with ``torch.autograd``'s gradients,
what a draw claims (moments, mode frequencies, independence, shard and replay invariance), and `PolicyHead` through
`WireEDMVectorEnv` and `RolloutBuffer` on the CPU oracle backend (which has no ``policy_head`` and so runs the definition)."""
from __future__ import annotations

import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from sparc_amd import PolicyHead, RolloutBuffer, WireEDMVectorEnv, _abi, _lib
from sparc_amd.core.tables import VALID_CRATER_MODES
from sparc_amd.policy_head import (BACKWARD, EVALUATE, HALF_LOG_2PI, HALF_LOG_2PIE, LN2, SAMPLE, polar_normal,
                                   policy_head_definition, portable_exp, portable_log)
from tests._normalize_common import same_bits
from tests._policy_head_common import (ALL_M, CONSTS, HI, LO, LOG_SPAN, MODES, desc_consts, random_params, random_stored, wide_params,
                                        zero_probability_rows)
from tests._snapshot_common import make

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------ 1. the C-ABI
def test_desc_struct_mirror_matches_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wedm_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(wedm_head_desc));']
    for field, _ in _abi.HeadDesc._fields_:
        lines.append(f'  printf("{field} %zu\\n", offsetof(wedm_head_desc, {field}));')
    lines += ['  printf("consts %d %u abi %d\\n", WEDM_HEAD_MAX_MODES, WEDM_HEAD_STREAM0, WEDM_ABI_VERSION);',
              '  printf("enums %d %d %d %d\\n", WEDM_HEAD_SAMPLE, WEDM_HEAD_EVALUATE, WEDM_HEAD_BACKWARD, WEDM_HEAD_DETERMINISTIC);',
              "  return 0;", "}"]
    src = tmp_path / "desc.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "desc"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                   check=True)
    out = dict(row.split(" ", 1) for row in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("size")) == C.sizeof(_abi.HeadDesc)
    assert out.pop("consts") == f"{_abi.HEAD_MAX_MODES} {_abi.HEAD_STREAM0} abi 4" == f"19 {0xC0000000} abi 4"
    assert out.pop("enums") == f"{_abi.HEAD_SAMPLE} {_abi.HEAD_EVALUATE} {_abi.HEAD_BACKWARD} {_abi.HEAD_DETERMINISTIC}" == "0 1 2 1"
    assert (SAMPLE, EVALUATE, BACKWARD) == (0, 1, 2)
    assert {k: int(v) for k, v in out.items()} == {f: getattr(_abi.HeadDesc, f).offset for f, _ in _abi.HeadDesc._fields_}


def test_the_call_is_exported_and_the_abi_version_stays():
    assert "wedm_policy_head" in _lib.EXPORTS
    L = _lib.load()
    assert L.wedm_policy_head is not None and L.wedm_abi_version() == _abi.ABI_VERSION == 4


def test_the_header_s_constants_are_python_s():
    assert (LN2, HALF_LOG_2PI, HALF_LOG_2PIE) == (math.log(2.0), 0.5 * math.log(2.0 * math.pi), 0.5 * math.log(2.0 * math.pi) + 0.5)
    text = (ROOT / "include" / "wedm_hip.h").read_text()
    assert all(repr(c) in text for c in (LN2, HALF_LOG_2PI, HALF_LOG_2PIE))
    kernels = (ROOT / "sparc_amd" / "csrc" / "wedm_head.h").read_text()
    assert all(repr(c) in kernels for c in (LN2, HALF_LOG_2PI, HALF_LOG_2PIE))


def test_bad_arguments_are_refused_before_anything_is_launched():
    """Every pointer below is an address nobody owns: a call that launched would fault (and on a machine without a device
    fail with WEDM_ERR_HIP); every case returns WEDM_ERR_BAD_ARG with a text."""
    L = _lib.load()
    A = 0x100000   # blocks 0x10000 apart: 100 rows of stride 20 are 8 000 bytes of float32

    def desc(op, **kw):
        f = dict(params=A, u=A + 0x10000, mode_index=A + 0x20000, current_mode=A + 0x30000, log_prob=A + 0x40000,
                 entropy=A + 0x50000, g_log_prob=A + 0x60000, g_entropy=A + 0x70000, grad_params=A + 0x80000,
                 param_stride=20, grad_stride=20, rows=100, op=op)
        arrays = {name: kw.pop(name) for name in ("action", "lo", "hi", "log_span") if name in kw}
        arrays.setdefault("action", [A + 0x90000, A + 0xA0000, A + 0xB0000, A + 0xC0000])
        n_modes = kw.pop("n_modes", 9)
        f.update(kw)
        d = desc_consts(_abi.HeadDesc(**f), 9)
        d.n_modes = n_modes
        for name, values in arrays.items():
            getattr(d, name)[:] = values
        return d

    def refused(d, what):
        assert L.wedm_policy_head(C.byref(d), None) == _abi.ERR_BAD_ARG, what
        assert b"wedm_policy_head" in L.wedm_last_error(None), what

    assert L.wedm_policy_head(None, None) == _abi.ERR_BAD_ARG and L.wedm_last_error(None).startswith(b"wedm_policy_head:")
    # NULLs that the op needs
    needs = {SAMPLE: ("params", "u", "mode_index", "current_mode", "log_prob", "entropy"),
             EVALUATE: ("params", "u", "mode_index", "log_prob", "entropy"),
             BACKWARD: ("params", "u", "mode_index", "g_log_prob", "grad_params")}
    for op, names in needs.items():
        for name in names:
            refused(desc(op, **{name: None}), (op, name))
    for i in range(4):
        action = [A + 0x90000, A + 0xA0000, A + 0xB0000, A + 0xC0000]
        action[i] = None
        refused(desc(SAMPLE, action=action), ("action", i))
    # misaligned pointers: every float32 / int32 block to 4, the float64 leaves to 8, u to 16
    for name in ("params", "mode_index", "log_prob", "entropy"):
        refused(desc(EVALUATE, **{name: A + 0xD0000 + 2}), ("misaligned", name))
    for name in ("g_log_prob", "g_entropy", "grad_params"):
        refused(desc(BACKWARD, **{name: A + 0xD0000 + 2}), ("misaligned", name))
    refused(desc(SAMPLE, current_mode=A + 0x30000 + 1), "misaligned current_mode")
    refused(desc(SAMPLE, action=[A + 0x90000 + 4, A + 0xA0000, A + 0xB0000, A + 0xC0000]), "misaligned leaf")
    for op in (SAMPLE, EVALUATE, BACKWARD):
        refused(desc(op, u=A + 0x10000 + 8), ("u to 16 bytes", op))
    # rows, modes, strides
    refused(desc(EVALUATE, rows=0), "rows 0")
    refused(desc(EVALUATE, rows=-5), "rows negative")
    refused(desc(EVALUATE, n_modes=0), "no modes")
    refused(desc(EVALUATE, n_modes=_abi.HEAD_MAX_MODES + 1), "too many modes")
    refused(desc(EVALUATE, param_stride=16), "param_stride below P")
    refused(desc(BACKWARD, grad_stride=16), "grad_stride below P")
    # bounds
    for x in (math.nan, math.inf, -math.inf):
        for name in ("lo", "hi", "log_span"):
            v = list(dict(lo=LO, hi=HI, log_span=LOG_SPAN)[name])
            v[2] = x
            refused(desc(EVALUATE, **{name: v}), (name, x))
    refused(desc(EVALUATE, hi=[1.0, 200.0, 0.0, 100.0]), "hi == lo")
    refused(desc(EVALUATE, hi=[-2.0, 200.0, 5.0, 100.0]), "hi < lo")
    # op and flags
    refused(desc(3), "undefined op")
    refused(desc(-1), "undefined op")
    refused(desc(SAMPLE, flags=2), "undefined flag")
    refused(desc(SAMPLE, flags=-1), "undefined flags")
    refused(desc(EVALUATE, flags=_abi.HEAD_DETERMINISTIC), "a flag with EVALUATE")
    refused(desc(BACKWARD, flags=_abi.HEAD_DETERMINISTIC), "a flag with BACKWARD")
    # an output block on an input block: the same address, its last element, the byte before its first
    last = (99 * 20 + 17) * 4
    refused(desc(EVALUATE, log_prob=A), "log_prob on params")
    refused(desc(EVALUATE, entropy=A + last - 4), "entropy on params' last element")
    refused(desc(EVALUATE, log_prob=A + 0x10000 + 1596), "log_prob on u's last element")
    refused(desc(EVALUATE, entropy=A + 0x20000 - 396), "entropy's last element on mode_index")
    refused(desc(BACKWARD, grad_params=A), "grad_params on params")
    refused(desc(BACKWARD, grad_params=A + 0x60000 - last + 4), "grad_params' last element on g_log_prob")
    refused(desc(BACKWARD, grad_params=A + 0x70000 + 396), "grad_params on g_entropy's last element")
    refused(desc(BACKWARD, grad_params=A + 0x10000), "grad_params on u")
    refused(desc(SAMPLE, u=A), "u on params")
    refused(desc(SAMPLE, mode_index=A + 8), "mode_index inside params")
    refused(desc(SAMPLE, current_mode=A + last - 4), "current_mode on params' last element")
    refused(desc(SAMPLE, action=[A + 0x90000, A, A + 0xB0000, A + 0xC0000]), "a leaf on params")


# ------------------------------------------------------------------------------------------------ 2. portable math, normals
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_numpy_portable_exp_and_log_equal_the_oracle_s(orc):
    L = orc.lib()
    rng = np.random.default_rng(0)   # the ranges of test_oracle_math.py, and the edges of the branches
    xs = np.concatenate([rng.uniform(-700, 700, 20000), rng.uniform(-1, 1, 20000),
                         [0.0, -0.0, 1e-10, 24.0, -500.0, 709.0, 709.5, -708.0, -708.5, 0.34657359027997264, 0.3465735902799727,
                          -0.3465735902799727, 3.725290298461914e-09, -3.7e-09, np.inf, -np.inf]])
    want = np.array([L.wedm_oracle_exp(float(x), orc.MATH_PORTABLE) for x in xs])
    assert np.array_equal(bits(portable_exp(xs)), bits(want))
    assert np.isnan(portable_exp(np.array([np.nan])))[0]
    xs = np.concatenate([rng.uniform(0, 1, 20000)[1:], 2.0 ** rng.uniform(-104, 0, 20000), rng.uniform(1, 20, 20000),
                         [1.0, 2.0, 19.0, 0.5, math.sqrt(2.0), 1.0 / math.sqrt(2.0)]])
    want = np.array([L.wedm_oracle_log(float(x), orc.MATH_PORTABLE) for x in xs])
    assert np.array_equal(bits(portable_log(xs)), bits(want))


def test_numpy_polar_normal_at_stream_base_1_equals_the_oracle_s(orc):
    env, time = np.meshgrid(np.arange(60), np.arange(50), indexing="ij")
    got = polar_normal((1234, 0), time, 0, env, 1)
    want = np.array([[orc.std_normal(1234, int(e), 0, int(t))[0] for t in range(50)] for e in range(60)])
    assert np.array_equal(bits(got), bits(want))
    attempts = np.array([[orc.std_normal(1234, int(e), 0, int(t))[1] for t in range(50)] for e in range(60)])
    assert attempts.max() > 1, "a rejected attempt is among them"
    hi = polar_normal((7, 9), 5, 2, np.arange(100), 1)   # a key and an episode with high words
    assert np.array_equal(bits(hi), bits([orc.std_normal(7 | (9 << 32), e, 2, 5)[0] for e in range(100)]))


# ------------------------------------------------------------------------------------------------ 3. an independent definition
def torch_distributions(params, u, k, g_lp, g_ent, M):
    """log_prob, entropy and the gradient of ``sum(g_lp * log_prob + g_ent * entropy)`` from torch.distributions in float64:
    Normal -> TanhTransform -> AffineTransform, and Categorical.  The transforms cache their last (x, y), so the density at
    ``y = transform(u)`` is evaluated at ``u`` itself and not at an ``atanh`` of a rounded ``tanh``."""
    from torch.distributions import Categorical, Normal, TransformedDistribution
    from torch.distributions.transforms import AffineTransform, TanhTransform

    p = torch.from_numpy(params[:, : 8 + M].astype(np.float64)).requires_grad_(True)
    lo, hi = torch.tensor(LO, dtype=torch.float64), torch.tensor(HI, dtype=torch.float64)
    base = Normal(p[:, 0:4], p[:, 4:8].exp())
    tanh, affine = TanhTransform(cache_size=1), AffineTransform((lo + hi) / 2, (hi - lo) / 2, cache_size=1)
    y = affine(tanh(torch.from_numpy(u.astype(np.float64))))
    cat = Categorical(logits=p[:, 8:])
    lp = TransformedDistribution(base, [tanh, affine]).log_prob(y).sum(1) + cat.log_prob(torch.from_numpy(k.astype(np.int64)))
    ent = base.entropy().sum(1) + cat.entropy()
    (torch.from_numpy(g_lp.astype(np.float64)) * lp + torch.from_numpy(g_ent.astype(np.float64)) * ent).sum().backward()
    return lp.detach().numpy(), ent.detach().numpy(), p.grad.numpy(), y.detach().numpy()


# the largest discrepancies seen on the inputs below, relative to 1 + the sum of the absolute summands; the
# bounds are 8 x these.  log_prob's is the reference's own: TanhTransform's log-Jacobian takes softplus(-2u), which torch
# replaces by its argument above 20 -- at u = -10.17 that drops log1p(exp(-20.34)) = 1.5e-9, twice, from a log_prob of -5.4.
# (Seen at M = 1, 2, 9.  Over every M in 1..19 the largest are log_prob 6.76e-11 at M = 18, entropy 1.99e-16 at M = 14 and
# the gradient 1.18e-15 at M = 3: all within the 8 x of the figures below, which stay as they were.)
SEEN = dict(log_prob=4.36e-11, entropy=1.95e-16, grad=7.25e-16)


# the same on the wide regime's inputs (`wide_params`: log_std in [-6, 2], logit spreads of up to 1588, many p_j exactly 0), by
# the same scales -- which do not carry the logits' magnitude: a logit of 800 rounds l_j - m by 1e-13 absolute before anything
# is compared, so the friendly bounds do not hold there -- largest over M in WIDE_M (log_prob at M = 16, again torch's softplus
# cut-off; entropy at M = 8; the gradient at M = 19); the bounds are 8 x these
WIDE_SEEN = dict(log_prob=6.43e-11, entropy=4.87e-15, grad=6.81e-14)
WIDE_M = (2, 3, 4, 8, 12, 16, 19)


def against_torch_distributions(M, params, u, k, g_lp, g_ent):
    """The largest discrepancy of log_prob, entropy and the gradient between the definition and ``torch.distributions``,
    relative to 1 + the absolute summands of each quantity from plain NumPy; and the exact claims beside them."""
    rows = params.shape[0]
    kw = dict(modes=MODES[M], u=u, mode_index=k, **CONSTS)
    ev = policy_head_definition(EVALUATE, params, **kw)
    bw = policy_head_definition(BACKWARD, params, g_log_prob=g_lp, g_entropy=g_ent, **kw)
    lp, ent, grad, y = torch_distributions(params, u, k, g_lp, g_ent, M)
    # the scales: 1 + the absolute summands of each quantity, from plain NumPy
    mu, ls, l = (params[:, a:b].astype(np.float64) for a, b in ((0, 4), (4, 8), (8, 8 + M)))
    ud = u.astype(np.float64)
    z, a = (ud - mu) / np.exp(ls), np.abs(ud)
    m = l.max(1, keepdims=True)
    logW = np.log(np.exp(l - m).sum(1, keepdims=True))
    logp = l - m - logW
    p = np.exp(logp)
    H = -(p * logp).sum(1, keepdims=True)
    scale_lp = 1 + (0.5 * z * z + np.abs(ls) + HALF_LOG_2PI + np.abs(np.array(LOG_SPAN) + LN2) + 2 * a
                    + 2 * np.log1p(np.exp(-2 * a))).sum(1) + np.abs(l[np.arange(rows), k] - m[:, 0]) + np.abs(logW[:, 0])
    scale_ent = 1 + (np.abs(ls) + HALF_LOG_2PIE).sum(1) + np.abs(H[:, 0])
    G, E = np.abs(g_lp.astype(np.float64))[:, None], np.abs(g_ent.astype(np.float64))[:, None]
    scale_grad = np.concatenate([1 + G * np.abs(z / np.exp(ls)), 1 + G * z * z + G + E,
                                 1 + G * (1 + p) + E * p * (np.abs(logp) + np.abs(H))], axis=1)
    assert all(np.isfinite(x).all() for x in (lp, ent, grad, ev["log_prob64"], ev["entropy64"], bw["grad_params64"]))
    worst = dict(log_prob=(np.abs(ev["log_prob64"] - lp) / scale_lp).max(), entropy=(np.abs(ev["entropy64"] - ent) / scale_ent).max(),
                 grad=(np.abs(bw["grad_params64"] - grad) / scale_grad).max())
    print(M, worst)
    # the rounded outputs are the float64 values' float32, and the action of the stored u is the reference's transform of it
    assert same_bits(ev["log_prob"], ev["log_prob64"].astype(np.float32)) and same_bits(bw["grad_params"], bw["grad_params64"].astype(np.float32))
    sampled = policy_head_definition(SAMPLE, params, modes=MODES[M], deterministic=True, **CONSTS)
    means = torch_distributions(params, params[:, 0:4], np.zeros(rows, np.int32), g_lp, g_ent, M)[3]
    assert np.abs(sampled["action"] - means).max() <= 1e-12 * 200.0
    assert np.array_equal(sampled["mode_index"], l.argmax(1)) and np.array_equal(sampled["u"], params[:, 0:4])
    assert np.array_equal(sampled["current_mode"], np.asarray(MODES[M], dtype=np.int32)[l.argmax(1)])
    return worst


@pytest.mark.parametrize("M", ALL_M)
def test_the_definition_against_torch_distributions_in_float64(M):
    rows = 4096
    rng = np.random.default_rng(100 + M)
    params = random_params(rng, rows, M)
    u, k = random_stored(rng, params, M)
    g_lp, g_ent = rng.normal(size=rows).astype(np.float32), rng.normal(size=rows).astype(np.float32)
    worst = against_torch_distributions(M, params, u, k, g_lp, g_ent)
    for name, seen in SEEN.items():
        assert worst[name] <= 8 * seen, (name, worst[name])


@pytest.mark.parametrize("M", WIDE_M)
def test_the_definition_in_the_wide_regime_against_torch_distributions_in_float64(M):
    rows = 4096
    rng = np.random.default_rng(200 + M)
    params = wide_params(rng, rows, M)
    u, k = random_stored(rng, params, M)
    g_lp, g_ent = rng.normal(size=rows).astype(np.float32), rng.normal(size=rows).astype(np.float32)
    assert zero_probability_rows(params, M).sum() >= 50, "rows with a probability of exactly 0 occur"
    assert (np.abs(u) > 10.0).sum() >= 100, "stored values deep in the tanh's saturation occur"
    worst = against_torch_distributions(M, params, u, k, g_lp, g_ent)
    for name, seen in WIDE_SEEN.items():
        assert worst[name] <= 8 * seen, (name, worst[name])


# ------------------------------------------------------------------------------------------------ 4. what a draw claims
def draw(params, M=9, **kw):
    return policy_head_definition(SAMPLE, params, modes=MODES[M], **{**CONSTS, **kw})


def test_the_drawn_normals_and_modes_have_the_distribution_s_moments():
    n, M = 2 ** 16, 9
    row = random_params(np.random.default_rng(1), 1, M)
    params = np.repeat(row, n, axis=0)
    out = draw(params, seed=11, t=4)
    z = (out["u"].astype(np.float64) - row[0, 0:4]) / np.exp(row[0, 4:8].astype(np.float64))   # (u's float32 rounding: 1e-7)
    assert np.all(np.abs(z.mean(0)) <= 5.0 / math.sqrt(n))
    assert np.all(np.abs(z.var(0) - 1.0) <= 5.0 * math.sqrt(2.0 / n))
    assert np.all(np.abs(np.corrcoef(z.T)[np.triu_indices(4, 1)]) <= 5.0 / math.sqrt(n)), "the four components are independent"
    l = row[0, 8:].astype(np.float64)
    p = np.exp(l - l.max()) / np.exp(l - l.max()).sum()
    counts = np.bincount(out["mode_index"], minlength=M)
    assert np.all(np.abs(counts - n * p) <= 5.0 * np.sqrt(n * p * (1.0 - p))), (counts, n * p)
    assert np.array_equal(out["current_mode"], np.asarray(MODES[M])[out["mode_index"]])
    assert np.all(out["action"] >= np.array(LO)) and np.all(out["action"] <= np.array(HI))


def test_seeds_steps_and_global_ids_give_independent_different_actions():
    n, M = 4096, 9
    params = np.repeat(random_params(np.random.default_rng(2), 1, M), n, axis=0)
    base = draw(params, seed=21, t=7, env_id_offset=0)
    l = params[0, 8:].astype(np.float64)
    agree = float(((np.exp(l - l.max()) / np.exp(l - l.max()).sum()) ** 2).sum())
    for what, kw in (("seed", dict(seed=22, t=7, env_id_offset=0)), ("step", dict(seed=21, t=8, env_id_offset=0)),
                     ("high word of the step", dict(seed=21, t=7 + 2 ** 32, env_id_offset=0)),
                     ("high word of the seed", dict(seed=21 + 2 ** 32, t=7, env_id_offset=0)),
                     ("global id", dict(seed=21, t=7, env_id_offset=n))):
        other = draw(params, **kw)
        assert not (other["u"] == base["u"]).any(), what
        a, b = base["u"][:, 0].astype(np.float64), other["u"][:, 0].astype(np.float64)
        assert abs(np.corrcoef(a, b)[0, 1]) <= 5.0 / math.sqrt(n), what
        same_mode = (other["mode_index"] == base["mode_index"]).mean()   # independent draws agree with probability sum p^2
        assert abs(same_mode - agree) <= 5.0 * math.sqrt(agree * (1.0 - agree) / n), what
    assert not (base["u"][1:] == base["u"][:-1]).any(), "neighbouring global ids draw different values"
    again = draw(params, seed=21, t=7, env_id_offset=0)
    assert all(same_bits(again[k], base[k]) for k in base)


def test_a_batch_equals_its_shards_with_their_offsets():
    M = 9
    params = random_params(np.random.default_rng(3), 300, M)
    whole = draw(params, seed=31, t=2, env_id_offset=1000)
    a = draw(params[:128], seed=31, t=2, env_id_offset=1000)
    b = draw(params[128:], seed=31, t=2, env_id_offset=1128)
    for k in whole:
        assert same_bits(np.concatenate([a[k], b[k]]), whole[k]), k
    wrap = draw(params, seed=31, t=2, env_id_offset=2 ** 32 - 100)   # the global id is taken modulo 2^32
    assert same_bits(wrap["u"][100:], draw(params[100:], seed=31, t=2, env_id_offset=0)["u"])


def _vec(n=6, max_episode_steps=3000):
    return WireEDMVectorEnv(make("cpu", n, "autoreset", "s13"), max_episode_steps=max_episode_steps)


def test_reseed_and_load_state_dict_replay_exactly():
    vec = _vec()
    head = PolicyHead(vec, modes=(5, 9, 13), bounds={"servo": (-0.5, 0.5)}, seed=41)
    gen = torch.Generator().manual_seed(1)
    rows = [torch.randn(6, head.param_dim, generator=gen) for _ in range(4)]
    keep = lambda o: {k: getattr(o, k).clone() for k in ("u", "mode_index", "log_prob", "entropy")} | \
        {"servo": o.action.servo.clone(), "mode": o.action.current_mode.clone()}   # noqa: E731
    first = [keep(head.sample(r)) for r in rows[:2]]
    sd = head.state_dict()
    assert sd == {"seed": 41, "t": 2, "modes": [5, 9, 13], "bounds": head.bounds}
    rest = [keep(head.sample(r)) for r in rows[2:]]
    assert not same_bits(first[0]["u"], keep(head.sample(rows[0]))["u"]), "another step number draws other values"
    head.reseed(41)
    assert head.t == 0
    again = [keep(head.sample(r)) for r in rows]
    assert all(same_bits(x[k], y[k]) for x, y in zip(first + rest, again) for k in x)
    other = PolicyHead(_vec(), seed=0)
    other.load_state_dict(sd)
    assert other.state_dict() == sd and other.param_dim == 11
    resumed = [keep(other.sample(r)) for r in rows[2:]]
    assert all(same_bits(x[k], y[k]) for x, y in zip(rest, resumed) for k in x)
    det = keep(other.sample(rows[0], deterministic=True))
    assert other.t == 4 and same_bits(det["u"], rows[0][:, 0:4]), "a deterministic call draws nothing and keeps the step number"


def test_misuse_is_refused():
    vec = _vec()
    for bad in ((), (5, 5), (2,), (5, 20)):
        with pytest.raises(ValueError, match="modes"):
            PolicyHead(vec, modes=bad)
    for bad in ({"servo": (-2.0, 1.0)}, {"ON_time": (0.0, 6.0)}, {"OFF_time": (5.0, 5.0)}, {"target_voltage": (0.0, math.nan)},
                {"current_mode": (1, 19)}):
        with pytest.raises(ValueError, match="bounds"):
            PolicyHead(vec, bounds=bad)
    head = PolicyHead(vec)
    assert head.param_dim == 8 + len(VALID_CRATER_MODES) and head.modes == tuple(VALID_CRATER_MODES)
    assert head.bounds == dict(servo=(-1.0, 1.0), target_voltage=(0.0, 200.0), ON_time=(0.0, 5.0), OFF_time=(0.0, 100.0))
    for bad in (torch.zeros(6, head.param_dim + 1), torch.zeros(5, head.param_dim), torch.zeros(6, head.param_dim, dtype=torch.float64),
                np.zeros((6, head.param_dim), np.float32)):
        with pytest.raises(ValueError, match="params"):
            head.sample(bad)
    p = torch.zeros(6, head.param_dim)
    with pytest.raises(ValueError, match="u must"):
        head.evaluate(p, torch.zeros(6, 3), torch.zeros(6, dtype=torch.int32))
    with pytest.raises(ValueError, match="mode_index"):
        head.evaluate(p, torch.zeros(6, 4), torch.zeros(6))


# ------------------------------------------------------------------------------------------------ 5. through the stack
def test_policy_head_through_the_vector_env_and_the_rollout_buffer_on_the_oracle_backend():
    n, T = 6, 3
    vec = _vec(n)
    modes = (5, 9, 13)
    bounds = {"servo": (-0.2, 0.4), "target_voltage": (60.0, 100.0), "ON_time": (1.0, 4.0), "OFF_time": (20.0, 60.0)}
    head = PolicyHead(vec, modes=modes, bounds=bounds, seed=51)
    assert head._native is None
    buf = RolloutBuffer(vec, T, extras={"log_prob": torch.float32})
    gen = torch.Generator().manual_seed(2)
    obs, _ = vec.reset(seed=5)
    vec.env.state.workpiece_position = torch.linspace(10.5, 14.0, n, dtype=torch.float64)
    vec.env.state.wire_position = 10.0
    rows, seen = [], []
    first = None
    for _ in range(T):
        params = torch.randn(n, head.param_dim, generator=gen)
        out = head.sample(params)
        assert first is None or (out is first and out.action is first.action), "the same object at every call"
        first = out
        a = out.action
        seen.append({"u": out.u.clone(), "mode_index": out.mode_index.clone(), "log_prob": out.log_prob.clone(),
                     "mode": a.current_mode.clone(), "leaves": torch.stack([a.servo, a.target_voltage, a.on_time, a.off_time], 1).clone()})
        nxt, reward, term, trunc, _ = vec.step(a)
        buf.add(obs, head.stored(out), torch.zeros(n), reward, term, trunc, log_prob=out.log_prob)
        rows.append(params)
        obs = nxt
    buf.finish(torch.zeros(n))
    vec.env.check_errors()   # no mode without crater data reached the environment
    flat = buf.flat()
    stack = lambda name: torch.cat([s[name] for s in seen])   # noqa: E731
    assert same_bits(flat["action.u"], stack("u")) and same_bits(flat["action.mode_index"], stack("mode_index"))
    assert same_bits(flat["log_prob"], stack("log_prob"))
    lp, ent = head.evaluate(torch.cat(rows), flat["action.u"], flat["action.mode_index"])
    assert same_bits(lp, flat["log_prob"]), "evaluate at the sampling parameters returns the stored log_prob's bits"
    assert ent.shape == (T * n,) and bool(torch.isfinite(ent).all())
    assert set(stack("mode").tolist()) <= set(modes) and len(set(stack("mode").tolist())) > 1
    leaves = stack("leaves")
    lo = torch.tensor([bounds[k][0] for k in ("servo", "target_voltage", "ON_time", "OFF_time")], dtype=torch.float64)
    hi = torch.tensor([bounds[k][1] for k in ("servo", "target_voltage", "ON_time", "OFF_time")], dtype=torch.float64)
    assert bool((leaves >= lo).all() and (leaves <= hi).all()) and leaves.dtype == torch.float64
    assert bool((leaves.std(0) > 0).all())
    # the gradient through evaluate is the definition's BACKWARD
    leaf = torch.cat(rows).requires_grad_(True)
    lp, ent = head.evaluate(leaf, flat["action.u"], flat["action.mode_index"])
    (lp * torch.arange(T * n, dtype=torch.float32)).sum().backward()
    want = policy_head_definition(BACKWARD, leaf.detach(), modes=modes, lo=head._lo, hi=head._hi, log_span=head._log_span,
                                  u=flat["action.u"], mode_index=flat["action.mode_index"],
                                  g_log_prob=torch.arange(T * n, dtype=torch.float32))
    assert same_bits(leaf.grad, want["grad_params"])
