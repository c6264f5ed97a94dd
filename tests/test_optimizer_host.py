"""Adam with clipping and a KL gate (sparc_amd/optimizer.py) on the host side: the ABI mirror of
``wedm_opt_desc`` and the export with its refusals (no device is needed); the tree of the squared gradient against a plain
recursion; hand-worked cases of the definition; the definition against ``clip_grad_norm_`` and ``torch.optim.AdamW`` in float64;
a checkpoint of an `Adam` alone; and the training stacks of tests/_resume_common.py with a `PolicyNet` and an `Adam` on the CPU
oracle backend, cut at every control step.

Measured here (and recorded in DESIGN.md section 4.23; the bound below is 8 times it):
    50 steps at n = 1 000 against torch in float64, relative to 1 + |theta|: 3.3e-7"""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from sparc_amd import Adam, _abi, _lib
from sparc_amd.optimizer import (APPLIED, B1POW, B2POW, BC1, BC2, FRESH_STATE, INFO_NAMES, KL, LATCH, LR, NORM, SCALE, SKIPPED_KL,
                                 SKIPPED_NONFINITE, STATE_NAMES, SUMSQ, T, adam_reference)
from tests import _optimizer_common as oc
from tests._normalize_common import same_bits

ROOT = Path(__file__).resolve().parent.parent
TORCH_MEASURED = 3.3e-7


# ------------------------------------------------------------------------------------------------ 1. the C-ABI
def test_desc_struct_mirror_matches_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wedm_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(wedm_opt_desc));']
    for field, _ in _abi.OptDesc._fields_:
        lines.append(f'  printf("{field} %zu\\n", offsetof(wedm_opt_desc, {field}));')
    lines += ['  printf("consts %d %d %d %d abi %d\\n", WEDM_OPT_STATE, WEDM_OPT_INFO, WEDM_OPT_ONE_BLOCK_MAX, WEDM_NORM_MAX_TILES, WEDM_ABI_VERSION);',
              '  printf("flagbits %d %d %d %d %d %d\\n", WEDM_OPT_CLIP, WEDM_OPT_KL_GATE, WEDM_OPT_NEW_UPDATE, WEDM_OPT_NORM, WEDM_OPT_DECIDE, WEDM_OPT_APPLY);',
              '  printf("statewords %d %d %d %d %d %d\\n", WEDM_OS_B1POW, WEDM_OS_B2POW, WEDM_OS_T, WEDM_OS_SKIPPED_NONFINITE, WEDM_OS_SKIPPED_KL, WEDM_OS_LATCH);',
              '  printf("infowords %d %d %d %d %d %d %d %d\\n", WEDM_OI_SUMSQ, WEDM_OI_NORM, WEDM_OI_SCALE, WEDM_OI_LR, WEDM_OI_APPLIED, WEDM_OI_KL, WEDM_OI_BC1, WEDM_OI_BC2);',
              '  printf("klword %d\\n", WEDM_PT_KL);', "  return 0;", "}"]
    src = tmp_path / "desc.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "desc"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    out = dict(row.split(" ", 1) for row in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("size")) == C.sizeof(_abi.OptDesc)
    assert out.pop("consts") == f"{_abi.OPT_STATE} {_abi.OPT_INFO} {_abi.OPT_ONE_BLOCK_MAX} {_abi.NORM_MAX_TILES} abi 4" and _abi.OPT_STATE == _abi.OPT_INFO == 8
    assert 1 <= _abi.OPT_ONE_BLOCK_MAX <= 65536
    assert out.pop("flagbits") == "1 2 4 8 16 32" == " ".join(str(x) for x in (_abi.OPT_CLIP, _abi.OPT_KL_GATE, _abi.OPT_NEW_UPDATE, _abi.OPT_NORM,
                                                                                _abi.OPT_DECIDE, _abi.OPT_APPLY))
    assert out.pop("statewords") == " ".join(str(x) for x in (B1POW, B2POW, T, SKIPPED_NONFINITE, SKIPPED_KL, LATCH)) == "0 1 2 3 4 5"
    assert out.pop("infowords") == " ".join(str(x) for x in (SUMSQ, NORM, SCALE, LR, APPLIED, KL, BC1, BC2)) == "0 1 2 3 4 5 6 7"
    assert len(STATE_NAMES) == 6 and len(INFO_NAMES) == 8 and int(out.pop("klword")) == oc.KL_AT
    assert {k: int(v) for k, v in out.items()} == {f: getattr(_abi.OptDesc, f).offset for f, _ in _abi.OptDesc._fields_}


def test_the_call_is_exported_and_the_abi_version_stays():
    assert "wedm_adam" in _lib.EXPORTS and hasattr(_lib.HipBackend, "adam")
    L = _lib.load()
    assert L.wedm_adam is not None and L.wedm_abi_version() == _abi.ABI_VERSION == 4
    assert "int32_t wedm_adam(const wedm_opt_desc* desc, void* stream);" in (ROOT / "include" / "wedm_hip.h").read_text()


def test_bad_arguments_are_refused_before_anything_is_launched():
    """Every pointer below is an address nobody owns: a call that launched would fault (and on a machine without a device
    fail with WEDM_ERR_HIP); every case returns WEDM_ERR_BAD_ARG with a text."""
    L = _lib.load()
    A, n = 0x1000000, 1000   # blocks 0x100000 apart: the largest holds 4 000 bytes
    names = ("theta", "m", "v", "grad", "partials", "state", "info", "kl")
    at = {name: A + 0x100000 * i for i, name in enumerate(names)}
    size = {"theta": 4 * n, "m": 4 * n, "v": 4 * n, "grad": 4 * n, "partials": 8 * 4, "state": 64, "info": 64, "kl": 8}
    elem = {k: 4 if k in ("theta", "m", "v", "grad") else 8 for k in names}
    GATED = _abi.OPT_CLIP | _abi.OPT_KL_GATE
    nan, inf = float("nan"), float("inf")

    def desc(**kw):
        f = dict(at, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-5, weight_decay=0.01, max_norm=0.5, kl_limit=0.02, n=n, flags=GATED)
        f.update(kw)
        return _abi.OptDesc(**f)

    def refused(d, what):
        assert L.wedm_adam(C.byref(d), None) == _abi.ERR_BAD_ARG, what
        text = L.wedm_last_error(None)
        assert text.startswith(b"wedm_adam: ") and len(text) > len(b"wedm_adam: "), what

    assert L.wedm_adam(None, None) == _abi.ERR_BAD_ARG and L.wedm_last_error(None).startswith(b"wedm_adam:")
    for flags in (64, -1, 1 << 30, 128 | _abi.OPT_NORM, GATED | 256):
        refused(desc(flags=flags), ("flags", flags))
    for bad_n in (0, -5, _abi.NORM_MAX_TILES * 256 + 1, 2 ** 31 - 1):
        refused(desc(n=bad_n), ("n", bad_n))
    for name, values in (("lr", (-1e-9, nan, inf, -inf)), ("beta1", (-0.1, 1.0, 1.5, nan, inf)), ("beta2", (-0.1, 1.0, 1.5, nan, -inf)),
                         ("eps", (0.0, -1e-8, nan, inf)), ("weight_decay", (-1e-3, nan, inf)), ("max_norm", (0.0, -1.0, nan, inf)),
                         ("kl_limit", (-1e-9, nan, inf))):
        for x in values:
            refused(desc(**{name: x}), (name, x))
            for flags in (_abi.OPT_NORM, _abi.OPT_DECIDE, _abi.OPT_APPLY):   # in whichever phase
                refused(desc(flags=GATED | flags, **{name: x}), (name, x, flags))
    # every block a phase needs: null, and one byte off
    for name in names:
        refused(desc(**{name: None}), ("null", name))
        refused(desc(**{name: at[name] + 1}), ("one byte off", name))
    for name in ("partials", "state", "info", "kl"):
        refused(desc(**{name: at[name] + 4}), ("to 8 bytes", name))
    for flags, needed in ((_abi.OPT_NORM, ("grad", "partials")), (_abi.OPT_DECIDE, ("partials", "state", "info", "kl")),
                          (_abi.OPT_APPLY, ("theta", "m", "v", "grad", "info"))):
        for name in needed:
            refused(desc(flags=GATED | flags, **{name: None}), ("null in its phase alone", flags, name))
    # every output block on every input block: the same address, the input's last element, the output's last element
    outputs, inputs = ("theta", "m", "v", "partials", "state", "info"), ("grad", "kl")
    for o in outputs:
        for i in inputs:
            refused(desc(**{o: at[i]}), (o, "on", i))
            last = at[i] + size[i] - max(elem[o], elem[i])
            refused(desc(**{o: last - last % elem[o]}), (o, "on the last element of", i))
            first = at[i] - size[o] + elem[o]
            refused(desc(**{o: first + (-first) % elem[o]}), ("the last element of", o, "on", i))
    # every output block on every other output block
    for a in outputs:
        for b in outputs:
            if a != b:
                refused(desc(**{a: at[b]}), (a, "on", b))
                last = at[b] + size[b] - max(elem[a], elem[b])
                refused(desc(**{a: last - last % elem[a]}), (a, "on the last element of", b))


# ------------------------------------------------------------------------------------------------ 2. the tree
def _tree(leaves, width):
    """A plain recursion over a range padded with +0.0 to ``width``, a power of two: the lower index on the left."""
    if width == 1:
        return leaves[0] if len(leaves) else np.float64(0.0)
    half = width // 2
    return _tree(leaves[:half], half) + _tree(leaves[half:], half)


@pytest.mark.parametrize("n", (1, 255, 256, 257, 513, 65537))
def test_the_sum_of_squares_is_the_tree_bit_for_bit(n):
    rng = np.random.default_rng(n)
    g = (rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    state = np.array(FRESH_STATE)
    theta = np.zeros(n, dtype=np.float32)
    info, partials = adam_reference(theta, theta.copy(), theta.copy(), g, state, lr=0.0)
    q = g.astype(np.float64) * g.astype(np.float64)
    tiles = -(-n // 256)
    want_tiles = np.array([_tree(q[256 * t: 256 * t + 256], 256) for t in range(tiles)])
    padded = 1
    while padded < tiles:
        padded *= 2
    assert partials.shape == (tiles,) and same_bits(partials, want_tiles)
    assert same_bits(info[SUMSQ], _tree(want_tiles, padded)) and same_bits(info[NORM], np.sqrt(info[SUMSQ]))
    if n > 256:   # the order matters: this is not the left-to-right sum
        assert float(info[SUMSQ]) != float(np.cumsum(q)[-1]) or n < 1000


# ------------------------------------------------------------------------------------------------ 3. hand-worked cases
def _blocks(theta, m=None, v=None):
    theta = np.asarray(theta, dtype=np.float32)
    zeros = np.zeros_like(theta)
    return theta.copy(), (zeros if m is None else np.asarray(m, dtype=np.float32)).copy(), \
        (zeros if v is None else np.asarray(v, dtype=np.float32)).copy(), np.array(FRESH_STATE)


def test_three_four_five_and_the_clipping_factor():
    theta, m, v, state = _blocks([1.0, 2.0])
    info, partials = adam_reference(theta, m, v, np.array([3.0, 4.0], dtype=np.float32), state, lr=1e-3, max_norm=1.0)
    assert info[SUMSQ] == 25.0 and info[NORM] == 5.0 and info[SCALE] == 1.0 / (5.0 + 1e-6) and partials.tolist() == [25.0]
    assert info[APPLIED] == 1.0 and info[LR] == 1e-3 and info[KL] == 0.0
    assert state.tolist() == [0.9, 0.999, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0] and info[BC1] == 1.0 - 0.9 and info[BC2] == 1.0 - 0.999
    # the element by hand, in Python's float64
    c = 1.0 / (5.0 + 1e-6)
    for e, (p0, g0) in enumerate(((1.0, 3.0), (2.0, 4.0))):
        g = g0 * c
        mf = float(np.float32((1.0 - 0.9) * g))
        vf = float(np.float32((1.0 - 0.999) * (g * g)))
        want = np.float32(p0 - 1e-3 * ((mf / (1.0 - 0.9)) / (float(np.sqrt(vf / (1.0 - 0.999))) + 1e-5)))
        assert same_bits(theta[e], want) and same_bits(m[e], np.float32(mf)) and same_bits(v[e], np.float32(vf))
    # without clipping, and with a max_norm above the norm: the factor is exactly 1
    for max_norm in (None, 7.0):
        th2, m2, v2, st2 = _blocks([1.0, 2.0])
        info = adam_reference(th2, m2, v2, np.array([3.0, 4.0], dtype=np.float32), st2, lr=1e-3, max_norm=max_norm)[0]
        assert info[SCALE] == 1.0


def test_an_all_zero_gradient_changes_no_bit_of_theta_and_advances_t():
    start = np.array([0.5, -0.0, 0.0, -3.0, 1e-41], dtype=np.float32)
    for max_norm in (None, 0.5):
        theta, m, v, state = _blocks(start)
        info = adam_reference(theta, m, v, np.zeros(5, dtype=np.float32), state, lr=1e-2, max_norm=max_norm)[0]
        assert same_bits(theta, start) and np.signbit(theta[1]) and not np.signbit(theta[2])
        assert state[T] == 1.0 and info[APPLIED] == 1.0 and info[SUMSQ] == 0.0 and info[SCALE] == 1.0
        assert same_bits(m, np.zeros(5, dtype=np.float32)) and same_bits(v, np.zeros(5, dtype=np.float32))


@pytest.mark.parametrize("poison", (np.nan, np.inf, -np.inf))
def test_a_gradient_that_is_not_finite_is_skipped_and_counted(poison):
    rng = np.random.default_rng(1)
    n = 300
    theta, m, v, state = _blocks(rng.normal(size=n), 0.01 * rng.normal(size=n), 1e-4 * rng.random(n))
    state[:3] = 0.81, 0.998, 2.0
    held = (theta.copy(), m.copy(), v.copy(), state.copy())
    g = rng.normal(size=n).astype(np.float32)
    g[257] = poison
    info = adam_reference(theta, m, v, g, state, lr=1e-2, max_norm=0.5)[0]
    assert same_bits(theta, held[0]) and same_bits(m, held[1]) and same_bits(v, held[2])
    assert state[SKIPPED_NONFINITE] == 1.0 and same_bits(state[:3], held[3][:3]) and info[APPLIED] == 0.0
    assert info[SCALE] == (1.0 if poison != poison else 0.0) and (info[SUMSQ] != info[SUMSQ]) == (poison != poison)
    if poison != poison:
        assert info[[SUMSQ, NORM]].view(np.uint64).tolist() == [0x7FF8000000000000] * 2
    g[257] = 0.0   # the next, finite, gradient is applied
    info = adam_reference(theta, m, v, g, state, lr=1e-2, max_norm=0.5)[0]
    assert info[APPLIED] == 1.0 and state[T] == 3.0 and state[SKIPPED_NONFINITE] == 1.0 and not same_bits(theta, held[0])


def test_the_kl_gate_latches_until_a_new_update_and_a_nan_closes_it():
    rng = np.random.default_rng(2)
    n = 40
    theta, m, v, state = _blocks(rng.normal(size=n))
    g = rng.normal(size=n).astype(np.float32)

    def step(kl, **kw):
        before = theta.copy()
        info = adam_reference(theta, m, v, g, state, lr=1e-2, kl=kl, kl_limit=0.02, **kw)[0]
        assert (info[APPLIED] == 1.0) == (not same_bits(theta, before))
        assert same_bits(info[KL], np.float64(kl)) or kl != kl
        return info[APPLIED]

    assert step(0.02) == 1.0 and state[LATCH] == 0.0          # at the limit: not over it
    assert step(0.0200001) == 0.0 and state[LATCH] == 1.0     # over it: skipped, latched
    assert step(0.0) == 0.0 and state[LATCH] == 1.0           # the next call with kl = 0 is skipped too
    assert step(0.0, new_update=True) == 1.0 and state[LATCH] == 0.0
    assert step(float("nan")) == 0.0 and state[LATCH] == 1.0  # a NaN latches
    assert step(0.0) == 0.0
    assert step(0.5, new_update=True) == 0.0 and state[LATCH] == 1.0   # a new update whose first minibatch is over the limit
    assert state[T] == 2.0 and state[SKIPPED_KL] == 5.0 and state[SKIPPED_NONFINITE] == 0.0
    assert same_bits(state[:2], np.array([0.9 * 0.9, 0.999 * 0.999]))
    # without a limit kl is not looked at, and a gradient that is not finite under a closed gate counts as a KL skip
    th2, m2, v2, st2 = _blocks(theta)
    assert adam_reference(th2, m2, v2, g, st2, lr=1e-2, kl=float("nan"))[0][APPLIED] == 1.0
    g_bad = g.copy()
    g_bad[3] = np.inf
    assert step(0.0) == 0.0 and adam_reference(theta, m, v, g_bad, state, lr=1e-2, kl=0.0, kl_limit=0.02)[0][APPLIED] == 0.0
    assert state[SKIPPED_NONFINITE] == 0.0 and state[SKIPPED_KL] == 7.0


def test_beta1_zero_and_weight_decay_on_and_off():
    rng = np.random.default_rng(3)
    n = 50
    start, g = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
    theta, m, v, state = _blocks(start, rng.normal(size=n))
    info = adam_reference(theta, m, v, g, state, lr=1e-2, betas=(0.0, 0.99))[0]
    assert state[B1POW] == 0.0 and info[BC1] == 1.0 and same_bits(m, g)   # the first moment is the gradient
    info = adam_reference(theta, m, v, g, state, lr=1e-2, betas=(0.0, 0.99))[0]
    assert state[B1POW] == 0.0 and info[BC1] == 1.0 and same_bits(m, g) and state[T] == 2.0
    # decoupled weight decay: p - (lr wd) p before the step, the moments untouched by it
    plain, decayed = _blocks(start), _blocks(start)
    adam_reference(*plain[:3], g, plain[3], lr=1e-2, weight_decay=0.0)
    adam_reference(*decayed[:3], g, decayed[3], lr=1e-2, weight_decay=0.1)
    assert same_bits(plain[1], decayed[1]) and same_bits(plain[2], decayed[2]) and not same_bits(plain[0], decayed[0])
    p64 = start.astype(np.float64)
    moved = plain[0].astype(np.float64) - p64   # (up to the float32 rounding of theta)
    assert np.allclose(decayed[0], (p64 - (1e-2 * 0.1) * p64) + moved, rtol=0, atol=1e-6)
    # a zero gradient with weight decay still shrinks theta
    th, m0, v0, st = _blocks(start)
    adam_reference(th, m0, v0, np.zeros(n, dtype=np.float32), st, lr=1e-2, weight_decay=0.1)
    assert same_bits(th, (p64 - (1e-2 * 0.1) * p64).astype(np.float32))


# ------------------------------------------------------------------------------------------------ 4. against torch in float64
def test_fifty_steps_against_clip_grad_norm_and_adamw_in_float64():
    rng = np.random.default_rng(50)
    n, max_norm, kw = 1000, 0.5, dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-5, weight_decay=0.01)
    theta, m, v, state = _blocks(rng.normal(size=n))
    ref = torch.tensor(theta.astype(np.float64), requires_grad=True)
    opt = torch.optim.AdamW([ref], lr=kw["lr"], betas=kw["betas"], eps=kw["eps"], weight_decay=kw["weight_decay"])
    worst, clipped = 0.0, []
    for k in range(50):
        g = ((0.1 + 0.9 * rng.random()) * rng.normal(size=n) / np.sqrt(n)).astype(np.float32)   # norms from 0.1 to 1
        info = adam_reference(theta, m, v, g, state, max_norm=max_norm, **kw)[0]
        clipped.append(bool(info[SCALE] < 1.0))
        ref.grad = torch.tensor(g.astype(np.float64))
        torch.nn.utils.clip_grad_norm_([ref], max_norm)
        opt.step()
        want = ref.detach().numpy()
        worst = max(worst, float((np.abs(theta.astype(np.float64) - want) / (1.0 + np.abs(want))).max()))
    print(f"50 steps against torch in float64: largest difference relative to 1 + |theta| {worst:.3g}")
    assert 10 <= sum(clipped) <= 40 and any(a != b for a, b in zip(clipped, clipped[1:])), "the norm crosses max_norm both ways"
    assert state[T] == 50.0 and worst <= 8 * TORCH_MEASURED


# ------------------------------------------------------------------------------------------------ 5. Adam, its checkpoint
def _drive(opt: Adam, theta: torch.Tensor, first: int, last: int, begin=(0, 4, 7, 11)) -> None:
    """Steps ``first .. last - 1`` of a fixed schedule: seeded gradients (one with a NaN), KL values that close the gate, and
    `begin_update` before the steps of ``begin``."""
    for k in range(first, last):
        if k in begin:
            opt.begin_update()
        g = torch.randn(theta.shape[0], generator=torch.Generator().manual_seed(100 + k)) * (0.05 if k % 3 else 1.0)
        if k == 9:
            g[5] = float("nan")
        theta.grad = g
        stats = torch.zeros(_abi.PPO_STATS, dtype=torch.float64)
        stats[oc.KL_AT] = (0.0, 0.01, 0.03, 0.0, 0.0, 0.01, 0.05, 0.01, 0.0, 0.0, 0.0, 0.0, 0.015, 0.0)[k]
        opt.step(stats)
        opt.zero_grad()


def test_a_checkpoint_of_adam_alone_resumes_byte_for_byte(tmp_path):
    n = 300
    start = torch.randn(n, generator=torch.Generator().manual_seed(1))
    lr = lambda k: 1e-2 / (1 + k)   # noqa: E731
    kw = dict(betas=(0.9, 0.99), eps=1e-6, weight_decay=0.01, max_grad_norm=0.5, kl_limit=0.02)
    whole_theta = start.clone().requires_grad_(True)
    whole = Adam(whole_theta, lr=lr, **kw)
    _drive(whole, whole_theta, 0, 14)
    a_theta = start.clone().requires_grad_(True)
    a = Adam(a_theta, lr=lr, **kw)
    _drive(a, a_theta, 0, 7)
    a.begin_update()   # pending at the cut: step 7 carries NEW_UPDATE
    torch.save({"opt": a.state_dict(), "theta": a_theta.detach().clone()}, tmp_path / "adam.pt")
    ck = torch.load(tmp_path / "adam.pt", map_location="cpu", weights_only=True)
    b_theta = torch.zeros(n).requires_grad_(True)
    b = Adam(b_theta, lr=lr, betas=(0.5, 0.6), eps=1e-3, weight_decay=0.5, max_grad_norm=None, kl_limit=None)
    _drive(b, b_theta, 0, 3)   # dirtied by steps of its own
    b.load_state_dict(ck["opt"])
    with torch.no_grad():
        b_theta.copy_(ck["theta"])
    assert b.calls == 7 and b._new_update and (b.betas, b.eps, b.weight_decay, b.max_grad_norm, b.kl_limit) == ((0.9, 0.99), 1e-6, 0.01, 0.5, 0.02)
    _drive(b, b_theta, 7, 14, begin=(11,))   # (step 7's begin_update is the pending one)
    for name, got, want in (("theta", b_theta, whole_theta), ("m", b.m, whole.m), ("v", b.v, whole.v), ("state", b.state, whole.state),
                            ("info", b.info, whole.info)):
        assert same_bits(got, want), name
    st = whole.state
    assert b.calls == whole.calls == 14 and st[SKIPPED_KL] >= 2 and st[SKIPPED_NONFINITE] == 1 and st[T] >= 5
    assert float(st[T] + st[SKIPPED_KL] + st[SKIPPED_NONFINITE]) == 14.0
    # refusals: moments of another length, a callable lr that the target lacks, no gradient, no stats
    other_theta = torch.zeros(n + 1).requires_grad_(True)
    other = Adam(other_theta, lr=lr)
    with pytest.raises(ValueError, match="m must be"):
        other.load_state_dict(ck["opt"])
    assert other.calls == 0 and same_bits(other.state, torch.tensor(FRESH_STATE, dtype=torch.float64))
    with pytest.raises(ValueError, match="callable"):
        Adam(torch.zeros(n).requires_grad_(True), lr=1e-3).load_state_dict(ck["opt"])
    with pytest.raises(RuntimeError, match="grad is None"):
        b.step(torch.zeros(8, dtype=torch.float64))
    b_theta.grad = torch.zeros(n)
    with pytest.raises(ValueError, match="stats"):
        b.step()
    for bad in (dict(lr=-1.0), dict(betas=(1.0, 0.9)), dict(eps=0.0), dict(weight_decay=-1.0), dict(max_grad_norm=0.0), dict(kl_limit=-1.0)):
        with pytest.raises(ValueError):
            Adam(torch.zeros(3).requires_grad_(True), **bad)
    with pytest.raises(ValueError):
        Adam(torch.zeros(3, 2).requires_grad_(True))


# ------------------------------------------------------------------------------------------------ 6. the stacks
@pytest.mark.parametrize("variant", ("in-kernel", "frozen", "host-reset"))
def test_the_stack_with_a_policy_net_and_adam_resumes_byte_for_byte_at_every_cut(variant, tmp_path):
    oc.check_resume_at_every_cut(variant, "cpu", tmp_path)
