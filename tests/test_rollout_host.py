"""Rollout storage and GAE (sparc_amd/rollout.py) on the host side: the ABI mirror of ``wedm_gae_desc``
and the export with its refusals (no device is needed), `torch_gae` against a textbook GAE written here in plain Python
loops and against hand-worked cases, its split invariance, and `RolloutBuffer` through `WireEDMVectorEnv` on the CPU oracle
backend (which has no ``gae`` and so runs the host path)."""
from __future__ import annotations

import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from sparc_amd import RolloutBuffer, WireEDMVectorEnv, _abi, _lib
from sparc_amd.rollout import APPLY, NORMALIZE, SCAN, SCAN_UNROLL, SKIP_AFTER_DONE, torch_gae
from tests._gae_common import FLAG_BYTES, GAE_KINDS, PAIRS, draw_mixed, is_subnormal, kinds_of
from tests._normalize_common import same_bits
from tests._snapshot_common import make

ROOT = Path(__file__).resolve().parent.parent


def draw(rng, T, N, p=0.1):
    """Float32 rewards, values and last values, and done flags with probability ``p`` each."""
    return dict(reward=rng.normal(size=(T, N)).astype(np.float32), value=rng.normal(size=(T, N)).astype(np.float32),
                last_value=rng.normal(size=N).astype(np.float32), terminated=rng.random((T, N)) < p,
                truncated=rng.random((T, N)) < p)


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_desc_struct_mirror_matches_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wedm_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(wedm_gae_desc));']
    for field, _ in _abi.GaeDesc._fields_:
        lines.append(f'  printf("{field} %zu\\n", offsetof(wedm_gae_desc, {field}));')
    lines += ['  printf("consts %d abi %d\\n", WEDM_GAE_MAX_STEPS, WEDM_ABI_VERSION);',
              '  printf("flagbits %d %d %d %d\\n", WEDM_GAE_SKIP_AFTER_DONE, WEDM_GAE_NORMALIZE, WEDM_GAE_SCAN, WEDM_GAE_APPLY);',
              "  return 0;", "}"]
    src = tmp_path / "desc.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "desc"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                   check=True)
    out = dict(row.split(" ", 1) for row in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("size")) == C.sizeof(_abi.GaeDesc)
    assert out.pop("consts") == f"{_abi.GAE_MAX_STEPS} abi 4" == "65536 abi 4"
    assert out.pop("flagbits") == f"{_abi.GAE_SKIP_AFTER_DONE} {_abi.GAE_NORMALIZE} {_abi.GAE_SCAN} {_abi.GAE_APPLY}" == "1 2 4 8"
    assert (SKIP_AFTER_DONE, NORMALIZE, SCAN, APPLY) == (1, 2, 4, 8)
    assert {k: int(v) for k, v in out.items()} == {f: getattr(_abi.GaeDesc, f).offset for f, _ in _abi.GaeDesc._fields_}


def test_the_call_is_exported_and_the_abi_version_stays():
    assert "wedm_gae" in _lib.EXPORTS
    L = _lib.load()
    assert L.wedm_gae is not None and L.wedm_abi_version() == _abi.ABI_VERSION == 4


def test_the_unroll_depth_python_names_is_the_kernel_header_s():
    text = (ROOT / "sparc_amd" / "csrc" / "wedm_gae.h").read_text()
    assert int(re.search(r"^#define WEDM_GAE_UNROLL (\d+)", text, re.M).group(1)) == SCAN_UNROLL


def test_bad_arguments_are_refused_before_anything_is_launched():
    """Every pointer below is an address nobody owns: a call that launched would fault (and on this machine, without a
    device, fail with WEDM_ERR_HIP); every case returns WEDM_ERR_BAD_ARG with a text."""
    L = _lib.load()
    A = 0x100000   # blocks 0x10000 apart: T = 16 rows of stride 128 are 8 192 bytes of float32

    def desc(**kw):
        f = dict(reward=A, value=A + 0x10000, last_value=A + 0x20000, terminated=A + 0x30000, truncated=A + 0x40000,
                 prev_done_in=A + 0x50000, advantage=A + 0x60000, returns=A + 0x70000, advantage_norm=A + 0x80000,
                 valid=A + 0x90000, prev_done_out=A + 0xA0000, partials=A + 0xB0000, moments=A + 0xC0000, in_stride=128,
                 out_stride=128, gamma=0.99, lam=0.95, eps=1e-8, T=16, num_envs=100, tile_offset=0, n_tiles_total=1,
                 flags=SKIP_AFTER_DONE | NORMALIZE)
        f.update(kw)
        return _abi.GaeDesc(**f)

    def refused(d, what):
        assert L.wedm_gae(C.byref(d), None) == _abi.ERR_BAD_ARG, what
        assert b"wedm_gae" in L.wedm_last_error(None), what

    assert L.wedm_gae(None, None) == _abi.ERR_BAD_ARG and L.wedm_last_error(None).startswith(b"wedm_gae:")
    # NULLs that the flags need
    for name in ("reward", "value", "last_value", "terminated", "truncated", "advantage", "returns", "valid", "advantage_norm",
                 "partials", "moments"):
        refused(desc(**{name: None}), name)
    refused(desc(flags=0, reward=None), "SCAN without NORMALIZE needs reward")
    refused(desc(flags=NORMALIZE | SCAN, partials=None), "SCAN with NORMALIZE needs partials")
    refused(desc(flags=NORMALIZE | APPLY, moments=None), "APPLY needs moments")
    refused(desc(flags=NORMALIZE | APPLY, advantage_norm=None), "APPLY needs advantage_norm")
    # num_envs, T, strides
    refused(desc(num_envs=0), "num_envs 0")
    refused(desc(num_envs=-3), "num_envs negative")
    refused(desc(T=0), "T 0")
    refused(desc(T=_abi.GAE_MAX_STEPS + 1), "T past the limit")
    refused(desc(in_stride=99), "in_stride")
    refused(desc(out_stride=99), "out_stride")
    # the tile range
    refused(desc(tile_offset=-1), "negative offset")
    refused(desc(tile_offset=1), "past the workspace")
    refused(desc(num_envs=257, in_stride=300, out_stride=300), "two tiles in a workspace of one")
    refused(desc(n_tiles_total=0), "no workspace")
    refused(desc(n_tiles_total=_abi.NORM_MAX_TILES + 1), "too many tiles")
    # numbers that are not finite, flags
    for name in ("gamma", "lam", "eps"):
        for x in (math.nan, math.inf, -math.inf):
            refused(desc(**{name: x}), (name, x))
    refused(desc(flags=16), "undefined flag")
    refused(desc(flags=-1), "undefined flags")
    # an output block on an input block: the same address, its last row's last element, the byte before its first
    last = (15 * 128 + 100) * 4
    refused(desc(advantage=A), "advantage on reward")
    refused(desc(returns=A + 0x10000 + last - 4), "returns on value's last element")
    refused(desc(advantage_norm=A + 0x10000 - last + 4), "advantage_norm's last element on value")
    refused(desc(valid=A + 0x30000 + 5), "valid inside terminated")
    refused(desc(prev_done_out=A + 0x40000), "prev_done_out on truncated")
    refused(desc(moments=A + 0x20000 + 8), "moments inside last_value")
    refused(desc(partials=A + 0x50000 + 96), "partials on prev_done_in")
    refused(desc(valid=A + 0x50000), "valid on prev_done_in: only prev_done_out may alias it")


# ------------------------------------------------------------------------------------------------ the definition
def textbook_gae(reward, value, last_value, terminated, truncated, gamma, lam):
    """GAE as the textbooks and the common PPO implementations write it, one environment at a time in Python floats
    (float64): multiplications by 0 / 1 masks where the definition selects."""
    T, N = reward.shape
    adv, ret = np.zeros((T, N)), np.zeros((T, N))
    for e in range(N):
        gae = 0.0
        for t in reversed(range(T)):
            next_value = float(last_value[e]) if t == T - 1 else float(value[t + 1, e])
            bootstrap = 0.0 if terminated[t, e] else 1.0
            carry = 0.0 if (terminated[t, e] or truncated[t, e]) else 1.0
            delta = float(reward[t, e]) + gamma * next_value * bootstrap - float(value[t, e])
            gae = delta + gamma * lam * carry * gae
            adv[t, e] = gae
            ret[t, e] = gae + float(value[t, e])
    return adv, ret


def test_torch_gae_against_a_textbook_gae():
    """Agreement to 1e-12 relative of the float32 outputs with the textbook's float64 results rounded to float32.  The two
    orderings (gamma * next_value * mask against a select; gamma * lam * mask * gae against gl * gae) may round differently
    in float64; observed maximum over these 12 x 40 x 2 values after the rounding to float32: 0."""
    rng = np.random.default_rng(1)
    x = draw(rng, 12, 40)
    got = torch_gae(**x, gamma=0.99, gae_lambda=0.95, flags=0)
    adv, ret = textbook_gae(**x, gamma=0.99, lam=0.95)
    for name, want in (("advantage", adv), ("returns", ret)):
        g, w = got[name].numpy().astype(np.float64), want.astype(np.float32).astype(np.float64)
        err = np.abs(g - w) / np.maximum(np.abs(w), 1e-300)
        print(name, "largest relative difference", err.max())
        assert err.max() <= 1e-12, name
    assert got["valid"].all() and "advantage_norm" not in got and "moments" not in got
    assert x["terminated"].any() and x["truncated"].any() and (x["terminated"] | x["truncated"])[:-1].any()


@pytest.mark.parametrize("gamma,lam", PAIRS, ids=[f"gamma{g}-lam{l}" for g, l in PAIRS])
def test_torch_gae_against_a_textbook_gae_on_mixed_kinds(gamma, lam):
    """26 x 513 environments of `GAE_KINDS` (normal, offset, constant, tiny, huge, subnormal, zeros, independently in
    ``reward``, ``value`` and ``last_value``) with flag bytes from {0, 1, 2, 0x80, 0xFF}: the criterion of the test above, 1e-12
    relative after rounding to float32.  Every output is finite -- the condition under which the device test compares bits
    -- with NumPy's overflow, invalid and division warnings raised as errors around the textbook's rounding (a subnormal
    result raises underflow by definition: that one is wanted here), and stored float32 subnormals occur."""
    T, N = 3 * SCAN_UNROLL + 2, 513
    x = draw_mixed(np.random.default_rng(11), T, N)
    for kinds in kinds_of(N):
        assert set(kinds.tolist()) == set(range(len(GAE_KINDS)))
    assert all(set(x[k].reshape(-1).tolist()) == set(FLAG_BYTES) for k in ("terminated", "truncated"))
    got = torch_gae(**x, gamma=gamma, gae_lambda=lam, flags=0)
    adv, ret = textbook_gae(**x, gamma=gamma, lam=lam)
    for name, want in (("advantage", adv), ("returns", ret)):
        with np.errstate(over="raise", invalid="raise", divide="raise"):
            w32 = want.astype(np.float32)
        g, w = got[name].numpy().astype(np.float64), w32.astype(np.float64)
        assert np.isfinite(g).all() and np.isfinite(w).all(), name
        err = np.abs(g - w) / np.maximum(np.abs(w), 1e-300)
        print(name, "largest relative difference", err.max(), "subnormals stored", int(is_subnormal(got[name].numpy()).sum()))
        assert err.max() <= 1e-12, name
        assert is_subnormal(got[name].numpy()).sum() >= 100, name
    both = torch_gae(**x, gamma=gamma, gae_lambda=lam, prev_done=x["terminated"][0])
    assert all(bool(torch.isfinite(both[k].to(torch.float64)).all()) for k in ("advantage", "returns", "advantage_norm", "moments", "partials"))
    assert set(both["prev_done_out"].tolist()) == {0, 1} and set(both["valid"].reshape(-1).tolist()) == {0, 1}


def test_lambda_zero_gives_the_one_step_residual_exactly():
    x = draw(np.random.default_rng(2), 9, 33)
    got = torch_gae(**x, gamma=0.97, gae_lambda=0.0, flags=0)
    r, v = x["reward"].astype(np.float64), x["value"].astype(np.float64)
    nv = np.concatenate([v[1:], x["last_value"].astype(np.float64)[None]])
    delta = (r + np.where(x["terminated"], 0.0, 0.97 * nv)) - v
    assert same_bits(got["advantage"], delta.astype(np.float32))


def test_lambda_one_gamma_one_without_dones_gives_the_reward_to_go():
    x = draw(np.random.default_rng(3), 10, 21, p=0.0)
    got = torch_gae(**x, gamma=1.0, gae_lambda=1.0, flags=0)
    to_go = np.cumsum(x["reward"].astype(np.float64)[::-1], axis=0)[::-1] + x["last_value"].astype(np.float64)
    # random float32 data: 1e-12 for the float64 recurrence against the float64 sum (two orders of summation), and half a
    # unit in the last place of the float32 the result is stored as
    assert np.all(np.abs(got["returns"].numpy().astype(np.float64) - to_go) <= (2.0 ** -24 + 1e-12) * np.abs(to_go) + 1e-12)
    # ... and to 1e-12 on the stored values themselves where nothing rounds: small integers
    rng = np.random.default_rng(4)
    y = dict(reward=rng.integers(-8, 9, (10, 21)).astype(np.float32), value=rng.integers(-8, 9, (10, 21)).astype(np.float32),
             last_value=rng.integers(-8, 9, 21).astype(np.float32), terminated=np.zeros((10, 21), bool), truncated=np.zeros((10, 21), bool))
    got = torch_gae(**y, gamma=1.0, gae_lambda=1.0, flags=0)
    to_go = np.cumsum(y["reward"].astype(np.float64)[::-1], axis=0)[::-1] + y["last_value"].astype(np.float64)
    np.testing.assert_allclose(got["returns"].numpy().astype(np.float64), to_go, rtol=1e-12, atol=0.0)


def test_a_terminated_step_does_not_see_the_next_value_and_a_truncated_one_does():
    x = draw(np.random.default_rng(5), 8, 4, p=0.0)
    x["terminated"][3, 1] = True
    x["truncated"][3, 2] = True
    base = torch_gae(**x, flags=0)
    moved = dict(x, value=x["value"].copy())
    moved["value"][4, :] += 1.0
    got = torch_gae(**moved, flags=0)
    for name in ("advantage", "returns"):
        assert same_bits(got[name][:4, 1], base[name][:4, 1]), "terminated: nothing at or before t moves"
        assert not torch.equal(got[name][3, 2], base[name][3, 2]), "truncated: bootstraps from value[t + 1]"
        assert not torch.equal(got[name][:4, 0], base[name][:4, 0]) and not torch.equal(got[name][:4, 3], base[name][:4, 3])
    # the last step: a terminated one does not see last_value, a truncated one does
    y = draw(np.random.default_rng(6), 3, 2, p=0.0)
    y["terminated"][2, 0], y["truncated"][2, 1] = True, True
    a, b = torch_gae(**y, flags=0), torch_gae(**dict(y, last_value=y["last_value"] + 1.0), flags=0)
    assert same_bits(a["advantage"][:, 0], b["advantage"][:, 0]) and not torch.equal(a["advantage"][2, 1], b["advantage"][2, 1])


def test_skip_after_done_on_a_hand_worked_case():
    """T = 5, a done at t = 1 and prev_done = 1; gamma = lambda = 1/2 and small integers, so every value is exact.  Steps 0
    and 2 are the steps after a done: skipped."""
    reward = np.array([[7.0], [2.0], [9.0], [1.0], [3.0]], dtype=np.float32)
    value = np.array([[1.0], [2.0], [4.0], [2.0], [1.0]], dtype=np.float32)
    last = np.array([8.0], dtype=np.float32)
    trunc = np.array([[0], [1], [0], [0], [0]], dtype=bool)
    got = torch_gae(reward, value, last, np.zeros((5, 1), bool), trunc, prev_done=np.array([1]), gamma=0.5, gae_lambda=0.5, eps=0.0)
    # t = 4: delta = 3 + 4 - 1 = 6, A = 6;  t = 3: delta = 1 + 0.5 - 2 = -0.5, A = -0.5 + 0.25 * 6 = 1
    # t = 2: skipped;  t = 1 (truncated): delta = 2 + 0.5 * value[2] - 2 = 2, the chain is cut: A = 2;  t = 0: skipped
    assert got["valid"][:, 0].tolist() == [0, 1, 0, 1, 1]
    assert got["advantage"][:, 0].tolist() == [0.0, 2.0, 0.0, 1.0, 6.0]
    assert got["returns"][:, 0].tolist() == [1.0, 4.0, 4.0, 3.0, 7.0]          # the skipped steps: returns == value
    assert got["prev_done_out"].tolist() == [0]                                # done_4
    # Welford over 6, 1, 2 in this order: n = 3, m = 3, S = 14; (x - 3) / sqrt(14 / 3)
    assert got["moments"].tolist() == [3.0, 3.0, 14.0]
    den = math.sqrt(14.0 / 3.0)
    assert got["advantage_norm"][:, 0].tolist() == [0.0, float(np.float32(-1.0 / den)), 0.0, float(np.float32(-2.0 / den)),
                                                    float(np.float32(3.0 / den))]
    done_last = torch_gae(reward, value, last, np.zeros((5, 1), bool), np.array([[0], [0], [0], [0], [1]], dtype=bool))
    assert done_last["prev_done_out"].tolist() == [1] and done_last["valid"][:, 0].tolist() == [1, 1, 1, 1, 1]
    # without the flag nothing is skipped, whatever prev_done says
    plain = torch_gae(reward, value, last, np.zeros((5, 1), bool), trunc, prev_done=np.array([1]), flags=NORMALIZE)
    assert plain["valid"].all() and plain["moments"][0] == 5.0


def test_split_invariance_on_the_host():
    """769 environments as shards of 512 + 257 (tiles 0-1 and 2-3) scanned into one workspace and then applied equal the
    whole batch in every bit."""
    x = draw(np.random.default_rng(7), 7, 769)
    prev = np.random.default_rng(8).random(769) < 0.2
    whole = torch_gae(**x, prev_done=prev)
    assert whole["partials"].shape == (4, 3)
    cut = lambda lo, hi: {k: np.ascontiguousarray(v[..., lo:hi]) for k, v in x.items()}
    a = torch_gae(**cut(0, 512), prev_done=prev[:512], flags=SKIP_AFTER_DONE | NORMALIZE | SCAN, n_tiles_total=4)
    b = torch_gae(**cut(512, 769), prev_done=prev[512:], flags=SKIP_AFTER_DONE | NORMALIZE | SCAN, tile_offset=2, n_tiles_total=4,
                  partials=a["partials"])
    assert same_bits(b["partials"], whole["partials"])
    applied = [torch_gae(**cut(lo, hi), flags=SKIP_AFTER_DONE | NORMALIZE | APPLY, tile_offset=off, n_tiles_total=4,
                         partials=b["partials"], advantage=s["advantage"], valid=s["valid"])
               for (lo, hi, off, s) in ((0, 512, 0, a), (512, 769, 2, b))]
    for name in ("advantage", "returns", "valid", "prev_done_out"):
        assert same_bits(torch.cat([a[name], b[name]], dim=-1), whole[name]), name
    assert same_bits(torch.cat([p["advantage_norm"] for p in applied], dim=1), whole["advantage_norm"])
    assert all(same_bits(p["moments"], whole["moments"]) for p in applied)
    assert whole["moments"][0] == float(whole["valid"].sum()) and 0 < whole["valid"].sum() < 7 * 769


def test_a_batch_with_every_step_skipped():
    x = draw(np.random.default_rng(9), 4, 300)
    x["terminated"][:] = True
    got = torch_gae(**x, prev_done=np.ones(300, bool))
    assert got["moments"].tolist() == [0.0, 0.0, 0.0] and not got["partials"].any()
    assert not got["advantage_norm"].any() and not got["advantage"].any() and not got["valid"].any()
    assert same_bits(got["returns"], x["value"])
    assert not any(bool(torch.isnan(t.to(torch.float64)).any()) for t in got.values())


def test_nothing_that_is_passed_in_is_modified():
    x = draw(np.random.default_rng(10), 5, 30)
    prev, parts = np.ones(30, np.uint8), np.full((1, 3), 7.0)
    before = {k: v.copy() for k, v in x.items()}
    torch_gae(**x, prev_done=prev, partials=parts)
    assert all(same_bits(x[k], before[k]) for k in x) and prev.all() and (parts == 7.0).all()


# ------------------------------------------------------------------------------------------------ the buffer, host path
T_ROLL = 4


def _rollouts(vec, buffers, count, seed=11, stop_after=None):
    """Drives ``vec`` for ``count`` rollouts of T_ROLL steps with seeded values, adding every step to every buffer.  Returns the
    steps as they were handed out and every `finish`'s results (cloned) per buffer."""
    gen = torch.Generator().manual_seed(seed)
    obs, _ = vec.reset(seed=seed)
    vec.env.state.workpiece_position = torch.linspace(10.5, 14.0, vec.num_envs, dtype=torch.float64)
    vec.env.state.wire_position = 10.0
    action = vec.env.make_action(0.1, 80.0, 9, 3.0, 30.0)
    steps, results = [], [[] for _ in buffers]
    for k in range(count * T_ROLL):
        value = torch.randn(vec.num_envs, generator=gen)
        nxt, reward, term, trunc, _ = vec.step(action)
        steps.append(dict(obs=obs.clone(), value=value, reward=reward.clone(), terminated=term.clone(), truncated=trunc.clone()))
        for b in buffers:
            b.add(obs, action, value, reward, term, trunc, log_prob=-value)
        obs = nxt
        if stop_after is not None and k + 1 == stop_after:
            return steps, results
        if (k + 1) % T_ROLL == 0:
            last = torch.randn(vec.num_envs, generator=gen)
            steps[-1]["last_value"] = last
            for b, res in zip(buffers, results):
                res.append({name: t.clone() for name, t in b.finish(last).items()})
    return steps, results


def _vec(n=6, max_episode_steps=3000):   # three control intervals
    return WireEDMVectorEnv(make("cpu", n, "autoreset", "s13"), max_episode_steps=max_episode_steps)


def test_rollout_buffer_on_the_oracle_backend_equals_the_definition():
    vec = _vec()
    buf = RolloutBuffer(vec, T_ROLL, extras={"log_prob": torch.float32})
    assert buf._native is None
    steps, (results,) = _rollouts(vec, [buf], 2)
    prev = np.zeros(6, dtype=np.uint8)
    for k, got in enumerate(results):
        part = steps[k * T_ROLL: (k + 1) * T_ROLL]
        stack = lambda name: torch.stack([s[name] for s in part])
        want = torch_gae(stack("reward"), stack("value"), part[-1]["last_value"], stack("terminated"), stack("truncated"),
                         prev_done=prev)
        assert set(got) == {"advantage", "advantage_norm", "returns", "valid"}
        for name in ("advantage", "advantage_norm", "returns"):
            assert same_bits(got[name], want[name]), (k, name)
        assert got["valid"].dtype == torch.bool and torch.equal(got["valid"], want["valid"].bool())
        done = stack("terminated") | stack("truncated")
        before = torch.cat([torch.from_numpy(prev).bool()[None], done[:-1]])
        assert torch.equal(got["valid"], ~before)                              # 0 exactly at the steps after a done
        prev = want["prev_done_out"].numpy()
        assert torch.equal(torch.from_numpy(prev).bool(), done[-1])            # the next rollout's prev_done: the last done row
        if k == 1:  # the stored blocks are what reset / step returned (the second rollout's: the buffer's live blocks)
            for name in ("obs", "value", "reward", "terminated", "truncated"):
                assert same_bits(buf.stored[name], stack(name)), name
            assert same_bits(buf.stored["log_prob"], -stack("value"))
            assert same_bits(buf.stored["action.servo"], torch.full((T_ROLL, 6), 0.1, dtype=torch.float64))
            assert buf.stored["action.current_mode"].dtype == torch.int32 and bool((buf.stored["action.current_mode"] == 9).all())
    assert same_bits(buf.prev_done, prev)
    all_trunc = torch.stack([s["truncated"] for s in steps])
    assert all_trunc.any() and not all_trunc[0].any(), "a truncation falls inside a rollout"
    assert not all(bool(r["valid"].all()) for r in results), "a step after a done is skipped"
    # flat views and minibatches
    flat = buf.flat()
    assert flat["obs"].shape == (T_ROLL * 6, len(vec.obs_names)) and flat["obs"].data_ptr() == buf.stored["obs"].data_ptr()
    assert all(v.shape[0] == T_ROLL * 6 for v in flat.values()) and flat["valid"].dtype == torch.bool
    seen = torch.cat([mb["returns"] for mb in buf.minibatches(5, generator=torch.Generator().manual_seed(1))])
    assert seen.shape == (T_ROLL * 6,) and torch.equal(seen.sort().values, flat["returns"].sort().values)
    # reset forgets the done row
    buf.reset()
    assert not buf.prev_done.any() and buf._slot == 0


def test_a_state_dict_taken_mid_rollout_continues_to_the_same_bits():
    vec = _vec(max_episode_steps=4000)   # the first rollout's last step truncates
    a = RolloutBuffer(vec, T_ROLL, gamma=0.9, gae_lambda=0.8, extras={"log_prob": torch.float32})
    _, (first,) = _rollouts(vec, [a], 2, stop_after=T_ROLL + 2)               # one rollout and two steps of the second
    sd = a.state_dict()
    assert sd["slot"] == 2 and sd["stored"]["obs"].shape[0] == 2 and sd["settings"]["gamma"] == 0.9
    assert sd["prev_done"].any(), "the first rollout ended on a done row"
    b = RolloutBuffer(_vec(), T_ROLL, extras={"log_prob": torch.float32})
    b.load_state_dict(sd)
    assert b.settings() == a.settings() and b._slot == 2
    gen = torch.Generator().manual_seed(5)
    obs = torch.randn(6, len(vec.obs_names), generator=gen)
    action = vec.env.make_action(0.1, 80.0, 9, 3.0, 30.0)
    for _ in range(2):
        value, reward = torch.randn(6, generator=gen), torch.randn(6, generator=gen)
        term = torch.rand(6, generator=gen) < 0.3
        for buf in (a, b):
            buf.add(obs, action, value, reward, term, ~term & (reward > 0), log_prob=reward)
    last = torch.randn(6, generator=gen)
    ra, rb = a.finish(last), b.finish(last)
    assert all(same_bits(ra[k], rb[k]) for k in ra) and same_bits(a.prev_done, b.prev_done) and same_bits(a.moments, b.moments)
    assert all(same_bits(a.stored[k], b.stored[k]) for k in a.stored)
    with pytest.raises(ValueError, match="steps x"):
        RolloutBuffer(vec, T_ROLL + 1, extras={"log_prob": torch.float32}).load_state_dict(sd)


def test_misuse_is_refused():
    vec = _vec()
    D = len(vec.obs_names)
    buf = RolloutBuffer(vec, 2)
    obs, value, reward, flag = torch.zeros(6, D), torch.zeros(6), torch.zeros(6), torch.zeros(6, dtype=torch.bool)
    action = vec.env.make_action()
    with pytest.raises(ValueError, match="0 of 2"):
        buf.finish(value)
    for bad in (dict(obs=torch.zeros(6, D + 1)), dict(obs=obs.double()), dict(value=torch.zeros(5)), dict(reward=reward.double()),
                dict(terminated=flag.to(torch.uint8)), dict(truncated=torch.zeros(6, 1, dtype=torch.bool)),
                dict(value=torch.zeros(6, device="meta")), dict(value=[0.0] * 6)):
        with pytest.raises(ValueError):
            buf.add(**{**dict(obs=obs, action=action, value=value, reward=reward, terminated=flag, truncated=flag), **bad})
    with pytest.raises(ValueError, match="extras"):
        buf.add(obs, action, value, reward, flag, flag, log_prob=value)
    assert buf._slot == 0
    buf.add(obs, action, value, reward, flag, flag)
    with pytest.raises(ValueError, match="leaves"):
        buf.add(obs, {"servo": value}, value, reward, flag, flag)
    buf.add(obs, action, value, reward, flag, flag)
    with pytest.raises(ValueError, match="holds 2 steps"):
        buf.add(obs, action, value, reward, flag, flag)
    with pytest.raises(ValueError, match="last_value"):
        buf.finish(torch.zeros(6, dtype=torch.float64))
    buf.finish(value)
    with pytest.raises(ValueError):
        RolloutBuffer(vec, 0)
    with pytest.raises(ValueError):
        RolloutBuffer(vec, 2, gamma=math.nan)
    with pytest.raises(ValueError, match="taken"):
        RolloutBuffer(vec, 2, extras={"reward": torch.float32})
