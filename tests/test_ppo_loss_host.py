"""PPO's loss (sparc_amd/ppo.py) on the host side: the ABI mirror of ``wedm_ppo_desc`` and the export
with its refusals (no device is needed), `ppo_loss_definition` against a float64 composition of ``torch.distributions`` and
the textbook loss with ``torch.autograd``'s gradients, hand-worked cases, the tree, and `PPOLoss` through `PolicyHead`,
`RolloutBuffer` and a small network on the CPU oracle backend (which has no ``ppo_loss`` and so runs the definition)."""
from __future__ import annotations

import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from sparc_amd import PolicyHead, PPOLoss, RolloutBuffer, WireEDMVectorEnv, _abi, _lib
from sparc_amd.policy_head import BACKWARD, SAMPLE, policy_head_definition
from sparc_amd.ppo import MAX_ROWS, STAT_NAMES, PPOStats, pairwise_sum, ppo_loss_definition
from tests._normalize_common import same_bits
from tests._policy_head_common import ALL_M, CONSTS, HI, LO, LOG_SPAN, MODES, random_params, zero_probability_rows
from tests._ppo_common import (CLIP, CLIP_VALUE, ENT_COEF, STORED, VALUE_KINDS, VF_COEF, definition_kw, draw_minibatch,
                                draw_partials, draw_wide_minibatch, lane_sequential_stats, left_to_right_stats, telling_partials, tile_tree,
                                tile_tree_stats)
from tests._snapshot_common import make

ROOT = Path(__file__).resolve().parent.parent
NAN64_BITS = 0x7FF8000000000000


# ------------------------------------------------------------------------------------------------ 1. the C-ABI
def test_desc_struct_mirror_matches_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wedm_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(wedm_ppo_desc));']
    for field, _ in _abi.PpoDesc._fields_:
        lines.append(f'  printf("{field} %zu\\n", offsetof(wedm_ppo_desc, {field}));')
    lines += ['  printf("consts %d %d %d %d abi %d\\n", WEDM_PPO_SUMS, WEDM_PPO_STATS, WEDM_PPO_COUNT_WORDS, WEDM_NORM_MAX_TILES, WEDM_ABI_VERSION);',
              '  printf("flagbits %d %d %d %d\\n", WEDM_PPO_CLIP_VALUE, WEDM_PPO_COUNT, WEDM_PPO_MAIN, WEDM_PPO_FOLD);',
              '  printf("sums %d %d %d %d %d %d %d\\n", WEDM_PS_LIVE, WEDM_PS_BAD, WEDM_PS_POLICY, WEDM_PS_VALUE, WEDM_PS_ENTROPY, WEDM_PS_KL, WEDM_PS_CLIPPED);',
              '  printf("statrows %d %d %d %d %d %d %d %d\\n", WEDM_PT_N, WEDM_PT_N_BAD, WEDM_PT_LOSS, WEDM_PT_POLICY, WEDM_PT_VALUE, WEDM_PT_ENTROPY, WEDM_PT_KL, WEDM_PT_CLIP_FRACTION);',
              "  return 0;", "}"]
    src = tmp_path / "desc.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "desc"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                   check=True)
    out = dict(row.split(" ", 1) for row in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("size")) == C.sizeof(_abi.PpoDesc)
    assert out.pop("consts") == f"{_abi.PPO_SUMS} {_abi.PPO_STATS} {_abi.PPO_COUNT_WORDS} {_abi.NORM_MAX_TILES} abi 4" == "7 8 2 4096 abi 4"
    assert out.pop("flagbits") == f"{_abi.PPO_CLIP_VALUE} {_abi.PPO_COUNT} {_abi.PPO_MAIN} {_abi.PPO_FOLD}" == "1 2 4 8"
    assert out.pop("sums") == "0 1 2 3 4 5 6"
    assert out.pop("statrows") == "0 1 2 3 4 5 6 7"
    assert STAT_NAMES == ("n", "n_bad", "loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction")
    assert {k: int(v) for k, v in out.items()} == {f: getattr(_abi.PpoDesc, f).offset for f, _ in _abi.PpoDesc._fields_}


def test_the_call_is_exported_and_the_abi_version_stays():
    assert "wedm_ppo_loss" in _lib.EXPORTS and hasattr(_lib.HipBackend, "ppo_loss")
    L = _lib.load()
    assert L.wedm_ppo_loss is not None and L.wedm_abi_version() == _abi.ABI_VERSION == 4


def test_bad_arguments_are_refused_before_anything_is_launched():
    """Every pointer below is an address nobody owns: a call that launched would fault (and on a machine without a device
    fail with WEDM_ERR_HIP); every case returns WEDM_ERR_BAD_ARG with a text."""
    L = _lib.load()
    A = 0x100000   # blocks 0x10000 apart: 100 rows of stride 20 are 8 000 bytes of float32
    names = ("params", "value", "index", "u", "mode_index", "old_log_prob", "advantage", "returns", "old_value", "valid",
             "grad_params", "grad_value", "partials", "stats", "count")
    at = {name: A + 0x10000 * i for i, name in enumerate(names)}

    def desc(**kw):
        f = dict(at, param_stride=20, grad_stride=20, rows=100, n_src=150, clip=0.2, vf_coef=0.5, ent_coef=0.01, clip_value=0.2,
                 n_modes=9, flags=_abi.PPO_CLIP_VALUE)
        arrays = {name: kw.pop(name) for name in ("lo", "hi", "log_span") if name in kw}
        f.update(kw)
        d = _abi.PpoDesc(**f)
        d.lo[:], d.hi[:], d.log_span[:] = LO, HI, LOG_SPAN
        for name, values in arrays.items():
            getattr(d, name)[:] = values
        return d

    def refused(d, what):
        assert L.wedm_ppo_loss(C.byref(d), None) == _abi.ERR_BAD_ARG, what
        text = L.wedm_last_error(None)
        assert text.startswith(b"wedm_ppo_loss: ") and len(text) > len(b"wedm_ppo_loss: "), what

    assert L.wedm_ppo_loss(None, None) == _abi.ERR_BAD_ARG and L.wedm_last_error(None).startswith(b"wedm_ppo_loss:")
    for flags in (16, -1, 1 << 30, _abi.PPO_MAIN | 32):
        refused(desc(flags=flags), ("flags", flags))
    for rows in (0, -5, _abi.NORM_MAX_TILES * 256 + 1, 2 ** 31 - 1):
        refused(desc(rows=rows), ("rows", rows))
    for n_src in (0, -1):
        refused(desc(n_src=n_src), ("n_src", n_src))
    for n_modes in (0, -1, _abi.HEAD_MAX_MODES + 1):
        refused(desc(n_modes=n_modes), ("n_modes", n_modes))
    refused(desc(param_stride=16), "param_stride below P")
    refused(desc(grad_stride=16), "grad_stride below P")
    for x in (math.nan, math.inf, -math.inf):
        for name in ("clip", "vf_coef", "ent_coef", "clip_value"):
            refused(desc(**{name: x}), (name, x))
        for name in ("lo", "hi", "log_span"):
            v = list(dict(lo=LO, hi=HI, log_span=LOG_SPAN)[name])
            v[1] = x
            refused(desc(**{name: v}), (name, x))
    refused(desc(clip=-0.1), "clip < 0")
    refused(desc(clip_value=-1e-9), "clip_value < 0")
    refused(desc(hi=[1.0, 200.0, 0.0, 100.0]), "hi == lo")
    refused(desc(hi=[-2.0, 200.0, 5.0, 100.0]), "hi < lo")
    # NULLs that a phase needs
    for name in ("params", "value", "u", "mode_index", "old_log_prob", "advantage", "returns", "old_value", "partials", "stats", "count"):
        refused(desc(**{name: None}), ("null", name))
    refused(desc(flags=_abi.PPO_MAIN | _abi.PPO_CLIP_VALUE, old_value=None), "old_value with CLIP_VALUE, MAIN alone")
    refused(desc(flags=_abi.PPO_COUNT, count=None), "count for COUNT")
    refused(desc(flags=_abi.PPO_COUNT, count=None, valid=None), "count for COUNT with an index alone")
    refused(desc(flags=_abi.PPO_MAIN, count=None, index=None), "count for MAIN with a mask alone")
    refused(desc(flags=_abi.PPO_FOLD, stats=None), "stats for FOLD")
    refused(desc(flags=_abi.PPO_FOLD, partials=None), "partials for FOLD")
    # misaligned pointers: to the element; u to 16 bytes; index, partials and stats to 8
    for name in ("params", "value", "mode_index", "old_log_prob", "advantage", "returns", "old_value", "grad_params", "grad_value", "count"):
        refused(desc(**{name: at[name] + 2}), ("misaligned", name))
    refused(desc(u=at["u"] + 8), "u to 16 bytes")
    for name in ("index", "partials", "stats"):
        refused(desc(**{name: at[name] + 4}), ("to 8 bytes", name))
    # an output block on an input block: the same address, its last element, the byte before its first
    last = (99 * 20 + 17) * 4
    refused(desc(grad_params=at["params"]), "grad_params on params")
    refused(desc(grad_params=at["value"] - last + 4), "grad_params' last element on value")
    refused(desc(grad_value=at["params"] + last - 4), "grad_value on params' last element")
    refused(desc(grad_value=at["index"] + 99 * 8), "grad_value on index's last element")
    refused(desc(stats=at["u"] + 149 * 16 + 8), "stats on u's last element")
    refused(desc(partials=at["mode_index"] + 149 * 4 - 4), "partials on mode_index's last elements")
    refused(desc(count=at["valid"] + 149 - 1), "count on valid's last elements")
    refused(desc(count=at["old_log_prob"]), "count on old_log_prob")
    refused(desc(grad_value=at["advantage"] + 149 * 4), "grad_value on advantage's last element")
    refused(desc(grad_value=at["returns"] - 99 * 4), "grad_value's last element on returns")
    refused(desc(grad_value=at["old_value"]), "grad_value on old_value")


# ------------------------------------------------------------------------------------------------ 2. an independent definition
def torch_reference(mb, M, clip_value):
    """The textbook loss in float64: ``torch.distributions`` (Normal -> Tanh -> Affine, Categorical) evaluated at the stored
    ``u`` (the transforms' caches hand ``u`` back, as in tests/test_policy_head_host.py), ``torch.minimum`` of the two
    surrogates, the value loss with the optional clipping of the common implementations, means weighted by ``valid``,
    gradients from autograd."""
    from torch.distributions import Categorical, Normal, TransformedDistribution
    from torch.distributions.transforms import AffineTransform, TanhTransform

    f64 = lambda a: torch.from_numpy(np.asarray(a).astype(np.float64))   # noqa: E731
    p = f64(mb["params"][:, : 8 + M]).requires_grad_(True)
    v = f64(mb["value"]).requires_grad_(True)
    lo, hi = torch.tensor(LO, dtype=torch.float64), torch.tensor(HI, dtype=torch.float64)
    base = Normal(p[:, 0:4], p[:, 4:8].exp())
    tanh, affine = TanhTransform(cache_size=1), AffineTransform((lo + hi) / 2, (hi - lo) / 2, cache_size=1)
    y = affine(tanh(f64(mb["u"])))
    cat = Categorical(logits=p[:, 8:])
    lp = TransformedDistribution(base, [tanh, affine]).log_prob(y).sum(1) + cat.log_prob(torch.from_numpy(mb["mode_index"].astype(np.int64)))
    ent = base.entropy().sum(1) + cat.entropy()
    old, A, R, ov, w = (f64(mb[k]) for k in ("old_log_prob", "advantage", "returns", "old_value", "valid"))
    ratio = torch.exp(lp - old)
    surrogate = -torch.minimum(ratio * A, torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP) * A)
    vl = (v - R) ** 2
    if clip_value:
        vl = torch.maximum(vl, (ov + torch.clamp(v - ov, -CLIP_VALUE, CLIP_VALUE) - R) ** 2)
    vl = 0.5 * vl
    n = w.sum()
    mean = lambda x: (x * w).sum() / n   # noqa: E731
    loss = mean(surrogate) + VF_COEF * mean(vl) - ENT_COEF * mean(ent)
    loss.backward()
    with torch.no_grad():
        stats = [n, torch.zeros(()), loss.detach(), mean(surrogate), mean(vl), mean(ent), mean((ratio - 1.0) - (lp - old)),
                 mean(((ratio - 1.0).abs() > CLIP).double())]
    return dict(stats=np.array([float(s) for s in stats]), grad_params=p.grad.numpy(), grad_value=v.grad.numpy(),
                ratio=ratio.detach().numpy(), lp=lp.detach().numpy(), ent=ent.detach().numpy())


def branches(mb, ref):
    """How often each branch of the loss occurs among the valid rows, and the rows that sit on a tie, by the reference alone."""
    ratio, A = ref["ratio"], mb["advantage"].astype(np.float64)
    v, ov, R = (mb[k].astype(np.float64) for k in ("value", "old_value", "returns"))
    ok = mb["valid"] != 0
    d = v - ov
    dc = np.clip(d, -CLIP_VALUE, CLIP_VALUE)
    vl, vlc = (v - R) ** 2, (ov + dc - R) ** 2
    side = np.where(ratio < 1.0 - CLIP, 0, np.where(ratio > 1.0 + CLIP, 2, 1))
    vside = np.where(d < -CLIP_VALUE, 0, np.where(d > CLIP_VALUE, 2, 1))
    count = {}
    for s, where in enumerate(("below", "inside", "above")):
        for sign in (-1, 1):
            count[f"ratio {where} the clip range, advantage {'+' if sign > 0 else '-'}"] = int((ok & (side == s) & (np.sign(A) == sign)).sum())
        if s != 1:
            count[f"value moved {where}, clipped loss larger"] = int((ok & (vside == s) & (vlc > vl)).sum())
            count[f"value moved {where}, clipped loss smaller"] = int((ok & (vside == s) & (vlc < vl)).sum())
    count["value moved inside the clip range"] = int((ok & (vside == 1)).sum())
    count["not valid"] = int((~ok).sum())
    # inside the value clip range vlc equals vl by construction (ov + (v - ov) is v exactly for float32 inputs in float64) and
    # both branches are the same function of v: a tie in the value term is a clipped row with vlc == vl
    tie = (np.abs(ratio - (1.0 - CLIP)) <= 1e-6) | (np.abs(ratio - (1.0 + CLIP)) <= 1e-6) | (np.abs(d) == CLIP_VALUE) | \
        ((vside != 1) & (vlc == vl)) | (A == 0.0)
    return count, tie


def drawn_without_ties(M, seed, rows=4096):
    """`draw_minibatch` with the rows on a tie drawn again (on the host, before either side runs) until none is left.  For
    M = 2 and 9 ``|u|`` stays below 9: torch's ``TanhTransform`` takes ``softplus(-2u)``, which torch replaces by its argument
    above 20, and that cut-off would be the largest discrepancy in ``log_prob`` here too."""
    rng = np.random.default_rng(seed)
    mb = draw_minibatch(rng, rows, M, u_limit=9.0 if M > 1 else 0.0)
    for _ in range(20):
        ref = torch_reference(mb, M, True)
        tie = branches(mb, ref)[1]
        if not tie.any():
            return mb
        value = mb["value"].astype(np.float64)
        fresh = {"old_log_prob": ref["lp"] + rng.uniform(-0.5, 0.5, rows), "advantage": rng.normal(size=rows),
                 "old_value": value + rng.uniform(-0.5, 0.5, rows), "returns": value + rng.normal(size=rows)}
        for name, a in fresh.items():
            mb[name] = np.where(tie, a.astype(np.float32), mb[name])
    raise AssertionError("rows on a tie remain after 20 redraws")


# the largest discrepancies seen on the inputs below, relative to 1 + the sum of the absolute summands; the
# bounds are 8 x these.  The means are compared as they are; the gradients as the gradient of the SUM (n x the gradient of
# the mean), so that the 1 of the scale does not hide a row's terms behind the 1 / n of the mean.  What is seen is the
# float32 rounding of lp that the definition takes on purpose (EVALUATE's stored value: half an ulp of a log_prob of up to
# 32 is 1e-6, and it reaches the ratio, the surrogate and the gradient undamped); entropy and value_loss do not pass
# through it: what was seen there is 1.1e-17 (value_loss), 1.3e-16 (entropy), 5.6e-17 (clip_fraction) and 0 (grad_value) --
# below one unit in the last place of the scale, which another order of torch's sums could move; there the figure is that
# unit, 2.2e-16, the precision of the format.
ULP = 2.2e-16
SEEN = dict(loss=9.44e-10, policy_loss=3.64e-09, value_loss=ULP, entropy=ULP, approx_kl=7.94e-11, clip_fraction=ULP,
            grad_params=8.65e-07, grad_value=ULP)


# the same in the wide regime (`draw_wide_minibatch` without hostile u, |u| < 9, old_log_prob moved by up to +-300 in every
# fourth row -- ratios from 1e-130 to 1e130, all finite in float64, which a reference needs --, advantages and returns from
# +-0 and 1e-41 to 1e30), largest over M in WIDE_M with and without value clipping; the bounds are 8 x these.  What is seen
# is again the float32 rounding of lp, now of a log_prob of up to 1600 in magnitude (half an ulp there is 6e-5): it reaches
# the ratio undamped, and a ratio of 1e130 times an advantage of 1e30 is the scale's largest summand itself.
# Seen: loss and policy_loss 1.00e-6 (M = 3), approx_kl 4.67e-7 (M = 4), grad_params 6.04e-5 (M = 8); value_loss 2.19e-16,
# entropy 8.8e-17, clip_fraction 0, grad_value 0, which do not pass through lp: one unit in the last place, as above.
WIDE_SEEN = dict(loss=1.00e-06, policy_loss=1.00e-06, value_loss=ULP, entropy=ULP, approx_kl=4.67e-07, clip_fraction=ULP,
                 grad_params=6.04e-05, grad_value=ULP)
WIDE_M = (2, 3, 4, 8, 12, 16, 19)


def against_the_torch_composition(M, clip_value, mb, ref):
    """The largest discrepancy of every statistic and of the two gradients between the definition and the reference ``ref``
    on the minibatch ``mb``, relative to 1 + the sum of the absolute summands."""
    out = ppo_loss_definition(**mb, **definition_kw(M, clip_value))
    assert np.array_equal(out["live"], mb["valid"] != 0) and out["stats"][0] == ref["stats"][0] and out["stats"][1] == 0
    side = lambda r: np.where(r < 1.0 - CLIP, 0, np.where(r > 1.0 + CLIP, 2, 1))   # noqa: E731
    assert np.array_equal(side(out["ratio"]), side(ref["ratio"])), "no row changes sides through the rounding of lp"
    assert np.isfinite(out["stats"]).all() and np.isfinite(ref["stats"]).all() and np.isfinite(ref["grad_params"]).all()
    # the scales: 1 + the absolute summands of each quantity
    w = (mb["valid"] != 0).astype(np.float64)
    n = w.sum()
    A, v, R, ov, old = (np.abs(mb[k].astype(np.float64)) for k in ("advantage", "value", "returns", "old_value", "old_log_prob"))
    ratio, lp, ent = ref["ratio"], np.abs(ref["lp"]), np.abs(ref["ent"])
    mean = lambda x: (x * w).sum() / n   # noqa: E731
    scale = dict(policy_loss=1 + mean(ratio * A), value_loss=1 + mean(0.5 * (v + R + 2 * ov) ** 2), entropy=1 + mean(ent),
                 approx_kl=1 + mean(ratio + 1 + lp + old), clip_fraction=2.0)
    scale["loss"] = scale["policy_loss"] + VF_COEF * scale["value_loss"] + ENT_COEF * scale["entropy"]
    worst = {name: abs(out["stats"][i] - ref["stats"][i]) / scale[name] for i, name in enumerate(STAT_NAMES) if name in scale}
    # the gradients of the sum, by the scales of DESIGN.md 4.17 with G = |A| ratio and E = ent_coef
    p = mb["params"].astype(np.float64)
    mu, ls, l = p[:, 0:4], p[:, 4:8], p[:, 8: 8 + M]
    z = (mb["u"].astype(np.float64) - mu) / np.exp(ls)
    m = l.max(1, keepdims=True)
    logp = l - m - np.log(np.exp(l - m).sum(1, keepdims=True))
    pj = np.exp(logp)
    H = -(pj * logp).sum(1, keepdims=True)
    G, E = (ratio * A)[:, None], ENT_COEF
    scale_gp = np.concatenate([1 + G * np.abs(z / np.exp(ls)), 1 + G * z * z + G + E, 1 + G * (1 + pj) + E * pj * (np.abs(logp) + np.abs(H))], axis=1)
    scale_gv = 1 + VF_COEF * (v + R + 2 * ov)
    worst["grad_params"] = (n * np.abs(out["grad_params64"] - ref["grad_params"]) / scale_gp).max()
    worst["grad_value"] = (n * np.abs(out["grad_value64"] - ref["grad_value"]) / scale_gv).max()
    print(M, clip_value, {k: float(f"{x:.3g}") for k, x in worst.items()})
    assert np.array_equal(out["grad_params"][~out["live"]], np.zeros((int((~out["live"]).sum()), 8 + M), np.float32))
    with np.errstate(over="ignore"):   # (the wide regime: a gradient of 1e160 is +-inf in float32, in both)
        assert same_bits(out["grad_params"], out["grad_params64"].astype(np.float32)) and same_bits(out["grad_value"], out["grad_value64"].astype(np.float32))
    return worst


@pytest.mark.parametrize("M", ALL_M)
@pytest.mark.parametrize("clip_value", [False, True])
def test_the_definition_against_a_float64_torch_composition(M, clip_value):
    mb = drawn_without_ties(M, 500 + M)
    ref = torch_reference(mb, M, clip_value)
    count, tie = branches(mb, ref)
    assert not tie.any()
    assert all(c >= 100 for c in count.values()), count
    worst = against_the_torch_composition(M, clip_value, mb, ref)
    for name, seen in SEEN.items():
        assert worst[name] <= 8 * seen, (name, worst[name])


@pytest.mark.parametrize("M", WIDE_M)
@pytest.mark.parametrize("clip_value", [False, True])
def test_the_definition_in_the_wide_regime_against_a_float64_torch_composition(M, clip_value):
    """Rows within the float32 rounding of lp of a clip bound (by the reference alone: |ratio - bound| <= 2^-22 (1 + |lp|))
    get the reference's log-probability as ``old_log_prob`` before either side runs: a ratio of 1, inside the range.  Rows
    that the value clip moves and whose two losses tie (a return of 1e30 absorbs ``value`` and ``old_value`` alike, so
    ``vlc == vl``: the header takes the unclipped branch, autograd's ``maximum`` halves the gradient between the two) get
    ``value`` as ``old_value``: inside the range, where both branches are one function -- the tie rule of `branches`."""
    rows = 4096
    mb = draw_wide_minibatch(np.random.default_rng(600 + M), rows, M, hostile_u=False, move=300.0, u_limit=9.0)
    ref = torch_reference(mb, M, clip_value)
    near = np.minimum(np.abs(ref["ratio"] - (1.0 - CLIP)), np.abs(ref["ratio"] - (1.0 + CLIP))) <= 2.0 ** -22 * (1.0 + np.abs(ref["lp"]))
    mb["old_log_prob"] = np.where(near, ref["lp"].astype(np.float32), mb["old_log_prob"])
    v, ov, R = (mb[k].astype(np.float64) for k in ("value", "old_value", "returns"))
    tied = (np.abs(v - ov) > CLIP_VALUE) & ((ov + np.clip(v - ov, -CLIP_VALUE, CLIP_VALUE) - R) ** 2 == (v - R) ** 2)
    assert tied.sum() >= 100
    mb["old_value"] = np.where(tied, mb["value"], mb["old_value"])
    ref = torch_reference(mb, M, clip_value)
    live = mb["valid"] != 0
    assert (live & (ref["ratio"] < 1e-100)).sum() >= 50 and (live & (ref["ratio"] > 1e100)).sum() >= 50
    assert zero_probability_rows(mb["params"], M).sum() >= 50
    kinds = np.arange(rows) % len(VALUE_KINDS)
    assert all((live & (kinds == i)).sum() >= 100 for i in range(len(VALUE_KINDS)))
    worst = against_the_torch_composition(M, clip_value, mb, ref)
    for name, seen in WIDE_SEEN.items():
        assert worst[name] <= 8 * seen, (name, worst[name])


# ------------------------------------------------------------------------------------------------ 3. hand-worked cases
def sampled(rows, M, seed):
    rng = np.random.default_rng(seed)
    params = random_params(rng, rows, M)
    s = policy_head_definition(SAMPLE, params, modes=MODES[M], seed=seed, t=3, **CONSTS)
    return dict(params=params, value=rng.normal(size=rows).astype(np.float32), u=s["u"], mode_index=s["mode_index"],
                old_log_prob=s["log_prob"], advantage=rng.normal(size=rows).astype(np.float32),
                returns=rng.normal(size=rows).astype(np.float32))


def test_at_the_sampling_parameters_the_ratio_is_exactly_one():
    rows, M = 500, 9
    mb = sampled(rows, M, 61)
    out = ppo_loss_definition(**mb, modes=MODES[M], **CONSTS, clip=0.2, vf_coef=0.0, ent_coef=0.0)
    assert np.all(out["ratio"] == 1.0) and not out["clipped"].any()
    st = dict(zip(STAT_NAMES, out["stats"]))
    assert st["n"] == rows and st["approx_kl"] == 0.0 and st["clip_fraction"] == 0.0
    want = policy_head_definition(BACKWARD, mb["params"], modes=MODES[M], u=mb["u"], mode_index=mb["mode_index"],
                                  g_log_prob=-mb["advantage"].astype(np.float64) * (1.0 / rows), **CONSTS)
    assert np.array_equal(out["grad_params"], want["grad_params"]) and np.abs(out["grad_params"]).max() > 0
    assert np.all(out["grad_value"] == 0.0)


def test_no_valid_row_gives_zeros_and_no_nan():
    mb = sampled(300, 2, 62)
    out = ppo_loss_definition(**mb, valid=np.zeros(300, np.uint8), modes=MODES[2], **CONSTS, clip=0.2, vf_coef=0.5, ent_coef=0.01)
    assert same_bits(out["stats"], np.zeros(8)) and same_bits(out["partials"], np.zeros((2, 7)))
    assert same_bits(out["grad_params"], np.zeros((300, 10), np.float32)) and same_bits(out["grad_value"], np.zeros(300, np.float32))
    assert out["count"].tolist() == [0, 0]


def test_without_coefficients_and_with_a_huge_clip_the_loss_is_minus_the_mean_of_ratio_times_advantage():
    rows, M = 1000, 2
    mb = draw_minibatch(np.random.default_rng(63), rows, M)
    valid = mb.pop("valid")
    out = ppo_loss_definition(**mb, valid=valid, modes=MODES[M], **CONSTS, clip=1e300, vf_coef=0.0, ent_coef=0.0)
    live = valid != 0
    want = -(out["ratio"] * mb["advantage"].astype(np.float64))[live].mean()
    assert abs(out["stats"][2] - want) <= 1e-13 * np.abs(out["ratio"] * mb["advantage"])[live].mean()
    assert out["stats"][2] == out["stats"][3] and out["stats"][7] == 0.0 and not out["clipped"].any()


def test_an_index_out_of_range_counts_as_bad_and_gets_a_zero_gradient():
    rows, M = 300, 9
    mb = draw_minibatch(np.random.default_rng(64), rows, M)
    index = np.arange(rows, dtype=np.int64)
    outside = {5: -1, 6: rows, 7: -2 ** 63, 8: 2 ** 62, 200: rows + 1}
    for r, i in outside.items():
        index[r] = i
    out = ppo_loss_definition(**mb, index=index, **definition_kw(M, True))
    inside = np.array([r not in outside for r in range(rows)])
    assert out["stats"][1] == len(outside) == out["count"][1] and out["stats"][0] == (inside & (mb["valid"] != 0)).sum() == out["count"][0]
    for r in outside:
        assert not out["live"][r] and not out["grad_params"][r].any() and out["grad_value"][r] == 0.0
    sub = ppo_loss_definition(**{k: (a[inside] if k in ("params", "value") else a) for k, a in mb.items()}, index=index[inside],
                              **definition_kw(M, True))
    assert np.array_equal(sub["grad_params"], out["grad_params"][inside]), "the other rows are the minibatch without the bad ones"
    assert np.allclose(sub["stats"][2:], out["stats"][2:], rtol=1e-12, atol=0)


def test_a_nan_advantage_reaches_the_statistics_as_the_canonical_nan():
    rows, M = 300, 2
    mb = draw_minibatch(np.random.default_rng(65), rows, M)
    mb["valid"][:] = 1
    mb["advantage"][17] = np.array([0xFFC12345], dtype=np.uint32).view(np.float32)[0]   # a negative NaN with a payload
    out = ppo_loss_definition(**mb, **definition_kw(M))
    bits = out["stats"].view(np.uint64)
    assert bits[2] == bits[3] == NAN64_BITS and np.isfinite(out["stats"][[0, 1, 4, 5, 6, 7]]).all()
    assert out["partials"].view(np.uint64)[0, 2] == NAN64_BITS and np.isfinite(out["partials"][1]).all()
    g = out["grad_params"].view(np.uint32)
    assert np.all(g[17] == 0x7FC00000) and np.isfinite(np.delete(out["grad_params"], 17, axis=0)).all()


# ------------------------------------------------------------------------------------------------ 4. the tree
def test_the_sums_are_the_pairwise_tree_over_the_row_number():
    rows, M = 300, 9
    mb = draw_minibatch(np.random.default_rng(66), rows, M)
    out = ppo_loss_definition(**mb, **definition_kw(M, True))
    leaves = np.zeros((512, 7))
    leaves[:rows] = out["summands"]

    def tree(x):
        return x[0] if len(x) == 1 else tree(x[: len(x) // 2]) + tree(x[len(x) // 2:])

    S = tree(leaves)
    s = 1.0 / S[0]
    pl, vl, en = S[2] * s, S[3] * s, S[4] * s
    want = np.array([S[0], S[1], (pl + VF_COEF * vl) - ENT_COEF * en, pl, vl, en, S[5] * s, S[6] * s])
    assert same_bits(out["stats"], want)
    assert same_bits(out["partials"], np.stack([tree(leaves[:256]), tree(leaves[256:])]))
    assert not same_bits(want[3:7], (out["summands"].sum(0) * s)[2:6]), "another order of the additions gives other bits"
    assert same_bits(pairwise_sum(out["summands"])[1], S)
    # the same rows through an index into a shuffled store: the tree is over r, not over src
    perm = np.random.default_rng(67).permutation(rows).astype(np.int64)
    store = {k: np.empty_like(mb[k]) for k in STORED}
    for k in STORED:
        store[k][perm] = mb[k]
    again = ppo_loss_definition(mb["params"], mb["value"], index=perm, **store, **definition_kw(M, True))
    assert all(same_bits(again[k], out[k]) for k in ("stats", "partials", "grad_params", "grad_value", "count"))
    # more tiles than one level: 5 tiles are padded to 8
    big = draw_minibatch(np.random.default_rng(68), 1100, 2)
    out = ppo_loss_definition(**big, **definition_kw(2))
    leaves = np.zeros((2048, 7))
    leaves[:1100] = out["summands"]
    assert same_bits(pairwise_sum(out["summands"])[1], tree(leaves))


@pytest.mark.parametrize("tiles", [3, 257, 513, 1025, 2049, 4096])
def test_the_recursive_tile_tree_equals_the_definitions(tiles):
    """`tests._ppo_common.tile_tree` (what tests/test_ppo_loss.py holds the fold kernel to where it runs alone) is the tree of
    `pairwise_sum` and of `ppo_loss_definition` in every class of tiles per fold lane: on the tile nodes of a minibatch
    whose last tile holds one row, and on a synthesised block of wide magnitudes laid out one leaf per tile.  The sums that
    add in another order are told apart from it by that block."""
    rows, M = 256 * (tiles - 1) + 1, 2
    mb = draw_minibatch(np.random.default_rng(tiles), rows, M)
    out = ppo_loss_definition(**mb, **definition_kw(M, True))
    nodes, root = pairwise_sum(out["summands"])
    assert nodes.shape == (tiles, 7) and same_bits(out["partials"], nodes) and np.isfinite(nodes).all()
    assert same_bits(tile_tree(nodes), root) and same_bits(tile_tree_stats(nodes), out["stats"])
    assert out["stats"][0] == out["count"][0] > 0 and out["partials"][-1][0] in (0.0, 1.0)
    if tiles == 3:   # ((a + b) + c) and ((a + b) + (c + 0)) are the same bits: no data tells them apart
        wide = draw_partials(np.random.default_rng(tiles), tiles)
        assert same_bits(tile_tree(wide), (wide[0] + wide[1]) + wide[2])
        return
    wide = telling_partials(tiles, seed=tiles)
    leaves = np.zeros((256 * tiles, 7))
    leaves[::256] = wide
    nodes, root = pairwise_sum(leaves)
    assert same_bits(nodes, wide) and same_bits(tile_tree(wide), root)
    assert not same_bits(left_to_right_stats(wide), tile_tree_stats(wide))
    assert same_bits(lane_sequential_stats(wide), tile_tree_stats(wide)) == (tiles <= 512), "two tiles per lane are one addition"


# ------------------------------------------------------------------------------------------------ 5. PPOLoss
def _vec(n=6):
    return WireEDMVectorEnv(make("cpu", n, "autoreset", "s13"), max_episode_steps=3000)


def _rollout(n=6, T=3, extras=True):
    vec = _vec(n)
    head = PolicyHead(vec, modes=(5, 9, 13), bounds={"servo": (-0.2, 0.4), "ON_time": (1.0, 4.0)}, seed=71)
    buf = RolloutBuffer(vec, T, extras={"log_prob": torch.float32} if extras else None)
    gen = torch.Generator().manual_seed(3)
    D, P = len(vec.obs_names), head.param_dim
    W, b = (0.1 * torch.randn(D, P + 1, generator=gen)).requires_grad_(True), torch.zeros(P + 1, requires_grad=True)

    def net(obs):
        out = torch.nan_to_num(obs) * 1e-3 @ W + b
        return out[:, :P], out[:, P]

    obs, _ = vec.reset(seed=6)
    vec.env.state.workpiece_position = torch.linspace(10.5, 14.0, n, dtype=torch.float64)
    vec.env.state.wire_position = 10.0
    with torch.no_grad():
        for _ in range(T):
            params, value = net(obs)
            out = head.sample(params.contiguous())
            nxt, reward, term, trunc, _ = vec.step(out.action)
            buf.add(obs, head.stored(out), value, reward, term, trunc, **({"log_prob": out.log_prob} if extras else {}))
            obs = nxt
        buf.finish(net(obs)[1])
        W += 0.05 * torch.randn(D, P + 1, generator=gen)
    return vec, head, buf, net, (W, b)


def test_ppo_loss_through_the_head_the_rollout_buffer_and_a_network_on_the_oracle_backend():
    vec, head, buf, net, (W, b) = _rollout()
    ppo = PPOLoss(head, clip=0.2, vf_coef=0.5, ent_coef=0.01, clip_value=0.3)
    assert ppo._native is None
    flat = buf.flat()
    idx = torch.randperm(18, generator=torch.Generator().manual_seed(4))[:11]
    stats = ppo.backward(*net(flat["obs"][idx]), rollout=buf, index=idx)
    assert isinstance(stats, PPOStats) and stats.tensor.dtype == torch.float64 and tuple(stats.tensor.shape) == (8,)
    assert float(stats.n) == float(flat["valid"][idx].sum()) > 0 and float(stats.n_bad) == 0 and math.isfinite(float(stats.loss))
    assert stats.as_dict()["loss"] == float(stats.loss) and list(stats.as_dict()) == list(STAT_NAMES)
    first, first_stats = (W.grad.clone(), b.grad.clone()), stats.tensor.clone()
    assert float(first[0].abs().sum()) > 0
    W.grad = b.grad = None
    gathered = dict(u=flat["action.u"][idx], mode_index=flat["action.mode_index"][idx], old_log_prob=flat["log_prob"][idx],
                    advantage=flat["advantage_norm"][idx], returns=flat["returns"][idx], old_value=flat["value"][idx], valid=flat["valid"][idx])
    stats = ppo.backward(*net(flat["obs"][idx]), **gathered)
    assert same_bits(W.grad, first[0]) and same_bits(b.grad, first[1]) and same_bits(stats.tensor, first_stats)
    W.grad = b.grad = None
    loss = ppo.loss(*net(flat["obs"][idx]), **gathered)
    assert loss.dtype == torch.float32 and loss.ndim == 0 and float(loss) == float(first_stats[2].to(torch.float32))
    loss.backward()
    assert same_bits(W.grad, first[0]) and same_bits(b.grad, first[1]), "an upstream gradient of 1 changes no bit"
    # on leaves, with something upstream: one float32 rounding of the scalar multiply
    params, value = (t.detach().clone().requires_grad_(True) for t in net(flat["obs"][idx]))
    (0.7 * ppo.loss(params, value, **gathered)).backward()
    B, P = params.shape
    gp, gv = ppo._grad[: B * P].view(B, P), ppo._grad[B * P: B * (P + 1)]
    assert same_bits(params.grad, gp * torch.tensor(0.7)) and same_bits(value.grad, gv * torch.tensor(0.7))
    stale = ppo.loss(params, value, **gathered)
    ppo.backward(params, value, **gathered)
    with pytest.raises(RuntimeError, match="overwritten"):
        stale.backward()
    # checkpoints
    sd = ppo.state_dict()
    assert sd == {"clip": 0.2, "vf_coef": 0.5, "ent_coef": 0.01, "clip_value": 0.3}
    other = PPOLoss(head)
    assert other.state_dict() == {"clip": 0.2, "vf_coef": 0.5, "ent_coef": 0.0, "clip_value": None}
    other.load_state_dict(sd)
    assert other.state_dict() == sd
    assert same_bits(other.backward(params, value, **gathered).tensor, ppo.stats.tensor)


def test_misuse_is_refused():
    vec, head, buf, net, _ = _rollout()
    ppo = PPOLoss(head, clip_value=0.2)
    flat = buf.flat()
    idx = torch.arange(18)
    params, value = (t.detach().contiguous() for t in net(flat["obs"]))
    good = dict(u=flat["action.u"], mode_index=flat["action.mode_index"], old_log_prob=flat["log_prob"], advantage=flat["advantage"],
                returns=flat["returns"], old_value=flat["value"])
    ppo.backward(params.clone().requires_grad_(True), value, **good)
    for bad in (params.double(), params[:, :-1], params.numpy()):
        with pytest.raises(ValueError, match="params"):
            ppo.backward(bad, value, **good)
    with pytest.raises(ValueError, match="value"):
        ppo.backward(params, value[:-1], **good)
    with pytest.raises(ValueError, match="value"):
        ppo.backward(params, value.double(), **good)
    for name, bad in (("u", flat["action.u"][:, :3]), ("old_log_prob", flat["log_prob"].double()), ("advantage", flat["advantage"][:5]),
                      ("mode_index", flat["action.mode_index"].float()), ("valid", flat["valid"].float())):
        with pytest.raises(ValueError, match=name):
            ppo.backward(params, value, **{**good, name: bad})
    with pytest.raises(ValueError, match="lies on"):
        ppo.backward(params, value, **{**good, "returns": flat["returns"].to("meta")})
    with pytest.raises(ValueError, match="old_value"):
        ppo.backward(params, value, **{**good, "old_value": None})
    with pytest.raises(ValueError, match="at most 1048576 rows"):
        ppo.backward(torch.zeros(MAX_ROWS + 1, head.param_dim), value, **good)
    with pytest.raises(ValueError, match="index"):
        ppo.backward(params, value, rollout=buf)
    with pytest.raises(ValueError, match="index"):
        ppo.backward(params, value, rollout=buf, index=idx.to(torch.int32))
    with pytest.raises(ValueError, match="index"):
        ppo.backward(params, value, index=idx, **good)
    with pytest.raises(ValueError, match="rollout"):
        ppo.backward(params, value, rollout=buf, index=idx, u=flat["action.u"])
    bare = _rollout(extras=False)[2]
    with pytest.raises(ValueError, match="log_prob"):
        ppo.backward(params, value, rollout=bare, index=idx)
    for kw in (dict(clip=-0.1), dict(clip=math.nan), dict(vf_coef=math.inf), dict(ent_coef=math.nan), dict(clip_value=-1.0)):
        with pytest.raises(ValueError):
            PPOLoss(head, **kw)
    with pytest.raises(ValueError, match="at most"):
        ppo_loss_definition(np.zeros((MAX_ROWS + 1, 9), np.float32), np.zeros(MAX_ROWS + 1, np.float32), modes=MODES[1], **CONSTS,
                            **{k: np.zeros(1, np.float32) for k in ("old_log_prob", "advantage", "returns")},
                            u=np.zeros((1, 4), np.float32), mode_index=np.zeros(1, np.int32))
