"""The shaped reward (sparc_amd/reward.py) on the host side: the ABI mirror of ``wedm_reward_desc`` and the
export with its refusals (no device is needed), `reward_definition` on hand-worked cases and against a plain loop over
environments written here, and `ShapedReward` through the vector adapter on the CPU oracle backend (which has no ``reward``
and so runs the definition): against a formula written independently from the state rows, the accumulators against the
published rows, the in-kernel autoreset's restart position, ``autoreset=False``, the episode log's per-term sums, the
normaliser, and checkpoints."""
from __future__ import annotations

import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from sparc_amd import EpisodeLog, Normalizer, ShapedReward, WireEDMVectorEnv, _abi, _lib, reward_definition
from sparc_amd.reward import TERM_NAMES
from tests import _resume_common as rc
from tests import _snapshot_common as snap
from tests._reward_common import (ALL_ON, ALL_ZERO, GAP_FLOOR, POS_RESTART, TMAX_CEILING, Problem, ShapedStack, alone,
                                  differences, every_term, in_kernel_stack, shaped_env, stack_everything)

ROOT = Path(__file__).resolve().parent.parent
RW, F64, I8, PULSE, SIG = _abi.RW, _abi.F64, _abi.I8, _abi.PULSE, _abi.SIG
K = _abi.RW_COUNT


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_desc_struct_mirror_matches_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wedm_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(wedm_reward_desc));']
    for field, _ in _abi.RewardDesc._fields_:
        lines.append(f'  printf("{field} %zu\\n", offsetof(wedm_reward_desc, {field}));')
    lines += ['  printf("consts %d abi %d\\n", WEDM_RW_COUNT, WEDM_ABI_VERSION);',
              '  printf("terms %d %d %d %d %d %d %d %d %d %d\\n", WEDM_RW_PROGRESS, WEDM_RW_STEP, WEDM_RW_WIRE_BREAK, WEDM_RW_TARGET, '
              'WEDM_RW_SPARKS, WEDM_RW_SHORTS, WEDM_RW_SHORT_STEPS, WEDM_RW_ENERGY, WEDM_RW_GAP_BELOW, WEDM_RW_TMAX_ABOVE);',
              "  return 0;", "}"]
    src = tmp_path / "desc.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "desc"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                   check=True)
    out = dict(row.split(" ", 1) for row in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("size")) == C.sizeof(_abi.RewardDesc)
    assert out.pop("consts") == f"{_abi.RW_COUNT} abi 4"
    assert out.pop("terms") == " ".join(str(int(k)) for k in RW) == "0 1 2 3 4 5 6 7 8 9"
    assert [k.name.lower() for k in RW] == [n.replace("target_reached", "target") for n in TERM_NAMES]
    assert {k: int(v) for k, v in out.items()} == {f: getattr(_abi.RewardDesc, f).offset for f, _ in _abi.RewardDesc._fields_}


def test_the_call_is_exported_and_the_abi_version_stays():
    assert "wedm_reward" in _lib.EXPORTS and hasattr(_lib.HipBackend, "reward")
    L = _lib.load()
    assert L.wedm_reward is not None and L.wedm_abi_version() == _abi.ABI_VERSION == 4


def test_bad_arguments_are_refused_before_anything_is_launched():
    """Every pointer below is an address nobody owns: a call that launched would fault (and on a machine without a device,
    fail with WEDM_ERR_HIP); every case returns WEDM_ERR_BAD_ARG with a text."""
    L = _lib.load()
    A = 0x100000
    N, S = 100, 128
    at = dict(f64=A, i8=A + 0x10000, pulse=A + 0x20000, sig=A + 0x30000, pos_before=A + 0x40000, restart=A + 0x50000,
              mask=A + 0x60000, reward_out=A + 0x70000, terms_out=A + 0x80000)

    def desc(weights=ALL_ON, **kw):
        f = dict(at, stride=S, terms_stride=S, pos_restart=50.0, gap_floor=10.0, tmax_ceiling=500.0, num_envs=N)
        f.update(kw)
        d = _abi.RewardDesc(**f)
        d.weight[:] = weights
        return d

    def refused(d, what, text=None):
        assert L.wedm_reward(C.byref(d), None) == _abi.ERR_BAD_ARG, what
        got = (L.wedm_last_error(None) or b"").decode()
        assert got.startswith("wedm_reward: ") and (text is None or text in got), (what, got)

    assert L.wedm_reward(None, None) == _abi.ERR_BAD_ARG and L.wedm_last_error(None) == b"wedm_reward: null descriptor"
    for n in (0, -5):
        refused(desc(num_envs=n), f"num_envs {n}", "num_envs must be positive")
    refused(desc(stride=N - 1), "stride below num_envs", "stride smaller than num_envs")
    refused(desc(terms_stride=N - 1), "terms_stride below num_envs", "terms_stride smaller than num_envs")
    for bad in (math.nan, math.inf, -math.inf):
        for k in range(K):
            refused(desc(weights=tuple(bad if j == k else w for j, w in enumerate(ALL_ON))), f"weight {k} = {bad}", f"weight {k} is not finite")
        for name in ("pos_restart", "gap_floor", "tmax_ceiling"):
            refused(desc(**{name: bad}), f"{name} = {bad}", "is not finite")
    # a block that a nonzero weight needs: every term alone, each of its blocks NULL in turn
    needs = {RW.PROGRESS: ("f64", "pos_before"), RW.WIRE_BREAK: ("i8",), RW.TARGET: ("i8",), RW.SPARKS: ("pulse",), RW.SHORTS: ("pulse",),
             RW.SHORT_STEPS: ("pulse",), RW.ENERGY: ("sig",), RW.GAP_BELOW: ("sig",), RW.TMAX_ABOVE: ("sig",)}
    for k, blocks in needs.items():
        for name in blocks:
            refused(desc(weights=alone(k), **{name: None}), f"{k.name} without {name}", f"{name} is null or not aligned to its element")
    refused(desc(reward_out=None), "reward_out NULL", "reward_out is null or not aligned to its element")
    refused(desc(weights=ALL_ZERO, reward_out=None), "reward_out NULL with every weight zero")
    # alignment to the element
    for name, off in (("f64", 4), ("pulse", 2), ("sig", 4), ("pos_before", 4), ("reward_out", 2), ("terms_out", 4)):
        refused(desc(**{name: at[name] + off}), f"{name} misaligned", f"{name} is null or not aligned to its element")
    refused(desc(weights=ALL_ZERO, sig=at["sig"] + 1), "a block nobody reads is still aligned")
    # an output block over an input block: first and last byte that the call may touch
    refused(desc(reward_out=at["f64"] + 8 * N - 4), "reward_out's first word on the position row's last", "reward_out overlaps f64")
    refused(desc(reward_out=at["pos_before"] - 4 * N + 4), "reward_out's last word on pos_before's first", "reward_out overlaps pos_before")
    refused(desc(reward_out=(at["i8"] + int(I8.TARGET_REACHED) * S + N - 1) & ~3), "reward_out's first word on the target row's last byte", "overlaps i8")
    refused(desc(reward_out=at["pulse"] + 4 * (int(PULSE.SHORT_STEPS_ACC) * S + N - 1)), "reward_out on the pulse rows' last word", "overlaps pulse")
    refused(desc(terms_out=at["sig"] + 8 * (int(SIG.TMAX_PEAK_ACC) * S + N - 1)), "terms_out on the signal rows' last element", "terms_out overlaps sig")
    refused(desc(terms_out=at["restart"] - 8 * ((K - 1) * S + N) + 8), "terms_out's last element on restart's first", "terms_out overlaps restart")
    refused(desc(terms_out=at["mask"] + 96), "terms_out inside the mask", "terms_out overlaps mask")
    refused(desc(terms_out=at["reward_out"] + 4 * N - 8), "the outputs on one another", "terms_out overlaps reward_out")


# ------------------------------------------------------------------------------------------------ the definition, by hand
def blocks(n: int, stride=None):
    s = n if stride is None else stride
    return dict(f64=np.zeros((_abi.F64_COUNT, s)), i8=np.zeros((_abi.I8_COUNT, s), dtype=np.int8),
                pulse=np.zeros((_abi.PULSE_COUNT, s), dtype=np.int32), sig=np.zeros((_abi.SIG_COUNT, s)), pos_before=np.zeros(n))


def define(b, weights, n, restart=None, mask=None, gap_floor=10.0, tmax_ceiling=500.0, pos_restart=50.0, terms=True):
    reward = np.full(n, 77.0, dtype=np.float32)
    out = np.full((K, n), 77.0) if terms else None
    reward_definition(b.get("f64"), b.get("i8"), b.get("pulse"), b.get("sig"), b.get("pos_before"), restart, mask, reward, out,
                      weights=weights, pos_restart=pos_restart, gap_floor=gap_floor, tmax_ceiling=tmax_ceiling, num_envs=n)
    return reward, out


def bits(a) -> list:
    a = np.asarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).reshape(-1).tolist()


def test_a_zero_weight_reads_nothing():
    """NaN and inf sources under zero weights give +0.0 (never 0 * inf = NaN), and the blocks may be None."""
    n = 3
    b = blocks(n)
    b["f64"][F64.WORKPIECE_POS] = [np.nan, np.inf, -np.inf]
    b["pos_before"][:] = [np.inf, np.nan, 1.0]
    b["sig"][[SIG.ENERGY_ACC, SIG.GAP_MIN_ACC, SIG.TMAX_PEAK_ACC]] = np.nan
    b["sig"][SIG.SAMPLES_ACC] = np.inf
    reward, terms = define(b, ALL_ZERO, n)
    assert bits(reward) == [0] * n and bits(terms) == [0] * (K * n)
    reward, terms = define({}, ALL_ZERO, n)
    assert bits(reward) == [0] * n and bits(terms) == [0] * (K * n)
    # -0.0 is a zero weight too: the term is +0.0, not -0.0 * x
    reward, terms = define({}, (-0.0,) * K, n)
    assert bits(reward) == [0] * n and bits(terms) == [0] * (K * n)
    # the step term alone needs no block at all
    reward, terms = define({}, alone(RW.STEP), n)
    assert reward.tolist() == [np.float32(ALL_ON[RW.STEP])] * n and terms[RW.STEP].tolist() == [ALL_ON[RW.STEP]] * n
    with pytest.raises(ValueError, match="sig"):
        define({}, alone(RW.ENERGY), n)


def test_the_hinge_terms_guard_on_samples_and_fail_on_nan():
    n = 6
    b = blocks(n)
    #                         no sample: identities   one sample below / above   at the threshold   NaN extrema   NaN samples
    b["sig"][SIG.SAMPLES_ACC] = [0.0, 999.0, 999.0, 1.0, 5.0, np.nan]
    b["sig"][SIG.GAP_MIN_ACC] = [np.inf, 4.0, 12.0, 10.0, np.nan, 4.0]
    b["sig"][SIG.TMAX_PEAK_ACC] = [-np.inf, 650.0, 300.0, 500.0, np.nan, 650.0]
    w = tuple(-2.0 if k in (RW.GAP_BELOW, RW.TMAX_ABOVE) else 0.0 for k in range(K))
    reward, terms = define(b, w, n)
    assert terms[RW.GAP_BELOW].tolist() == [-0.0, -12.0, -0.0, -0.0, -0.0, -0.0]
    assert terms[RW.TMAX_ABOVE].tolist() == [-0.0, -300.0, -0.0, -0.0, -0.0, -0.0]
    assert reward.tolist() == [0.0, -312.0, 0.0, 0.0, 0.0, 0.0] and not np.isnan(terms).any()
    # SAMPLES_ACC == 0 with finite extrema left over: still nothing
    b["sig"][SIG.SAMPLES_ACC] = 0.0
    b["sig"][SIG.GAP_MIN_ACC] = 1.0
    b["sig"][SIG.TMAX_PEAK_ACC] = 900.0
    reward, terms = define(b, w, n)
    assert not reward.any() and not terms.any()


def test_the_additions_run_in_term_order():
    """Progress, step and wire break all have x = 1, so the weights are the terms.  1e16, 1, -1e16 in term order is
    (1e16 + 1) - 1e16 = 0: the 1 is lost.  Every other arrangement of the three weights is the left-to-right sum of that
    arrangement, and the arrangements do not all agree (1e16, -1e16, 1 gives 1)."""
    import itertools

    b = blocks(1)
    b["f64"][F64.WORKPIECE_POS] = 4.0
    b["pos_before"][:] = 3.0
    b["i8"][I8.WIRE_BROKEN] = 1
    seen = {}
    for order in itertools.permutations((1e16, 1.0, -1e16)):
        w = order + (0.0,) * (K - 3)
        reward, terms = define(b, w, 1)
        assert terms[:3, 0].tolist() == list(order)
        assert float(reward[0]) == (0.0 + order[0] + order[1]) + order[2], order
        seen[order] = float(reward[0])
    assert seen[(1e16, 1.0, -1e16)] == 0.0 and seen[(1e16, -1e16, 1.0)] == 1.0 and math.fsum((1e16, 1.0, -1e16)) == 1.0
    # with a term between them that is off: the order is that of the terms that are on
    w = (1e16, 0.0, 1.0, -1e16) + (0.0,) * (K - 4)
    b["i8"][I8.TARGET_REACHED] = -1
    assert float(define(b, w, 1)[0][0]) == 0.0


def test_the_sum_is_rounded_to_float32_once():
    """1 + 2^-24 + 2^-52 lies just above the tie between 1 and 1 + 2^-23 in float32: one rounding gives 1 + 2^-23; terms
    rounded to float32 on the way (or summed in float32) give 1.  1 + 2^-24 exactly is the tie and goes to the even 1."""
    b = blocks(2)
    b["f64"][F64.WORKPIECE_POS] = 1.0
    b["i8"][I8.WIRE_BROKEN] = [1, 0]
    w = (1.0, 2.0 ** -24, 2.0 ** -52) + (0.0,) * (K - 3)
    reward, terms = define(b, w, 2)
    assert terms[:3, 0].tolist() == [1.0, 2.0 ** -24, 2.0 ** -52] and terms[2, 1] == 0.0
    assert reward.dtype == np.float32 and reward.tolist() == [1.0 + 2.0 ** -23, 1.0]
    assert np.float32(np.float32(1.0) + np.float32(2.0 ** -24)) + np.float32(2.0 ** -52) == np.float32(1.0)


def test_a_frozen_environment_earns_nothing_and_restart_picks_pos_restart():
    n = 4
    b = blocks(n, stride=n + 3)
    b["f64"][F64.WORKPIECE_POS, :n] = [60.0, 60.0, np.nan, 60.0]
    b["pos_before"][:] = [58.0, 5000.0, 1.0, 5000.0]
    b["i8"][I8.WIRE_BROKEN, :n] = 1
    b["pulse"][PULSE.SPARK_ACC, :n] = 2 ** 31 - 1
    b["sig"][:, :n] = np.inf
    restart = np.array([0, 7, 0, 255], dtype=np.uint8)
    mask = np.array([1, 200, 0, 0], dtype=np.uint8)
    reward, terms = define(b, ALL_ON, n, restart=restart, mask=mask, pos_restart=50.0)
    assert terms[RW.PROGRESS].tolist() == [2.0, 10.0, 0.0, 0.0], "pos_before where restart is zero, pos_restart elsewhere"
    assert bits(reward[2:]) == [0, 0] and bits(terms[:, 2:]) == [0] * (2 * K), "not live: +0.0 whatever the rows hold"
    # the live ones: +inf energy and -inf temperature excess add up to a NaN, stored in its canonical form
    assert terms[RW.SPARKS, 0] == ALL_ON[RW.SPARKS] * (2 ** 31 - 1) and terms[RW.ENERGY, 0] == np.inf and terms[RW.TMAX_ABOVE, 0] == -np.inf
    assert bits(reward[:2]) == [0x7FC00000] * 2
    # without restart nobody takes pos_restart
    assert define(b, alone(RW.PROGRESS), n, mask=mask)[1][RW.PROGRESS].tolist() == [2.0, -4940.0, 0.0, 0.0]


def loop_call(p: Problem, buf: np.ndarray, weights) -> None:
    """The whole call on the blocks of ``buf``, one environment after the other in Python floats: written from the header's
    text, sharing nothing with `reward_definition`."""
    v = lambda name: p.view(buf, name)   # noqa: E731
    for e in range(p.N):
        live = not p.masked or v("mask")[e] != 0
        t = [0.0] * K
        if live:
            x = [None] * K
            if weights[0] != 0.0:
                p0 = POS_RESTART if p.restarts and v("restart")[e] != 0 else float(v("pos_before")[e])
                x[0] = float(v("f64")[F64.WORKPIECE_POS, e]) - p0
            x[1] = 1.0
            x[2] = 1.0 if v("i8")[I8.WIRE_BROKEN, e] != 0 else 0.0
            x[3] = 1.0 if v("i8")[I8.TARGET_REACHED, e] != 0 else 0.0
            x[4], x[5], x[6] = (float(int(v("pulse")[r, e])) for r in (PULSE.SPARK_ACC, PULSE.SHORT_ACC, PULSE.SHORT_STEPS_ACC))
            sig = v("sig")[:, e]
            x[7] = float(sig[SIG.ENERGY_ACC])
            has = float(sig[SIG.SAMPLES_ACC]) > 0
            gmin, peak = float(sig[SIG.GAP_MIN_ACC]), float(sig[SIG.TMAX_PEAK_ACC])
            x[8] = GAP_FLOOR - gmin if has and GAP_FLOOR > gmin else 0.0
            x[9] = peak - TMAX_CEILING if has and peak > TMAX_CEILING else 0.0
            r = 0.0
            for k in range(K):
                if weights[k] != 0.0:
                    t[k] = weights[k] * x[k]
                    r = r + t[k]
        else:
            r = 0.0
        v("reward_out")[e] = np.float32(r)
        if p.has_terms:
            v("terms_out")[:, e] = t


@pytest.mark.parametrize("N", [1, 64, 257, 1000])
def test_the_definition_against_a_plain_loop(N):
    rng = np.random.default_rng(N)
    for case in range(4):
        p = Problem(rng, N, pad=3 * (case % 2), terms_pad=3 * (case // 2), masked=case in (1, 2), restart=case in (0, 1),
                    terms=case != 3)
        for weights in (ALL_ON, ALL_ZERO, alone(RW.GAP_BELOW), tuple(rng.standard_normal(K) * (rng.random(K) < 0.6))):
            got, want = p.buf.copy(), p.buf.copy()
            p.define(got, weights)
            loop_call(p, want, weights)
            assert differences(p, got, want) == [], (N, case, weights)
            written = [name for name in p.layout if got[p.layout[name][0]: p.layout[name][0] + 8].tobytes() != p.buf[p.layout[name][0]: p.layout[name][0] + 8].tobytes()]
            assert set(written) <= {"reward_out", "terms_out"}
    # two shards in turn are the whole batch
    p = Problem(rng, 600, pad=5, terms_pad=2, masked=True, restart=True)
    whole, shards = p.buf.copy(), p.buf.copy()
    p.define(whole)
    for part in ((0, 256), (256, 344)):
        p.define(shards, part=part)
    assert differences(p, shards, whole) == []


# ------------------------------------------------------------------------------------------------ through the adapter
def host(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy().copy()


def formula(vec, rw: ShapedReward, before: np.ndarray, restarted, live) -> np.ndarray:
    """The shaped reward of the step that just ended, per environment in Python floats from the state rows."""
    st = vec.env.state
    f64, i8, pulse, sig = host(st.f64), host(st.i8), host(st.pulse), host(st.signal)
    w = rw.weights
    out = np.zeros((vec.num_envs, K + 1))
    for e in range(vec.num_envs):
        if live is not None and not live[e]:
            continue
        p0 = float(vec.env.config.initial_gap) if restarted is not None and restarted[e] else float(before[e])
        has = sig[SIG.SAMPLES_ACC, e] > 0
        gmin, peak = float(sig[SIG.GAP_MIN_ACC, e]), float(sig[SIG.TMAX_PEAK_ACC, e])
        x = [float(f64[F64.WORKPIECE_POS, e]) - p0, 1.0, float(i8[I8.WIRE_BROKEN, e] != 0), float(i8[I8.TARGET_REACHED, e] != 0),
             float(pulse[PULSE.SPARK_ACC, e]), float(pulse[PULSE.SHORT_ACC, e]), float(pulse[PULSE.SHORT_STEPS_ACC, e]),
             float(sig[SIG.ENERGY_ACC, e]), rw.gap_floor - gmin if has and rw.gap_floor > gmin else 0.0,
             peak - rw.tmax_ceiling if has and peak > rw.tmax_ceiling else 0.0]
        r = 0.0
        for k in range(K):
            out[e, k] = w[k] * x[k]
            r = r + out[e, k]
        out[e, K] = float(np.float32(r))
    return out


def test_the_adapter_hands_out_the_formula_of_the_accumulators_and_logs_every_term():
    """64 environments that reset in the kernel, every term on, a normaliser and a log, over six control steps: the reward and
    the terms against `formula`; the sparks term against SPARK_ACC and against observation column 8 (the published count,
    one interval late); the restart position; the normaliser's input; the log's per-term sums."""
    vec, log, action = in_kernel_stack("cpu", capacity=1024)
    rw, n = vec._shaped, vec.num_envs
    assert log._native is None and rw._native is None, "the oracle backends run the definitions"
    assert vec.obs_names[8] == "spark_pulses" and rw.term_names == TERM_NAMES and len(rw.weights) == K
    sums, recorded, late, restarts, raws, scaleds = np.zeros((n, K + 1)), [], 0, 0, [], []
    for step in range(6):
        before = host(vec.env.state.workpiece_position)
        restarted = host(vec._need_reset)
        _, scaled, term, trunc, info = vec.step(action)
        want = formula(vec, rw, before, restarted, None)
        raw, terms = host(info["raw_reward"]), host(info["reward_terms"])
        assert terms.shape == (K, n) and terms.dtype == np.float64 and raw.dtype == np.float32
        assert terms.T.tobytes() == want[:, :K].tobytes() and raw.tolist() == want[:, K].tolist(), step
        # the accumulators, not the publication
        acc, obs8 = host(vec.env.state.pulse)[PULSE.SPARK_ACC, :n], host(info["raw_observation"])[:, 8]
        assert np.array_equal(terms[RW.SPARKS], ALL_ON[RW.SPARKS] * acc.astype(np.float64))
        late += int((acc != obs8).sum()) if step >= 1 else 0
        # the restart position: an environment the launch restarted advanced from the initial gap
        restarts += int(restarted.sum())
        for e in np.flatnonzero(restarted):
            assert terms[RW.PROGRESS, e] == float(vec.env.state.workpiece_position[e]) - float(vec.env.config.initial_gap)
        raws.append(raw)
        scaleds.append((host(scaled), host(info["episode_stats"]["r"])))
        # what the log must hold
        sums[:, :K] += terms.T
        sums[:, K] += raw.astype(np.float64)
        for e in np.flatnonzero(host(term | trunc)):
            recorded.append((step + 1, e, sums[e].copy()))
            sums[e] = 0.0
    assert late > 0, "SPARK_ACC and the published count of the same step differ somewhere"
    assert restarts > 0, "the launch restarted somebody"
    rec = log.read()
    assert len(rec["env"]) == len(recorded) > n and rec["lost"] == 0
    names = [f"rw_{name}" for name in TERM_NAMES]
    assert [c for c in log.columns if c.startswith("rw_")] == names and log.columns.index("rw_progress") > log.columns.index("energy")
    by_key = {(int(s), int(e)): i for i, (s, e) in enumerate(zip(rec["stamp"], rec["env"]))}
    steps_seen = set()
    for stamp, e, want in recorded:
        i = by_key[(stamp, e)]
        got = np.array([rec[name][i] for name in names])
        assert got.tobytes() == want[:K].tobytes(), (stamp, e)
        assert rec["reward_sum"][i] == want[K]
        # the terms reproduce reward_sum to within the float32 rounding of each step's reward (half an ulp of float32 each)
        steps = int(rec["steps"][i])
        steps_seen.add(steps)
        bound = steps * 2.0 ** -24 * max(abs(want[:K]).sum(), 1.0) * 2
        assert abs(math.fsum(got) - rec["reward_sum"][i]) <= bound, (stamp, e, math.fsum(got), rec["reward_sum"][i])
    assert max(steps_seen) >= 2, "episodes of more than one control step"
    summary = log.summary(rec)
    assert all(summary[f"mean_{name}"] == float(np.mean(rec[name])) for name in names)
    vec.close()
    # the normaliser is fed the shaped reward: a twin whose reward is a callable handing out the same numbers scales alike
    feed = [torch.from_numpy(r) for r in raws]
    twin = WireEDMVectorEnv(shaped_env("cpu", n), max_episode_steps=3000, reward=lambda env, prev: feed.pop(0),
                            normalizer=Normalizer(gamma=0.9, clip_obs=5.0))
    twin.reset(seed=33)
    action = snap.scenario(twin.env, seed=77)
    for step, (scaled, returns) in enumerate(scaleds):
        _, got, _, _, info = twin.step(action)
        assert host(got).tobytes() == scaled.tobytes() and host(info["episode_stats"]["r"]).tobytes() == returns.tobytes(), step
        assert not np.array_equal(scaled, raws[step]), "the reward is scaled"
    twin.close()


def test_the_sparks_term_is_this_launchs_count_not_the_published_one():
    """Four environments at a sparking gap, three launches of one control interval: after the second, SPARK_ACC (this launch)
    and SPARK_LAST = observation column 8 (the launch before) differ, SAMPLES_ACC is 999 and SAMPLES_LAST 1001; the term
    follows SPARK_ACC."""
    env = shaped_env("cpu", 4, autoreset=False)
    vec = WireEDMVectorEnv(env, reward=ShapedReward(progress=0.0, sparks=1.0), autoreset=False)
    vec.reset(seed=5)
    env.state.workpiece_position = torch.full((4,), 25.0, dtype=torch.float64)
    env.state.wire_position = torch.full((4,), 10.0, dtype=torch.float64)
    action = env.make_action(0.0, 80.0, 9, 3.0, 30.0)
    seen = []
    for _ in range(3):
        obs, reward, _, _, info = vec.step(action)
        pulse, sig = host(env.state.pulse)[:, :4], host(env.state.signal)[:, :4]
        assert reward.tolist() == pulse[PULSE.SPARK_ACC].astype(np.float32).tolist()
        assert np.array_equal(host(info["reward_terms"])[RW.SPARKS], pulse[PULSE.SPARK_ACC].astype(np.float64))
        assert np.array_equal(host(obs)[:, 8], pulse[PULSE.SPARK_LAST].astype(np.float32))
        seen.append((pulse[PULSE.SPARK_ACC].copy(), pulse[PULSE.SPARK_LAST].copy(), sig[SIG.SAMPLES_ACC, 0], sig[SIG.SAMPLES_LAST, 0]))
    acc2, last2, samples_acc, samples_last = seen[1]
    assert (acc2 > 0).all() and not np.array_equal(acc2, last2), (acc2, last2)
    # what the second launch published is the first launch's count and the control sample's own pulse, if it had one
    assert ((last2 - seen[0][0] >= 0) & (last2 - seen[0][0] <= 1)).all() and (samples_acc, samples_last) == (999.0, 1001.0)
    assert not np.array_equal(host(reward), host(obs)[:, 8]), "the reward is not observation column 8"
    vec.close()


def test_with_autoreset_off_a_frozen_environment_earns_nothing():
    env = shaped_env("cpu", 30, autoreset=False)
    rw = every_term()
    vec = WireEDMVectorEnv(env, autoreset=False, max_episode_steps=2000, reward=rw)
    vec.reset(seed=3)
    action = snap.scenario(env, seed=4)
    frozen_steps = 0
    for step in range(4):
        before, frozen = host(env.state.workpiece_position), host(vec._need_reset)
        _, reward, term, trunc, info = vec.step(action)
        want = formula(vec, rw, before, None, ~frozen)
        assert host(info["reward_terms"]).T.tobytes() == want[:, :K].tobytes() and host(reward).tolist() == want[:, K].tolist()
        if frozen.any():
            assert host(reward)[frozen].view(np.uint32).tolist() == [0] * int(frozen.sum())
            assert not host(info["reward_terms"])[:, frozen].view(np.uint64).any()
            assert host(env.state.i8)[I8.WIRE_BROKEN, :30][frozen].any(), "a frozen environment whose rows would earn something"
            frozen_steps += 1
        assert "raw_reward" not in info
    assert frozen_steps >= 2
    vec.close()


def test_bind_refuses_terms_the_environment_does_not_keep():
    plain = snap.make("cpu", 4, "plain", "s13")
    with pytest.raises(ValueError, match="pulse_stats=True"):
        WireEDMVectorEnv(plain, reward=ShapedReward(sparks=0.1))
    with pytest.raises(ValueError, match="signal_stats=True"):
        WireEDMVectorEnv(plain, reward=ShapedReward(gap_below=(-1.0, 10.0)))
    pulse_only = snap.make("cpu", 4, "pulse", "s13")
    with pytest.raises(ValueError, match="energy"):
        WireEDMVectorEnv(pulse_only, reward=ShapedReward(shorts=-1.0, energy=1e-6))
    rw = ShapedReward(progress=1.0, step=-0.1, wire_break=-10.0, target_reached=5.0)
    vec = WireEDMVectorEnv(plain, reward=rw)   # no pulse or signal term: any environment serves
    vec.reset(seed=1)
    _, reward, _, _, info = vec.step(plain.make_action(0.0, 80.0, 9, 3.0, 30.0))
    assert reward.shape == (4,) and info["reward_terms"].shape == (K, 4) and (host(info["reward_terms"])[RW.STEP] == -0.1).all()
    with pytest.raises(ValueError, match="already serves"):
        WireEDMVectorEnv(pulse_only, reward=rw)
    for bad in (dict(progress=math.nan), dict(gap_below=(1.0, math.inf)), dict(tmax_above=(math.inf, 1.0))):
        with pytest.raises(ValueError, match="finite"):
            ShapedReward(**bad)
    for v in (vec, pulse_only):
        v.close()


# ------------------------------------------------------------------------------------------------ checkpoints
def test_a_mismatching_shaped_reward_is_refused_on_load():
    def adapter(rw, seed):
        vec = WireEDMVectorEnv(shaped_env("cpu", 6), max_episode_steps=3000, reward=rw, normalizer=Normalizer(), episode_log=EpisodeLog(32))
        vec.reset(seed=seed)
        action = snap.scenario(vec.env, seed=seed)
        vec.step(action)
        return vec

    src = adapter(every_term(), 3)
    sd = src.state_dict()
    assert sd["reward"] == "shaped" and sd["reward_weights"] == ALL_ON and sd["reward_gap_floor"] == GAP_FLOOR and sd["reward_tmax_ceiling"] == 320.0
    w = ALL_ON
    others = {
        "reward_weights": ShapedReward(w[0], w[1], w[2], w[3], w[4], w[5], w[6], 2e-6, (w[8], GAP_FLOOR), (w[9], 320.0)),
        "reward_gap_floor": ShapedReward(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], (w[8], GAP_FLOOR + 1.0), (w[9], 320.0)),
        "reward_tmax_ceiling": ShapedReward(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], (w[8], GAP_FLOOR), (w[9], 321.0)),
        "reward=": "progress",
    }
    for word, rw in others.items():
        dst = adapter(rw, 4)
        before = rc.vec_everything(dst)
        with pytest.raises(ValueError, match=word):
            dst.load_state_dict(sd)
        rc.assert_equal(rc.vec_everything(dst), before, f"refused ({word}): the target changed")
        with pytest.raises(ValueError):
            src.load_state_dict(dst.state_dict())
        dst.close()
    same = adapter(every_term(), 4)
    same.load_state_dict(sd)
    rc.assert_equal(rc.vec_everything(same), rc.vec_everything(src), "an equal ShapedReward takes the dict")
    for v in (src, same):
        v.close()


def test_a_stack_with_a_shaped_reward_resumes_byte_for_byte_at_every_cut(tmp_path):
    """The in-kernel training stack with the `ShapedReward`, cut after every control step, saved, loaded into a fresh stack
    built with other seeds and dirtied by two steps of its own, and continued: everything it hands out and holds afterwards
    -- the log's ring and per-term accumulators included -- equals the uninterrupted run's on every byte."""
    st = ShapedStack("cpu", rc.RUN_SEEDS)
    steps, calls, paths = [], [], []
    for k in rc.CUTS:
        rc.run(st, k, steps, calls)
        paths.append(tmp_path / f"shaped-{k}.pt")
        rc.save(st, paths[-1])
    rc.run(st, rc.K, steps, calls)
    end = stack_everything(st)
    st.close()
    assert len(calls) == 4 and all(bool(c["stats"].isfinite().all()) for c in calls) and any(bool((c["grad"] != 0).any()) for c in calls)
    rewards = torch.stack([s["raw_reward"] for s in steps])
    assert len(set(rewards.reshape(-1).tolist())) > 64, "the rewards vary"
    for k in rc.CUTS:
        other = ShapedStack("cpu", rc.OTHER_SEEDS)
        try:
            rc.run(other, 2, [], [])
            rc.load(other, paths[k])
            got_steps, got_calls = [], []
            rc.run(other, rc.K, got_steps, got_calls)
            assert len(got_steps) == rc.K - k
            for i, (got, want) in enumerate(zip(got_steps, steps[k:])):
                rc.assert_equal(got, want, f"cut {k}: what control step {k + i + 1} handed out")
            want_calls = [c for c in calls if c["step"] >= k]
            assert [(c["step"], c["part"]) for c in got_calls] == [(c["step"], c["part"]) for c in want_calls]
            for got, want in zip(got_calls, want_calls):
                rc.assert_equal({n: got[n] for n in ("grad", "stats")}, {n: want[n] for n in ("grad", "stats")}, f"cut {k}")
            rc.assert_equal(stack_everything(other), end, f"cut {k}: everything after control step {rc.K}")
        finally:
            other.close()
