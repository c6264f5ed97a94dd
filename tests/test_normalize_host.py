"""Running normalisation (sparc_amd/normalize.py) on the host side: the ABI mirror of ``wedm_norm_desc``
and the export with its refusals (no device is needed), `torch_normalize` against exact rational arithmetic and against
hand-computed per-environment rows, the `Normalizer`'s checkpoints, and the vector adapter on the CPU oracle backend (which
has no ``normalize`` and so runs the host path)."""
from __future__ import annotations

import ctypes as C
import math
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

from sparc_amd import Normalizer, WireEDMVectorEnv, _abi, _lib
from sparc_amd.normalize import APPLY, REDUCE, ROW_NAMES, STEP, UPDATE, fresh_rows, fresh_stats, torch_normalize
from tests._normalize_common import COLUMN_KINDS, columns, same_bits
from tests._snapshot_common import make

ROOT = Path(__file__).resolve().parent.parent
U = 2.0 ** -53


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_desc_struct_mirror_matches_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wedm_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(wedm_norm_desc));', '  printf("plane_size %zu\\n", sizeof(wedm_norm_plane));']
    for field, _ in _abi.NormDesc._fields_:
        lines.append(f'  printf("{field} %zu\\n", offsetof(wedm_norm_desc, {field}));')
    for field, _ in _abi.NormPlane._fields_:
        lines.append(f'  printf("plane.{field} %zu\\n", offsetof(wedm_norm_plane, {field}));')
    lines += ['  printf("consts %d %d %d abi %d\\n", WEDM_NORM_MAX_COLUMNS, WEDM_NORM_MAX_TILES, WEDM_NORM_TILE, WEDM_ABI_VERSION);',
              '  printf("flagbits %d %d %d %d\\n", WEDM_NORM_UPDATE, WEDM_NORM_STEP, WEDM_NORM_REDUCE, WEDM_NORM_APPLY);',
              '  printf("moments %d %d %d %d\\n", WEDM_NM_COUNT, WEDM_NM_MEAN, WEDM_NM_M2, WEDM_NORM_MOMENTS);',
              "  return 0;", "}"]
    src = tmp_path / "desc.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "desc"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                   check=True)
    out = dict(row.split(" ", 1) for row in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("size")) == C.sizeof(_abi.NormDesc) and int(out.pop("plane_size")) == C.sizeof(_abi.NormPlane)
    assert out.pop("consts") == f"{_abi.NORM_MAX_COLUMNS} {_abi.NORM_MAX_TILES} {_abi.NORM_TILE} abi 4" == "160 4096 256 abi 4"
    assert out.pop("flagbits") == f"{UPDATE} {STEP} {REDUCE} {APPLY}" == "1 2 4 8"
    assert out.pop("moments") == f"{_abi.NM_COUNT} {_abi.NM_MEAN} {_abi.NM_M2} {_abi.NORM_MOMENTS}" == "0 1 2 3"
    want = {f: getattr(_abi.NormDesc, f).offset for f, _ in _abi.NormDesc._fields_}
    want.update({f"plane.{f}": getattr(_abi.NormPlane, f).offset for f, _ in _abi.NormPlane._fields_})
    assert {k: int(v) for k, v in out.items()} == want


def test_the_call_is_exported_and_the_abi_version_stays():
    assert "wedm_normalize" in _lib.EXPORTS
    L = _lib.load()
    assert L.wedm_normalize is not None and L.wedm_abi_version() == _abi.ABI_VERSION == 4


def test_bad_arguments_are_refused_before_anything_is_launched():
    """Every pointer below is an address nobody owns: a call that launched would fault (and on this machine, without a
    device, fail with WEDM_ERR_HIP); every case returns WEDM_ERR_BAD_ARG with a text."""
    L = _lib.load()
    A = 0x100000

    def desc(planes=((A, 8, 128), (A + 0x10000, 12, 192)), **kw):
        f = dict(reward=A + 0x20000, terminated=A + 0x21000, truncated=A + 0x22000, mask=None, skip=None,
                 obs_out=A + 0x30000, reward_out=A + 0x40000, ret=A + 0x41000, ep_return=A + 0x42000, last_return=A + 0x43000,
                 ep_length=A + 0x44000, last_length=A + 0x45000, ep_count=A + 0x46000, finished=A + 0x47000,
                 stats_in=A + 0x50000, stats_out=A + 0x51000, partials=A + 0x60000, tile_offset=0, n_tiles_total=1,
                 gamma=0.99, eps=1e-8, clip_obs=10.0, clip_reward=10.0, flags=UPDATE | STEP, num_envs=100)
        f.update(kw)
        d = _abi.NormDesc(**f)
        for k, (rows, n_rows, stride) in enumerate(planes):
            d.plane[k].rows, d.plane[k].n_rows, d.plane[k].stride = rows, n_rows, stride
        return d

    def refused(d, what):
        assert L.wedm_normalize(C.byref(d), None) == _abi.ERR_BAD_ARG, what
        assert b"wedm_normalize" in L.wedm_last_error(None), what

    assert L.wedm_normalize(None, None) == _abi.ERR_BAD_ARG and b"wedm_normalize" in L.wedm_last_error(None)
    # NULLs that the flags need
    for name in ("reward", "ret", "obs_out", "reward_out", "stats_in", "stats_out", "partials", "terminated", "truncated",
                 "ep_return", "last_return", "ep_length", "last_length", "ep_count", "finished"):
        refused(desc(**{name: None}), name)
    refused(desc(planes=((None, 8, 128), (A, 12, 192))), "plane 0 null")
    refused(desc(planes=((A, 8, 128), (None, 12, 192))), "plane 1 null")
    refused(desc(flags=UPDATE | REDUCE, partials=None), "REDUCE needs partials")
    refused(desc(flags=STEP | REDUCE, ret=None), "REDUCE with STEP needs ret")
    refused(desc(flags=APPLY, stats_out=None), "APPLY needs stats_out")
    # D outside [1, 159]
    refused(desc(planes=((A, 0, 128), (A, 0, 128))), "D = 0")
    refused(desc(planes=((A, 100, 128), (A, 60, 128))), "D = 160")
    refused(desc(planes=((A, -1, 128), (A, 5, 128))), "negative rows")
    # stride < num_envs
    refused(desc(planes=((A, 8, 99), (A, 12, 192))), "stride 0")
    refused(desc(planes=((A, 8, 128), (A, 12, 99))), "stride 1")
    # aliasing statistics: C = 21 columns, 3 * 21 * 8 = 504 bytes
    refused(desc(stats_out=A + 0x50000), "same block")
    refused(desc(stats_out=A + 0x50000 + 496), "overlap above")
    refused(desc(stats_out=A + 0x50000 - 496), "overlap below")
    # a tile range outside the workspace
    refused(desc(tile_offset=-1), "negative offset")
    refused(desc(tile_offset=1), "past the workspace")
    refused(desc(num_envs=257, planes=((A, 8, 300), (A, 12, 300))), "two tiles in a workspace of one")
    refused(desc(n_tiles_total=0), "no workspace")
    refused(desc(n_tiles_total=4097), "too many tiles")
    # num_envs < 1, flags
    refused(desc(num_envs=0), "num_envs 0")
    refused(desc(num_envs=-5), "num_envs negative")
    refused(desc(flags=16), "undefined flag")


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 4099])
def test_batch_moments_against_exact_rational_arithmetic(N):
    """The tree's mean and sum of squared deviations against `fractions.Fraction` on the same float32 values.  With
    u = 2^-53 and L = ceil(log2 N):  |m - exact| <= (L + 2) u max|x|  and  |S - exact| <= (L + 2) u (S + n max|x| std): one
    rounding per tree level plus a constant.  A single-pass E[x^2] - E[x]^2 misses the second by orders of magnitude in the
    1e6 + U(0, 8) and U(20000, 20001) columns."""
    rng = np.random.default_rng(100 + N)
    x = columns(rng, N)                                   # [D, N] float32
    mask = rng.random(N) >= 0.2
    mask[0] = True
    D = x.shape[0]
    block = np.zeros((D, N + 5), dtype=np.float32)
    block[:, :N] = x
    block[:, N:] = np.nan                                  # the padding columns reach nothing
    out = torch_normalize([block], N, np.zeros((3, D + 1)), mask=mask, flags=UPDATE)
    n, m, S = out["stats_out"].numpy()
    assert (n[D], m[D], S[D]) == (0.0, 0.0, 0.0)           # without STEP the return's column passes through
    L = math.ceil(math.log2(N)) if N > 1 else 0
    count = int(mask.sum())
    for c, kind in enumerate(COLUMN_KINDS):
        vals = [Fraction(float(v)) for v in x[c][mask]]
        mean = sum(vals) / count
        ssd = sum((v - mean) ** 2 for v in vals)
        big = float(np.abs(x[c][mask]).max())
        std = math.sqrt(float(ssd) / count)
        assert n[c] == count, kind
        err_m, err_S = abs(Fraction(float(m[c])) - mean), abs(Fraction(float(S[c])) - ssd)
        assert err_m <= (L + 2) * U * big, (kind, float(err_m) / (U * big))
        assert err_S <= Fraction((L + 2) * U) * (ssd + Fraction(count * big * std)), kind
        if kind == "constant":
            assert S[c] == 0.0 and m[c] == float(np.float32(293.15))


def test_the_tree_depends_on_values_and_indices_only():
    """Tiles: partials of a batch equal the partials of its halves at their tile offsets, and the fold of both equals the
    whole batch's statistics -- the property the shards rely on."""
    rng = np.random.default_rng(5)
    N, D = 700, 3
    x = rng.normal(size=(D, N)).astype(np.float32)
    s0 = fresh_stats(D + 1)
    whole = torch_normalize([x], N, s0, flags=UPDATE)
    a = torch_normalize([x[:, :512]], 512, s0, flags=UPDATE | REDUCE, tile_offset=0, n_tiles_total=3)
    b = torch_normalize([np.ascontiguousarray(x[:, 512:])], N - 512, s0, flags=UPDATE | REDUCE, tile_offset=2, n_tiles_total=3,
                        partials=a["partials"])
    assert same_bits(b["partials"], whole["partials"])
    c = torch_normalize([x[:, :512]], 512, s0, flags=UPDATE | APPLY, tile_offset=0, n_tiles_total=3, partials=b["partials"])
    assert same_bits(c["stats_out"], whole["stats_out"]) and same_bits(c["obs_out"], whole["obs_out"][:512])


def test_per_environment_rows_over_a_scripted_sequence():
    """Three environments, gamma 1/2 (every value exact): the discounted return, the episode latch, and a masked-out
    environment that keeps everything -- its ``finished`` flag included."""
    obs = np.zeros((1, 3), dtype=np.float32)
    rows = fresh_rows(3)
    stats = fresh_stats(2)
    kw = dict(gamma=0.5, eps=0.0, clip_obs=math.inf, clip_reward=math.inf)
    script = [  # reward, terminated, truncated, mask -> ret, ep_return, last_return, ep_length, last_length, ep_count, finished
        ([1, 2, 3], [0, 0, 0], [0, 0, 0], [1, 1, 0], ([1, 2, 0], [1, 2, 0], [0, 0, 0], [1, 1, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0])),
        ([2, 2, 2], [1, 0, 0], [0, 0, 1], [1, 1, 1], ([0, 3, 0], [0, 4, 0], [3, 0, 2], [0, 2, 0], [2, 0, 1], [1, 0, 1], [1, 0, 1])),
        ([4, 1, 1], [0, 0, 0], [0, 0, 0], [1, 0, 0], ([4, 3, 0], [4, 4, 0], [3, 0, 2], [1, 2, 0], [2, 0, 1], [1, 0, 1], [0, 0, 1])),
        ([1, 1, 1], [0, 1, 0], [0, 1, 0], None, ([3, 0, 1], [5, 0, 1], [3, 5, 2], [2, 0, 1], [2, 3, 1], [1, 1, 1], [0, 1, 0])),
    ]
    for k, (reward, term, trunc, mask, want) in enumerate(script):
        out = torch_normalize([obs], 3, stats, reward=np.array(reward, dtype=np.float32), terminated=np.array(term, dtype=bool),
                              truncated=np.array(trunc, dtype=bool), mask=None if mask is None else np.array(mask, dtype=bool),
                              rows=rows, **kw)
        for name, w in zip(ROW_NAMES, want):
            assert out[name].tolist() == w, (k, name)
            assert out[name].dtype == torch.from_numpy(rows[name]).dtype
        if k == 0:  # the return's column: the leaves 1 and 2 (environment 2 is masked out), merged into the fresh statistics
            n = 1e-4 + 2.0
            m = 0.0 + 1.5 * (2.0 / n)
            S = 1e-4 + 0.5 + 1.5 * 1.5 * (1e-4 * 2.0 / n)
            assert out["stats_out"][:, 1].tolist() == [n, m, S]
            assert out["reward_out"].tolist() == [float(np.float32(r / math.sqrt(S / n))) for r in (1.0, 2.0, 3.0)]
        rows = {name: out[name].numpy() for name in ROW_NAMES}
        stats = out["stats_out"]


def test_evaluation_mode_uses_the_statistics_and_leaves_them():
    stats = np.array([[4.0, 4.0, 4.0], [10.0, 0.5, 1.0], [16.0, 4.0, 36.0]])   # var 4, 1, 9
    obs = np.array([[13.0, 100.0, 8.0], [1.0, 0.0, 1.0]], dtype=np.float32)
    rows = fresh_rows(3)
    out = torch_normalize([obs], 3, stats, reward=np.array([6.0, -60.0, 0.0], dtype=np.float32), terminated=np.zeros(3, bool),
                          truncated=np.zeros(3, bool), skip=np.array([0, 1], dtype=np.uint8), rows=rows, gamma=0.5, eps=0.0,
                          clip_obs=10.0, clip_reward=10.0, flags=STEP)
    assert same_bits(out["stats_out"], torch.from_numpy(stats))
    assert out["obs_out"].tolist() == [[1.5, 1.0], [10.0, 0.0], [-1.0, 1.0]]      # (x - 10) / 2 clipped at 10; column 1 as it is
    assert out["reward_out"].tolist() == [2.0, -10.0, 0.0]                          # r / 3 clipped at 10
    assert out["ret"].tolist() == [6.0, -60.0, 0.0] and out["ep_length"].tolist() == [1, 1, 1]   # the rows go on
    assert not out["partials"].any()                                                  # no partial is written
    free = torch_normalize([obs], 3, stats, eps=0.0, clip_obs=math.inf, flags=0)
    assert free["obs_out"][1].tolist() == [45.0, -0.5] and "reward_out" not in free


# ------------------------------------------------------------------------------------------------ the Normalizer
def _vec(n=6, **kw):
    return WireEDMVectorEnv(make("cpu", n, "autoreset", "s13"), **kw)


def _drive(vec, steps=4, seed=11):
    """Environments at gaps that spark; returns what every call handed out."""
    obs, info = vec.reset(seed=seed)
    vec.env.state.workpiece_position = torch.linspace(10.5, 14.0, vec.num_envs, dtype=torch.float64)
    vec.env.state.wire_position = 10.0
    action = vec.env.make_action(0.1, 80.0, 9, 3.0, 30.0)
    outs = [(obs.clone(), info)]
    for _ in range(steps):
        o, r, te, tr, info = vec.step(action)
        outs.append((o.clone(), r.clone(), te.clone(), tr.clone(), info))
    return outs


def test_state_dict_round_trip_and_another_column_set_is_refused():
    a = Normalizer(gamma=0.9, clip_obs=5.0, skip=("spark_state", "voltage"))
    va = _vec(normalizer=a)
    _drive(va, 3)
    sd = a.state_dict()
    assert sd["columns"] == tuple(va.obs_names) + ("discounted_return",) and sd["stats"].shape == (3, len(va.obs_names) + 1)
    assert float(sd["stats"][0, 0]) == (((1e-4 + 6.0) + 6.0) + 6.0) + 6.0   # the reset's observation and three steps of six
    b = Normalizer()
    b.load_state_dict(sd)                               # before it serves an adapter: kept, checked at binding
    vb = _vec(normalizer=b)
    assert b.settings() == a.settings() and b.gamma == 0.9 and b.skip == ("spark_state", "voltage")
    back = b.state_dict()
    assert same_bits(back["stats"], sd["stats"]) and all(same_bits(back["rows"][k], sd["rows"][k]) for k in ROW_NAMES)
    assert same_bits(b.mean, a.mean) and same_bits(b.var, a.var) and same_bits(b.count, a.count)
    # both go on to the same bits
    vb.load_state_dict(va.state_dict())   # the environment, which environments are due for a reset, and the normaliser again
    oa, ob = (v.step(v.env.make_action(0.1, 80.0, 9, 3.0, 30.0)) for v in (va, vb))
    assert same_bits(oa[0], ob[0]) and same_bits(oa[1], ob[1]) and same_bits(a.stats, b.stats)
    other = Normalizer()
    WireEDMVectorEnv(make("cpu", 6, "autoreset", "s13"), normalizer=other, wire_profile_bins=2)
    with pytest.raises(ValueError, match="columns"):
        other.load_state_dict(sd)
    late = Normalizer()
    late.load_state_dict(sd)
    with pytest.raises(ValueError, match="columns"):
        WireEDMVectorEnv(make("cpu", 6, "autoreset", "s13"), normalizer=late, wire_profile_bins=2)
    with pytest.raises(ValueError, match="environments"):
        WireEDMVectorEnv(make("cpu", 7, "autoreset", "s13"), normalizer=_loaded(sd))


def _loaded(sd):
    n = Normalizer()
    n.load_state_dict(sd)
    return n


def test_train_and_eval_switch_the_update():
    n = Normalizer()
    vec = _vec(normalizer=n)
    _drive(vec, 2)
    before = n.stats.clone()
    assert n.eval() is n and not n.training
    vec.step(vec.env.make_action(0.1, 80.0, 9, 3.0, 30.0))
    assert same_bits(n.stats, before)
    n.train()
    vec.step(vec.env.make_action(0.1, 80.0, 9, 3.0, 30.0))
    assert float(n.count[0]) == float(before[0, 0]) + 6


# ------------------------------------------------------------------------------------------------ the adapter, host path
@pytest.mark.parametrize("bins", [None, 4])
def test_adapter_on_the_oracle_backend_equals_the_definition(bins):
    kw = {} if bins is None else dict(wire_profile_bins=bins)
    plain = _drive(_vec(**kw), 4)
    norm = Normalizer()
    vec = _vec(normalizer=norm, **kw)
    got = _drive(vec, 4)
    D = len(vec.obs_names)
    assert D == (8 if bins is None else 8 + 4 + 2 * bins)
    skip = np.array([n == "spark_state" for n in vec.obs_names], dtype=np.uint8)
    assert skip.sum() == 1
    stats, rows, seen = fresh_stats(D + 1), fresh_rows(6), []
    for k, (p, g) in enumerate(zip(plain, got)):
        raw = p[0].numpy()
        seen.append(raw.astype(np.float64))
        assert same_bits(g[-1]["raw_observation"], p[0])
        planes = [np.ascontiguousarray(raw.T)]
        if k == 0:
            want = torch_normalize(planes, 6, stats, skip=skip, flags=UPDATE)
        else:
            want = torch_normalize(planes, 6, stats, reward=p[1], terminated=p[2], truncated=p[3], skip=skip, rows=rows)
            assert same_bits(g[1], want["reward_out"]) and same_bits(g[4]["raw_reward"], p[1])
            assert torch.equal(g[2], p[2]) and torch.equal(g[3], p[3])
            assert torch.equal(g[4]["episode"], p[4]["episode"])                   # info["episode"] keeps its meaning
            es = g[4]["episode_stats"]
            rows = {name: want[name].numpy() for name in ROW_NAMES}
            assert set(es) == {"r", "l", "count", "finished"}
            if k == len(got) - 1:
                assert same_bits(es["r"], want["last_return"]) and same_bits(es["l"], want["last_length"])
                assert same_bits(es["count"], want["ep_count"]) and same_bits(es["finished"], want["finished"])
        assert same_bits(g[0], want["obs_out"]), k
        stats = want["stats_out"].numpy()
    assert same_bits(norm.stats, torch.from_numpy(stats))
    # ... and the definition's running moments are the moments of everything seen, with the prior of count 1e-4, mean 0, var 1
    allx = np.concatenate(seen, axis=0)
    total = allx.shape[0] + 1e-4
    mean = allx.sum(axis=0) / total
    var = (((allx - mean) ** 2).sum(axis=0) + 1e-4 * (1.0 + mean ** 2)) / total
    np.testing.assert_allclose(norm.mean[:D].numpy(), mean, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(norm.var[:D].numpy(), var, rtol=1e-9, atol=1e-300)
    assert float(norm.count[0]) == pytest.approx(total, rel=1e-14) and any(float(r.abs().sum()) > 0 for r in (p[1] for p in plain[1:]))


def test_without_a_normalizer_the_adapter_is_the_present_one():
    outs = _drive(_vec(), 3)
    assert all("episode_stats" not in o[-1] and "raw_observation" not in o[-1] for o in outs)
    env = make("cpu", 6, "autoreset", "s13")
    obs, _ = env.reset(seed=11)
    assert same_bits(outs[0][0], obs)
    env.state.workpiece_position = torch.linspace(10.5, 14.0, 6, dtype=torch.float64)
    env.state.wire_position = 10.0
    act = env.make_action(0.1, 80.0, 9, 3.0, 30.0)
    for o in outs[1:]:
        obs, reward, term, trunc, _ = env.step_control(act)
        assert same_bits(o[0], obs) and same_bits(o[1], reward) and torch.equal(o[2], term)


def test_frozen_environments_are_masked_out_and_a_masked_reset_zeroes_their_rows():
    n = Normalizer()
    vec = WireEDMVectorEnv(make("cpu", 6, "plain", "s13"), autoreset=False, reward="progress", normalizer=n)
    vec.reset(seed=3)
    vec.env.state.workpiece_position = torch.linspace(10.5, 14.0, 6, dtype=torch.float64)
    vec.env.state.wire_position = 10.0
    vec.env.state.target_position = torch.tensor([5000.0, 10.0, 5000.0, 5000.0, 10.0, 5000.0], dtype=torch.float64)
    act = vec.env.make_action(0.1, 80.0, 9, 3.0, 30.0)
    _, _, term, _, info = vec.step(act)
    assert term.tolist() == [False, True, False, False, True, False]
    assert info["episode_stats"]["finished"].tolist() == [0, 1, 0, 0, 1, 0] and info["episode_stats"]["l"].tolist() == [0, 1, 0, 0, 1, 0]
    count = float(n.count[0])
    vec.step(act)                                        # environments 1 and 4 are frozen: four leaves, their rows stay
    assert float(n.count[0]) == count + 4
    assert n.rows["finished"].tolist() == [0, 1, 0, 0, 1, 0] and n.rows["ep_length"].tolist() == [2, 0, 2, 2, 0, 2]
    stats = n.stats.clone()
    vec.reset(options={"mask": torch.tensor([False, True, False, False, False, False])})
    assert n.rows["finished"].tolist() == [0, 0, 0, 0, 1, 0] and n.rows["ep_count"].tolist() == [0, 0, 0, 0, 1, 0]
    assert n.rows["ep_length"].tolist() == [2, 0, 2, 2, 0, 2]
    assert float(n.count[0]) == float(stats[0, 0]) + 1   # the statistics stay, and take the one fresh observation
    src, dst = [0, 4], [2, 3]
    vec.fork(src, dst)
    for t in n.rows.values():
        assert t[2] == t[0] and t[3] == t[4]
