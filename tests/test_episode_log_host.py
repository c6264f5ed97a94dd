"""The episode log (sparc_amd/episode_log.py) on the host side: the ABI mirror of ``wedm_elog_desc`` and
the export with its refusals (no device is needed), `episode_log_definition` against a plain loop over environments written
here, the phases and the shards, and `EpisodeLog` through the vector adapter on the CPU oracle backends (which have no
``episode_log`` and so run the definition): against an independent host scan of what every step handed out, with
``autoreset=False``, across `reset`, `fork` and checkpoints."""
from __future__ import annotations

import ctypes as C
import io
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from sparc_amd import EpisodeLog, Normalizer, WireEDMVectorEnv, _abi, _lib
from sparc_amd.core import env_params as envp
from sparc_amd.episode_log import COMMIT, COUNT, LAST, SCATTER, SUM_F32, SUM_F64, SUM_I32
from tests import _snapshot_common as snap
from tests._resume_common import assert_equal, vec_everything
from tests._episode_log_common import (CAPS, DRAWS, SPEC, SPEC_MAX, SPEC_SHARD, WHERE, WORKSPACES, Problem, differences, finishing,
                                        flags_from, full_stack, shard_case)

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_desc_struct_mirror_matches_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wedm_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(wedm_elog_desc));', '  printf("plane_size %zu\\n", sizeof(wedm_elog_plane));']
    for field, _ in _abi.ElogDesc._fields_:
        lines.append(f'  printf("{field} %zu\\n", offsetof(wedm_elog_desc, {field}));')
    for field, _ in _abi.ElogPlane._fields_:
        lines.append(f'  printf("plane.{field} %zu\\n", offsetof(wedm_elog_plane, {field}));')
    lines += ['  printf("consts %d %d abi %d\\n", WEDM_ELOG_MAX_PLANES, WEDM_ELOG_MAX_ROWS, WEDM_ABI_VERSION);',
              '  printf("kinds %d %d %d %d\\n", WEDM_ELOG_LAST, WEDM_ELOG_SUM_F32, WEDM_ELOG_SUM_F64, WEDM_ELOG_SUM_I32);',
              '  printf("flagbits %d %d %d\\n", WEDM_ELOG_COUNT, WEDM_ELOG_SCATTER, WEDM_ELOG_COMMIT);', "  return 0;", "}"]
    src = tmp_path / "desc.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "desc"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                   check=True)
    out = dict(row.split(" ", 1) for row in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("size")) == C.sizeof(_abi.ElogDesc) and int(out.pop("plane_size")) == C.sizeof(_abi.ElogPlane)
    assert out.pop("consts") == f"{_abi.ELOG_MAX_PLANES} {_abi.ELOG_MAX_ROWS} abi 4"
    assert _abi.ELOG_MAX_PLANES >= 32 and _abi.ELOG_MAX_ROWS >= 64
    assert out.pop("kinds") == f"{LAST} {SUM_F32} {SUM_F64} {SUM_I32}" == "0 1 2 3"
    assert out.pop("flagbits") == f"{COUNT} {SCATTER} {COMMIT}" == "1 2 4"
    want = {f: getattr(_abi.ElogDesc, f).offset for f, _ in _abi.ElogDesc._fields_}
    want.update({f"plane.{f}": getattr(_abi.ElogPlane, f).offset for f, _ in _abi.ElogPlane._fields_})
    assert {k: int(v) for k, v in out.items()} == want


def test_the_call_is_exported_and_the_abi_version_stays():
    assert "wedm_episode_log" in _lib.EXPORTS
    L = _lib.load()
    assert L.wedm_episode_log is not None and L.wedm_abi_version() == _abi.ABI_VERSION == 4


def test_bad_arguments_are_refused_before_anything_is_launched():
    """Every pointer below is an address nobody owns: a call that launched would fault (and on a machine without a device,
    fail with WEDM_ERR_HIP); every case returns WEDM_ERR_BAD_ARG with a text."""
    L = _lib.load()
    A = 0x100000
    default = ((LAST, 1, 2), (LAST, 4, 3), (LAST, 8, 1), (SUM_F32, 4, 2), (SUM_F64, 8, 1), (SUM_I32, 4, 1))

    def desc(planes=default, edit=None, **kw):
        f = dict(terminated=A + 0x1000, truncated=A + 0x2000, mask=A + 0x3000, env_out=A + 0x10000, stamp_out=A + 0x20000,
                 head=A + 0x30000, tile_counts=A + 0x31000, capacity=64, env_id_offset=0, stamp=1, n_planes=len(planes),
                 num_envs=100, tile_offset=0, n_tiles_total=1, flags=0)
        f.update(kw)
        d = _abi.ElogDesc(**f)
        for p, (kind, eb, rows) in enumerate(planes):
            q = d.plane[p]
            q.src, q.dst, q.acc = A + 0x100000 * (p + 1), A + 0x100000 * (p + 1) + 0x40000, A + 0x100000 * (p + 1) + 0x80000
            q.src_stride, q.n_rows, q.elem_bytes, q.kind = 128, rows, eb, kind
        if edit:
            edit(d)
        return d

    def refused(d, what):
        assert L.wedm_episode_log(C.byref(d), None) == _abi.ERR_BAD_ARG, what
        assert b"wedm_episode_log" in L.wedm_last_error(None), what

    def plane(p, **kw):
        def edit(d):
            for k, v in kw.items():
                setattr(d.plane[p], k, v)
        return edit

    assert L.wedm_episode_log(None, None) == _abi.ERR_BAD_ARG and b"wedm_episode_log" in L.wedm_last_error(None)
    # needed pointers: NULL, or misaligned to their element
    for name in ("terminated", "env_out", "stamp_out", "head", "tile_counts"):
        refused(desc(**{name: None}), name)
    for name, off in (("env_out", 4), ("stamp_out", 4), ("head", 4), ("tile_counts", 2)):
        refused(desc(**{name: A + 0x10000 * (3 + len(name)) + off}), name + " misaligned")
    refused(desc(flags=COUNT, terminated=None), "COUNT needs terminated")
    refused(desc(flags=COMMIT, head=None), "COMMIT needs head")
    refused(desc(flags=COMMIT, tile_counts=None), "COMMIT needs tile_counts")
    for p, (kind, eb, _) in enumerate(default):
        refused(desc(edit=plane(p, src=None)), f"plane {p} src null")
        refused(desc(edit=plane(p, dst=None)), f"plane {p} dst null")
        if eb > 1:
            refused(desc(edit=plane(p, src=A + 0x100000 * (p + 1) + eb // 2)), f"plane {p} src misaligned")
        if kind != LAST:
            refused(desc(edit=plane(p, acc=None)), f"plane {p}: a sum without an accumulator")
            refused(desc(edit=plane(p, acc=A + 4)), f"plane {p}: acc misaligned")
            refused(desc(edit=plane(p, dst=A + 0x100000 * (p + 1) + 0x40004)), f"plane {p}: a sum's dst is 8 bytes wide")
    # n_planes, rows in all, elem_bytes, kind
    refused(desc(n_planes=0), "no plane")
    refused(desc(n_planes=_abi.ELOG_MAX_PLANES + 1), "too many planes")
    refused(desc(planes=((LAST, 4, 40), (LAST, 4, 40), (LAST, 4, 17))), "97 rows")
    refused(desc(edit=plane(0, n_rows=0)), "a plane without rows")
    refused(desc(edit=plane(0, n_rows=-1)), "negative rows")
    for eb in (0, 2, 3, 16, -1):
        refused(desc(edit=plane(1, elem_bytes=eb)), f"elem_bytes {eb}")
    refused(desc(edit=plane(3, elem_bytes=1)), "a float sum of one byte")
    refused(desc(edit=plane(5, elem_bytes=1)), "an integer sum of one byte")
    refused(desc(edit=plane(3, elem_bytes=8)), "SUM_F32 of eight bytes")
    refused(desc(edit=plane(4, elem_bytes=4)), "SUM_F64 of four bytes")
    refused(desc(edit=plane(0, kind=4)), "kind 4")
    refused(desc(edit=plane(0, kind=-1)), "kind -1")
    # strides, capacity, num_envs
    refused(desc(edit=plane(2, src_stride=99)), "stride below num_envs")
    refused(desc(capacity=0), "capacity 0")
    refused(desc(capacity=-3), "capacity negative")
    refused(desc(num_envs=0), "num_envs 0")
    refused(desc(num_envs=-5), "num_envs negative")
    # tiles, as wedm_normalize refuses them
    refused(desc(tile_offset=-1), "negative offset")
    refused(desc(tile_offset=1), "past the workspace")
    refused(desc(num_envs=257, edit=lambda d: [setattr(d.plane[p], "src_stride", 300) for p in range(6)]), "two tiles in a workspace of one")
    refused(desc(n_tiles_total=0), "no workspace")
    refused(desc(n_tiles_total=4097), "too many tiles")
    # flags
    refused(desc(flags=8), "undefined flag")
    # an output block over an input block: plane 1's source is 3 rows of 128 floats, of which 2 * 128 + 100 are read
    src1 = A + 0x100000 * 2
    refused(desc(env_out=src1), "env_out on a source")
    refused(desc(edit=plane(0, dst=src1 + (2 * 128 + 100) * 4 - 1)), "dst reaches a source's last byte")
    refused(desc(edit=plane(3, acc=A + 0x1000 - 8 * 200 + 8)), "acc reaches terminated's first byte")
    refused(desc(head=A + 0x2000 + 96), "head inside truncated")
    refused(desc(tile_counts=A + 0x3000), "tile_counts on the mask")
    refused(desc(stamp_out=src1 - 64 * 8 + 8), "stamp_out's last word on a source's first")


# ------------------------------------------------------------------------------------------------ the definition
def loop_call(p: Problem, buf: np.ndarray, stamp: int, env_id_offset: int = 0) -> None:
    """The whole call on the blocks of ``buf``, one environment after the other in plain Python: written from the header's
    text, sharing nothing with `episode_log_definition`."""
    v = lambda name: p.view(buf, name)   # noqa: E731
    N, cap = p.N, p.capacity
    term, trunc = v("terminated"), v("truncated") if p.has_truncated else None
    mask = v("mask") if p.masked else None
    live = [mask is None or mask[e] != 0 for e in range(N)]
    fin = [live[e] and (term[e] != 0 or (trunc is not None and trunc[e] != 0)) for e in range(N)]
    tc, head = v("tile_counts"), v("head")
    for t in range(p.tiles):
        tc[p.tile_offset + t] = sum(fin[256 * t: 256 * (t + 1)])
    n = sum(int(c) for c in tc[: p.ntt])
    k = sum(int(c) for c in tc[: p.tile_offset])
    h0 = int(head[0])
    blocks = [(kind, v(f"src{i}"), v(f"dst{i}"), None if kind == LAST else v(f"acc{i}")) for i, (kind, _, _) in enumerate(p.spec)]
    for e in range(N):
        if not live[e]:
            continue
        for kind, src, dst, acc in blocks:
            if kind == LAST:
                continue
            for r in range(src.shape[0]):
                acc[r, e] = int(acc[r, e]) + int(src[r, e]) if kind == SUM_I32 else np.float64(acc[r, e]) + np.float64(src[r, e])
        if not fin[e]:
            continue
        if k >= n - cap:
            slot = (h0 + k) % cap
            for kind, src, dst, acc in blocks:
                for r in range(src.shape[0]):
                    if kind == LAST:
                        size = src.dtype.itemsize
                        dst.view(np.uint8).reshape(dst.shape[0], -1)[r, slot * size: (slot + 1) * size] = \
                            np.frombuffer(src[r, e: e + 1].tobytes(), dtype=np.uint8)
                    else:
                        dst[r, slot] = acc[r, e]
            v("env_out")[slot] = env_id_offset + e
            v("stamp_out")[slot] = stamp
        for kind, src, dst, acc in blocks:
            if kind != LAST:
                acc[:, e] = 0
        k += 1
    head[0] = h0 + n
    head[1] = n


SEEN = {"wrap": 0, "overflow": 0, "nan": 0}


@pytest.mark.parametrize("how", ["none", "first", "last", "few", "all"])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1000])
def test_the_definition_against_a_plain_loop(N, how):
    """Capacity 1, 7 and more than n; three calls in a row (the second with everybody's neighbours, so that the ring wraps
    across calls; the third as the first again); with and without a mask, with and without ``truncated``."""
    rng = np.random.default_rng(1000 * N + len(how))
    for case, cap in enumerate((1, 7, N + 5)):
        masked, with_trunc = (case + N) % 2 == 0, (case + len(how)) % 3 != 0
        p = Problem(rng, N, cap, pad=3 * (case % 2), head0=int(rng.integers(0, 50)), truncated=with_trunc, masked=masked)
        got, want = p.buf.copy(), p.buf.copy()
        fins = [finishing(rng, N, how), finishing(rng, N, "few"), finishing(rng, N, how)]
        for call, fin in enumerate(fins):
            mask = (rng.random(N) < 0.8).astype(np.uint8) if masked else None
            term, trunc = flags_from(rng, fin, mask)
            if not with_trunc:
                term, trunc = term | trunc, None
            for buf in (got, want):
                p.set_flags(buf, term, trunc, mask)
            h0 = int(p.view(want, "head")[0])
            p.define(got, stamp=10 + call, env_id_offset=4000)
            loop_call(p, want, stamp=10 + call, env_id_offset=4000)
            assert differences(p, got, want) == [], (N, how, cap, call)
            n = int(p.view(want, "head")[1])
            assert n == int((fin & (mask != 0 if masked else True)).sum())
            SEEN["wrap"] += h0 % cap + n > cap and n <= cap and cap > 1
            SEEN["overflow"] += n > cap
            assert all(p.view(got, name).tobytes() == p.view(p.buf, name).tobytes() for name in p.layout
                       if name.startswith("src")), "a source plane changed"


def test_the_cases_above_hold_what_they_name():
    """A ring that wraps across calls and n > capacity in one call occur among the cases above (one of them is run here, so
    that this test stands alone)."""
    test_the_definition_against_a_plain_loop(257, "all")
    assert SEEN["wrap"] > 0 and SEEN["overflow"] > 0, SEEN


def test_a_nan_keeps_its_payload_through_a_last_copy():
    rng = np.random.default_rng(5)
    N = 300
    p = Problem(rng, N, N + 5)
    buf = p.buf.copy()
    fin = np.ones(N, dtype=bool)
    p.set_flags(buf, fin.astype(np.uint8), np.zeros(N, dtype=np.uint8), None)
    p.define(buf, stamp=1)
    for i, (kind, dt, rows) in enumerate(p.spec):
        if kind == LAST and np.dtype(dt).kind == "f":
            src, dst = p.view(buf, f"src{i}"), p.view(buf, f"dst{i}")
            raw = np.uint32 if np.dtype(dt).itemsize == 4 else np.uint64
            assert np.isnan(src[:, :N]).sum() > 4, "the sources hold NaNs"
            assert np.array_equal(dst.view(raw)[:, :N], src.view(raw)[:, :N])
            assert len(set(src.view(raw)[:, :N][np.isnan(src[:, :N])].tolist())) == 2, "two payloads, one of them signalling"


@pytest.mark.parametrize("N,cap", [(1, 1), (257, 7), (1000, 100), (1000, 1005)])
def test_the_phases_apart_equal_the_one_call(N, cap):
    rng = np.random.default_rng(N + cap)
    p = Problem(rng, N, cap, spec=SPEC_MAX if N == 257 else SPEC, masked=True, head0=3)
    one, three = p.buf.copy(), p.buf.copy()
    for call in range(2):
        mask = (rng.random(N) < 0.7).astype(np.uint8)
        term, trunc = flags_from(rng, finishing(rng, N, "few" if call else "all"), mask)
        for buf in (one, three):
            p.set_flags(buf, term, trunc, mask)
        p.define(one, stamp=call)
        for phase in (COUNT, SCATTER, COMMIT):
            p.define(three, stamp=call, flags=phase)
        assert differences(p, three, one) == []
    # COUNT alone writes this batch's tile counts and nothing else; COMMIT alone writes head
    alone = one.copy()
    p.define(alone, stamp=9, flags=COUNT)
    assert all(d.startswith("tile_counts") for d in differences(p, alone, one))
    p.define(alone, stamp=9, flags=COMMIT)
    assert {d.split(":")[0] for d in differences(p, alone, one)} <= {"tile_counts", "head"}


@pytest.mark.parametrize("N,first", [(768, 256), (1000, 512)])
@pytest.mark.parametrize("cap", [5, 64, 2000])
def test_shards_in_turn_equal_the_whole_batch_on_every_byte(N, first, cap):
    """COUNT every shard into its tiles of one workspace, SCATTER every shard, COMMIT once."""
    rng = np.random.default_rng(N + cap)
    p = Problem(rng, N, cap, spec=SPEC_SHARD, masked=True, head0=11, pad=2)
    whole, shards = p.buf.copy(), p.buf.copy()
    parts = ((0, first), (first, N - first))
    for call, how in enumerate(("few", "all", "few")):
        mask = (rng.random(N) < 0.8).astype(np.uint8)
        term, trunc = flags_from(rng, finishing(rng, N, how), mask)
        for buf in (whole, shards):
            p.set_flags(buf, term, trunc, mask)
        p.define(whole, stamp=call, env_id_offset=70)
        for phase in (COUNT, SCATTER):
            for part in parts:
                p.define(shards, stamp=call, env_id_offset=70, flags=phase, part=part)
        p.define(shards, stamp=call, env_id_offset=70, flags=COMMIT, part=parts[1])
        assert differences(p, shards, whole) == [], (call, how)
    want = whole.copy()
    loop_call(p, want, stamp=3, env_id_offset=70)
    p.define(whole, stamp=3, env_id_offset=70)
    assert differences(p, whole, want) == []


# ------------------------------------------------------------------------------------------------ the stack
def host(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy().copy()


def scan_step(vec, out, sums, records, stamp):
    """What an observer of the adapter collects from one step: the flags it handed out and the state blocks, environment
    by environment, with accumulators of its own."""
    _, reward, term, trunc, info = out
    env, st = vec.env, vec.env.state
    n = env.num_envs
    term, trunc = host(term), host(trunc)
    raw = host(info["raw_reward"]).astype(np.float64)
    pulse, signal = host(st.pulse), host(st.signal)
    stats = {k: host(v) for k, v in info["episode_stats"].items()}
    time = host(st.time)
    for e in range(n):
        sums["reward_sum"][e] += raw[e]
        sums["steps"][e] += 1
        for name, r in (("sparks", _abi.PULSE.SPARK_LAST), ("shorts", _abi.PULSE.SHORT_LAST), ("short_steps", _abi.PULSE.SHORT_STEPS_LAST)):
            sums[name][e] += int(pulse[r, e])
        for name, r in (("samples", _abi.SIG.SAMPLES_LAST), ("current", _abi.SIG.CURRENT_LAST), ("energy", _abi.SIG.ENERGY_LAST)):
            sums[name][e] += signal[r, e]
        if not (term[e] or trunc[e]):
            continue
        rec = {"env": env.env_id_offset + e, "stamp": stamp, "terminated": bool(term[e]), "truncated": bool(trunc[e]),
               "wire_broken": bool(st.is_wire_broken[e]), "target_reached": bool(st.is_target_distance_reached[e]),
               "time_us": int(time[e]), "episode": int(st.episode[e]), "spark_count": int(st.spark_count[e]),
               "workpiece_position": float(st.workpiece_position[e]), "wire_position": float(st.wire_position[e]),
               "tmax": float(st.wire_max_temperature[e]), "episode_count": int(vec.episode_count[e]),
               "return": float(stats["r"][e]), "length": int(stats["l"][e]), "draw": int(vec._episode_sampler._count[e]),
               "material": int(env._wmat_index[e]), "height": float(env._dyn.height[e]), "diameter_index": int(env._dyn.dia[e])}
        rec.update({f"envp_{f.name.lower()}": float(env._envp_rows[int(f), e]) for f in _abi.ENVP})
        rec.update({f"held.{name}": float(env._envp_src[envp.INDEX[name], e]) for name in vec._episode_sampler.params})
        for name in sums:
            rec[name] = sums[name][e]
            sums[name][e] = 0
        records.append(rec)
    return int((term | trunc).sum()), term, trunc


@pytest.mark.parametrize("capacity", [16, 4096])
def test_the_log_of_a_stack_equals_an_independent_host_scan(capacity):
    """capacity 16: the ring wraps and the reader, who comes every third step, loses records; capacity 4096: nothing is lost."""
    vec, log, action = full_stack("cpu", capacity)
    n = vec.num_envs
    assert log._native is None, "the oracle backends run the definition"
    sums = {"reward_sum": np.zeros(n), "steps": [0] * n, "sparks": [0] * n, "shorts": [0] * n, "short_steps": [0] * n,
            "samples": np.zeros(n), "current": np.zeros(n), "energy": np.zeros(n)}
    records, read, per_step, lost = [], [], [], 0
    any_term = any_trunc = False
    for step in range(1, 10):
        if step == 9:   # a reset of everybody cuts every episode: nothing is logged, every sum starts again
            vec.reset()
            sums = {k: np.zeros(n) if isinstance(v, np.ndarray) else [0] * n for k, v in sums.items()}
        out = vec.step(action)
        count, term, trunc = scan_step(vec, out, sums, records, step)
        per_step.append(count)
        any_term, any_trunc = any_term or bool(term.any()), any_trunc or bool(trunc.any())
        if step % 3 == 0:
            peek = log.peek()
            got = log.read()
            assert all(np.array_equal(peek[k], got[k]) for k in got), "peek is read without moving the cursor"
            lost += got["lost"]
            # what a reader sees: the newest `capacity` records of all so far, minus what was read before
            want = records[max(len(records) - capacity, sum(len(r["env"]) for r in read) + lost):]
            assert len(got["env"]) == len(want)
            read.append(got)
            for i, rec in enumerate(want):
                for key, value in rec.items():
                    if key.startswith("held."):
                        continue
                    g = got[key][i]
                    assert g == value or (value != value and g != g), (step, i, key, g, value)
            assert log.read()["env"].shape == (0,), "a second read finds nothing new"
    vec.env.check_errors()
    # the physics of every logged episode from the log alone
    sampler = vec._episode_sampler
    for got in read:
        want = sampler.expected(got["env"], got["draw"] - 1)
        assert np.array_equal(want["wire_material"], got["material"])
        assert np.array_equal(want["workpiece_height"], got["height"])
        assert np.array_equal(want["wire_diameter_index"], got["diameter_index"])
    by_key = {(r["env"], r["stamp"]): r for r in records}
    for got in read:
        want = sampler.expected(got["env"], got["draw"] - 1)
        for i in range(len(got["env"])):
            rec = by_key[(int(got["env"][i]), int(got["stamp"][i]))]
            for name in sampler.params:
                assert want[name][i] == rec[f"held.{name}"], (name, i)
    # the run itself
    flat = {k: np.concatenate([g[k] for g in read]) for k in ("terminated", "truncated", "wire_broken", "target_reached", "steps")}
    assert any_term and any_trunc and flat["terminated"].any() and flat["truncated"].any()
    assert any(r["wire_broken"] for r in records) and any(r["target_reached"] for r in records)
    if capacity > 16:
        assert flat["wire_broken"].any() and flat["target_reached"].any() and len(flat["steps"]) == len(records)
    assert 0 in per_step and max(per_step) > 1, per_step
    assert len(records) > 16, "more episodes than the small ring holds"
    assert (lost > 0) == (capacity == 16), (lost, capacity)
    assert set(flat["steps"].tolist()) - {1}, "episodes of more than one control step"
    summary = log.summary(read[-1])
    assert summary["episodes"] == len(read[-1]["env"]) and set(summary["per_material"]) == set(m.name for m in vec.env.wire_materials)
    assert sum(s["episodes"] for s in summary["per_material"].values()) == summary["episodes"]
    vec.close()


# ------------------------------------------------------------------------------------------------ behaviour
def frozen_stack(seed: int = 3, capacity: int = 256, **kw):
    env = snap.make("cpu", 30, "all", "s13")
    log = EpisodeLog(capacity=capacity, **kw)
    vec = WireEDMVectorEnv(env, autoreset=False, max_episode_steps=2000, reward="progress", normalizer=Normalizer(), episode_log=log)
    vec.reset(seed=seed)
    return vec, log, snap.scenario(env, seed=seed + 1)


def test_with_autoreset_off_every_episode_is_logged_once():
    vec, log, action = frozen_stack()
    done = np.zeros(30, dtype=bool)
    for _ in range(4):
        _, _, term, trunc, _ = vec.step(action)
        done |= host(term | trunc)
    rec = log.read()
    assert done.all() and sorted(rec["env"].tolist()) == list(range(30)), "everybody ended, everybody is logged once"
    assert set(rec["stamp"].tolist()) == {1, 2} and (rec["steps"] == rec["stamp"]).all()
    assert (rec["length"] == rec["steps"]).all()
    vec.close()


def test_reset_logs_nothing_and_zeroes_the_sums():
    vec, log, action = frozen_stack()
    vec.step(action)
    head = host(log._head)
    steps = next(p for p in log._planes if p.names == ("steps",))
    live = host(steps.acc)[0] == 1
    assert 0 < live.sum() < 30, "some environments are in mid-episode"
    mask = torch.arange(30) % 2 == 0
    vec.reset(options={"mask": mask})
    assert np.array_equal(host(log._head), head) and log.peek()["env"].shape[0] == head[0]
    for p in log._planes:
        if p.acc is not None:
            acc = host(p.acc)
            assert not acc[:, ::2].any(), p.names
    assert np.array_equal(host(steps.acc)[0, 1::2], live[1::2].astype(np.int64))
    vec.reset()
    assert not any(host(p.acc).any() for p in log._planes if p.acc is not None) and np.array_equal(host(log._head), head)
    vec.close()


def test_fork_carries_the_sums():
    vec, log, action = frozen_stack()
    vec.step(action)
    before = {p.names: host(p.acc) for p in log._planes if p.acc is not None}
    vec.fork([0, 1, 2], [10, 11, 12])
    assert any(b[:, [0, 1, 2]].tobytes() != b[:, [10, 11, 12]].tobytes() for b in before.values())
    for p in log._planes:
        if p.acc is not None:
            want = before[p.names].copy()
            want[:, [10, 11, 12]] = want[:, [0, 1, 2]]
            assert host(p.acc).tobytes() == want.tobytes(), p.names
    vec.close()


def log_bytes(log) -> dict:
    sd = log.state_dict()
    out = {k: v for k, v in sd.items() if torch.is_tensor(v)}
    out.update({f"ring{i}": t for i, t in enumerate(sd["ring"])})
    out.update({f"sums{i}": t for i, t in enumerate(sd["sums"])})
    out["plain"] = torch.tensor([sd["cursor"], sd["stamp"], sd["capacity"], sd["num_envs"]])
    return {k: v.numpy().tobytes() for k, v in out.items()}


def test_a_checkpoint_inside_an_episode_continues_on_the_bytes_of_the_uninterrupted_log(tmp_path):
    a, log_a, action = full_stack("cpu", 32, n=40)
    for _ in range(2):
        a.step(action)
    log_a.read()                                       # the cursor is part of the state
    a.step(action)
    steps = next(p for p in log_a._planes if p.names == ("steps",))
    assert len(set(host(steps.acc)[0].tolist())) > 1, "the cut lies inside episodes of different ages"
    a.save_checkpoint(tmp_path / "cut.pt")
    b, log_b, _ = full_stack("cpu", 32, n=40, seed=9)    # another seed, dirtied by steps of its own
    b.step(action)
    b.load_checkpoint(tmp_path / "cut.pt")
    assert log_bytes(log_b) == log_bytes(log_a)
    for _ in range(4):
        a.step(action)
        b.step(action)
    assert log_bytes(log_b) == log_bytes(log_a)
    ra, rb = log_a.read(), log_b.read()
    assert ra["env"].shape[0] > 0 and all(np.array_equal(ra[k], rb[k], equal_nan=np.asarray(ra[k]).dtype.kind == "f") for k in ra)
    a.close()
    b.close()


def test_refusals_leave_the_target_untouched():
    src, log_src, action = frozen_stack()
    src.step(action)
    sd = src.state_dict()
    targets = {"capacity": frozen_stack(seed=4, capacity=128), "columns": frozen_stack(seed=4, params=True)}
    env = snap.make("cpu", 31, "all", "s13")
    other = WireEDMVectorEnv(env, autoreset=False, max_episode_steps=2000, reward="progress", normalizer=Normalizer(),
                             episode_log=EpisodeLog(capacity=256))
    other.reset(seed=4)
    for word, (dst, log_dst, _) in targets.items():
        dst.step(action)
        before = log_bytes(log_dst)
        held = vec_everything(dst)
        with pytest.raises(ValueError, match=word):
            dst.load_state_dict(sd)
        with pytest.raises(ValueError, match=word):
            log_dst.load_state_dict(sd["episode_log"])
        assert log_bytes(log_dst) == before
        assert_equal(vec_everything(dst), held, f"refused ({word}): the target changed")
        dst.load_state_dict(dst.state_dict())
        assert log_bytes(log_dst) == before
        dst.close()
    with pytest.raises(ValueError, match="environments"):
        other.episode_log.load_state_dict(sd["episode_log"])
    # a log on one side only
    plain = WireEDMVectorEnv(snap.make("cpu", 30, "all", "s13"), autoreset=False, max_episode_steps=2000, reward="progress",
                             normalizer=Normalizer())
    plain.reset(seed=4)
    with pytest.raises(ValueError, match="episode_log"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="episode_log"):
        src.load_state_dict(plain.state_dict())
    for v in (src, other, plain):
        v.close()


def test_an_adapter_without_a_log_has_the_state_dict_keys_it_had():
    plain = WireEDMVectorEnv(snap.make("cpu", 6, "plain", "s13"), max_episode_steps=3000)
    plain.reset(seed=1)
    keys = ["num_envs", "autoreset", "max_episode_steps", "wire_profile_bins", "obs_names", "reward", "samplers", "need_reset",
            "episode_count", "env"]
    assert list(plain.state_dict()) == keys
    normed = WireEDMVectorEnv(snap.make("cpu", 6, "plain", "s13"), normalizer=Normalizer())
    normed.reset(seed=1)
    assert list(normed.state_dict()) == keys + ["normalizer"]
    logged = WireEDMVectorEnv(snap.make("cpu", 6, "plain", "s13"), normalizer=Normalizer(), episode_log=EpisodeLog(8))
    logged.reset(seed=1)
    assert list(logged.state_dict()) == keys + ["normalizer", "episode_log"]
    torch.save(logged.state_dict(), io.BytesIO())
    for v in (plain, normed, logged):
        v.close()


def test_the_shard_cases_store_every_record_none_and_a_strict_part():
    """The input conditions of tests/test_episode_log.py's shard in a large workspace, over its whole parametrisation: some call stores every finishing record of
    the shard, some call stores none of them though some finish (the SUM planes still move), some a strict part; and the
    largest total reaches 900 000, near the 1 048 576 that the kernels' int32 sums are said to hold."""
    seen, largest = set(), 0
    for ntt in WORKSPACES:
        for where in WHERE:
            for draw in DRAWS:
                for cap in CAPS:
                    offset, others, _, capacity, stored, _ = shard_case(ntt, where, draw, cap)
                    largest = max(largest, int(others.sum()))
                    assert 0 <= offset and offset + 2 <= ntt and all(n > 0 for _, n in stored)
                    seen |= {"every" if s == n else ("none" if s == 0 else "part") for s, n in stored}
    assert seen == {"every", "none", "part"} and largest > 900_000
