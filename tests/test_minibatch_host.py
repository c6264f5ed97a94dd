"""The seeded minibatch permutation (sparc_amd/minibatch.py) on the host side: the ABI mirror of
``wedm_mb_desc`` and the export with its refusals (no device is needed); the bijection E exhaustively, the walk PI and the
placement's properties; hand-worked cases; a chi-square of the row-by-part membership counts against a uniform shuffle's; a
checkpoint of a `MinibatchSampler` alone; and the training stacks of tests/_optimizer_common.py with a `MinibatchSampler` on
the CPU oracle backend, cut at every control step.

Measured here with the definition (R = 4 096, n = 8, every row live, seed 3, draws 0 ... 255; recorded in DESIGN.md section
4.24): chi-square 28 735.8 against 28 672 expected and 28 153.7 ... 29 184.8 over 20 uniform shuffles; neighbouring rows in one part
0.1245 of the time against 0.1248 expected; the longest walk 1 at V = 2^20 and 21 at V = 2^20 + 1."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from sparc_amd import MinibatchSampler, RolloutBuffer, _abi, _lib
from sparc_amd.minibatch import bijection, keys, minibatch_index_reference, part_bounds, walk
from sparc_amd.randomize import philox4x32_10
from tests import _minibatch_common as mc

ROOT = Path(__file__).resolve().parent.parent
KEY_SETS = ((3, 0), (0xDEADBEEF_00000001, 2 ** 40 + 7))   # (seed, draw)


# ------------------------------------------------------------------------------------------------ 1. the C-ABI
def test_desc_struct_mirror_matches_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wedm_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(wedm_mb_desc));']
    for field, _ in _abi.MbDesc._fields_:
        lines.append(f'  printf("{field} %zu\\n", offsetof(wedm_mb_desc, {field}));')
    lines += ['  printf("consts %d %d %d %u abi %d\\n", WEDM_MB_TILE, WEDM_MB_MAX_ROWS, WEDM_MB_MAX_PARTS, WEDM_MB_STREAM0, WEDM_ABI_VERSION);',
              '  printf("flagbits %d %d %d\\n", WEDM_MB_COUNT, WEDM_MB_OFFSETS, WEDM_MB_SCATTER);',
              '  printf("streams %u %u\\n", WEDM_DRAW_STREAM0, WEDM_HEAD_STREAM0);', "  return 0;", "}"]
    src = tmp_path / "desc.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "desc"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    out = dict(row.split(" ", 1) for row in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("size")) == C.sizeof(_abi.MbDesc)
    assert out.pop("consts") == f"{_abi.MB_TILE} {_abi.MB_MAX_ROWS} {_abi.MB_MAX_PARTS} {_abi.MB_STREAM0} abi 4"
    assert (_abi.MB_TILE, _abi.MB_MAX_ROWS, _abi.MB_MAX_PARTS, _abi.MB_STREAM0) == (1024, 2 ** 26, 4096, 0xE0000000)
    assert out.pop("flagbits") == "1 2 4" == f"{_abi.MB_COUNT} {_abi.MB_OFFSETS} {_abi.MB_SCATTER}"
    # clear of the other streams: the draw calls count up from theirs by a few, the head's reach 0xC0000000 + 256
    assert out.pop("streams") == f"{_abi.DRAW_STREAM0} {_abi.HEAD_STREAM0}" and _abi.DRAW_STREAM0 < _abi.HEAD_STREAM0 + 256 < _abi.MB_STREAM0
    assert {k: int(v) for k, v in out.items()} == {f: getattr(_abi.MbDesc, f).offset for f, _ in _abi.MbDesc._fields_}


def test_the_call_is_exported_and_the_abi_version_stays():
    assert "wedm_minibatch_index" in _lib.EXPORTS and hasattr(_lib.HipBackend, "minibatch_index")
    L = _lib.load()
    assert L.wedm_minibatch_index is not None and L.wedm_abi_version() == _abi.ABI_VERSION == 4
    assert "int32_t wedm_minibatch_index(const wedm_mb_desc* desc, void* stream);" in (ROOT / "include" / "wedm_hip.h").read_text()


def test_bad_arguments_are_refused_before_anything_is_launched():
    """Every pointer below is an address nobody owns: a call that launched would fault (and on a machine without a device
    fail with WEDM_ERR_HIP); every case returns WEDM_ERR_BAD_ARG with a text."""
    L = _lib.load()
    A, rows = 0x1000000, 3000   # blocks 0x100000 apart: the largest holds 24 000 bytes; three tiles
    names = ("valid", "index", "count", "tile_counts", "tile_base")
    at = {name: A + 0x100000 * i for i, name in enumerate(names)}
    size = {"valid": rows, "index": 8 * rows, "count": 16, "tile_counts": 12, "tile_base": 12}
    elem = {"valid": 1, "index": 8, "count": 8, "tile_counts": 4, "tile_base": 4}
    PHASES = (_abi.MB_COUNT, _abi.MB_OFFSETS, _abi.MB_SCATTER)

    def desc(**kw):
        f = dict(at, seed=1, draw=2, rows=rows, n_parts=8, flags=0)
        f.update(kw)
        return _abi.MbDesc(**f)

    def refused(d, what):
        assert L.wedm_minibatch_index(C.byref(d), None) == _abi.ERR_BAD_ARG, what
        text = L.wedm_last_error(None)
        assert text.startswith(b"wedm_minibatch_index: ") and len(text) > len(b"wedm_minibatch_index: "), what

    assert L.wedm_minibatch_index(None, None) == _abi.ERR_BAD_ARG and L.wedm_last_error(None).startswith(b"wedm_minibatch_index: ")
    for flags in (8, -1, 1 << 30, 16 | _abi.MB_COUNT, 7 | 64):
        refused(desc(flags=flags), ("flags", flags))
    for bad in (0, -5, _abi.MB_MAX_ROWS + 1, 2 ** 31 - 1):
        refused(desc(rows=bad, n_parts=1), ("rows", bad))
    for bad_rows, bad_n in ((rows, 0), (rows, -1), (rows, rows + 1), (5, 6), (1, 2), (_abi.MB_MAX_ROWS, _abi.MB_MAX_PARTS + 1), (rows, 2 ** 31 - 1)):
        for flags in (0,) + PHASES:   # in whichever phase
            refused(desc(rows=bad_rows, n_parts=bad_n, flags=flags), ("n_parts", bad_rows, bad_n, flags))
    # every block a phase needs: null, and off its alignment (valid may be null and sit at any address)
    for name in names[1:]:
        refused(desc(**{name: None}), ("null", name))
        for off in range(1, elem[name]):
            refused(desc(**{name: at[name] + off}), ("off its alignment by", off, name))
            for flags in PHASES:   # (alignment counts in every phase)
                refused(desc(flags=flags, **{name: at[name] + off}), ("off its alignment by", off, name, flags))
    for flags, needed in ((_abi.MB_COUNT, ("tile_counts",)), (_abi.MB_OFFSETS, ("tile_counts", "tile_base", "count")),
                          (_abi.MB_SCATTER, ("tile_base", "count", "index"))):
        for name in needed:
            refused(desc(flags=flags, **{name: None}), ("null in its phase alone", flags, name))
    # every output block on valid and on every other output block: its first byte on the other's first and last element,
    # and its last element on the other's first byte
    for a in names[1:]:
        for b in names:
            if a == b:
                continue
            refused(desc(**{a: at[b]}), (a, "on", b))
            last = at[b] + size[b] - 1
            refused(desc(**{a: last - last % elem[a]}), (a, "on the last byte of", b))
            refused(desc(**{a: at[b] - size[a] + elem[a]}), ("the last element of", a, "on the first byte of", b))
    # and next to each other they are fine as far as the checks go: with no device the launch itself fails, as WEDM_ERR_HIP
    if not torch.cuda.is_available():
        d = desc(count=at["index"] + size["index"], tile_counts=at["index"] + size["index"] + 16)
        assert L.wedm_minibatch_index(C.byref(d), None) == _abi.ERR_HIP


# ------------------------------------------------------------------------------------------------ 2. E, PI, the placement
def test_the_keys_are_two_philox_blocks_of_the_draw():
    seed, draw = 0x0123456789ABCDEF, 0xFEDCBA9876543210
    K = keys(seed, draw)
    for c in range(2):
        w = philox4x32_10((0x76543210, 0xFEDCBA98, 0, 0xE0000000 + c), (0x89ABCDEF, 0x01234567))
        assert [int(x) for x in w] == K[4 * c: 4 * c + 4].tolist()
    assert K.dtype == np.uint32 and len(set(K.tolist())) == 8


@pytest.mark.parametrize("seed,draw", KEY_SETS)
def test_e_is_a_bijection_of_every_width_up_to_sixteen_bits(seed, draw):
    K = keys(seed, draw)
    for bits in range(17):
        y = bijection(np.arange(1 << bits, dtype=np.uint32), bits, K)
        assert y.dtype == np.uint32 and np.array_equal(np.sort(y), np.arange(1 << bits)), bits
        if bits >= 8:
            assert not np.array_equal(y, np.arange(1 << bits)) and int((y == np.arange(1 << bits)).sum()) < 16


def test_e_round_by_round_in_plain_python():
    """bits = 5: hl = 2, hh = 3, in Python's integers."""
    K = [int(k) for k in keys(*KEY_SETS[0])]

    def mix(x):
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & 0xFFFFFFFF
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & 0xFFFFFFFF
        return x ^ (x >> 16)

    for x in range(32):
        lo, hi = x & 3, x >> 2
        for i in range(8):
            if i % 2 == 0:
                hi ^= mix(lo ^ K[i]) & 7
            else:
                lo ^= mix(hi ^ K[i]) & 3
        assert int(bijection(np.array([x], dtype=np.uint32), 5, np.array(K, dtype=np.uint32))[0]) == (hi << 2 | lo)


@pytest.mark.parametrize("V", (1, 2, 3, 5, 255, 256, 257, 4097, 65537))
def test_the_walk_is_a_permutation(V):
    for seed, draw in KEY_SETS:
        pi, steps = walk(V, keys(seed, draw), with_steps=True)
        assert np.array_equal(np.sort(pi), np.arange(V)) and steps.min() >= 1
        bits = (V - 1).bit_length() if V > 1 else 0
        assert 2 ** bits < 2 * V or V == 1
        # the first of E(k), E(E(k)), ... below V, element by element for the small ones
        if V <= 257:
            K = keys(seed, draw)
            for k in range(V):
                x = k
                for _ in range(int(steps[k])):
                    x = int(bijection(np.array([x], dtype=np.uint32), bits, K)[0])
                    assert x >= V or x == pi[k]
                assert x == pi[k]
        assert steps.max() <= 64 and steps.mean() < 2.0


def test_the_longest_walks_that_were_measured():
    for V, longest in ((2 ** 20, 1), (2 ** 20 + 1, 21)):
        assert int(walk(V, keys(3, 0), with_steps=True)[1].max()) == longest


@pytest.mark.parametrize("R", (1, 2, 9, 50, 1023, 1025, 2500))
def test_the_placement_properties(R):
    for name, valid in mc.masks(R, seed=R).items():
        V = R if valid is None else int((valid != 0).sum())
        for n in sorted({1, 2, 7, 8, R, max(1, min(V + 3, R))}):   # ... and more parts than live rows
            if n > min(R, _abi.MB_MAX_PARTS):
                continue
            index, count, tile_counts, tile_base = minibatch_index_reference(valid, n, 11, 4, rows=R)
            mc.check_placement(index, valid, n)
            assert count.tolist() == [V, R - V] and count.dtype == np.int64
            live = np.ones(R, dtype=bool) if valid is None else valid != 0
            want = [int(live[t: t + 1024].sum()) for t in range(0, R, 1024)]
            assert tile_counts.tolist() == want and tile_base.tolist() == [sum(want[:t]) for t in range(len(want))]
            assert tile_counts.dtype == tile_base.dtype == np.int32


def test_hand_worked_no_live_row_and_one_live_row():
    R, n = 11, 3
    index = minibatch_index_reference(np.zeros(R, dtype=np.uint8), n, 5, 0)[0]
    off, cnt = part_bounds(R, n)
    assert off.tolist() == [0, 4, 8] and cnt.tolist() == [4, 4, 3]
    for p in range(n):
        assert index[off[p]: off[p] + cnt[p]].tolist() == [p + s * n for s in range(cnt[p])]
    assert index.tolist() == [0, 3, 6, 9, 1, 4, 7, 10, 2, 5, 8]
    for r in range(R):   # one live row: slot 0 of part 0, the dead rows in their order behind it, round-robin from part 1 on
        valid = np.zeros(R, dtype=np.uint8)
        valid[r] = 7
        index, count = minibatch_index_reference(valid, n, 5, 0)[:2]
        dead = [x for x in range(R) if x != r]
        assert index[0] == r and count.tolist() == [1, 10]
        assert index[off[1]: off[1] + 4].tolist() == dead[0::3] and index[1:4].tolist() == dead[2::3] and index[8:].tolist() == dead[1::3]


def test_both_words_of_the_draw_and_of_the_seed_count():
    R, n = 1000, 8
    ref = lambda seed, draw: minibatch_index_reference(None, n, seed, draw, rows=R)[0]   # noqa: E731
    a = ref(9, 5)
    assert np.array_equal(a, ref(9, 5))
    assert not np.array_equal(a, ref(9, 2 ** 32 + 5)) and not np.array_equal(a, ref(9, 6))
    assert not np.array_equal(a, ref(2 ** 32 + 9, 5)) and not np.array_equal(a, ref(2 ** 63 + 9, 5)) and not np.array_equal(a, ref(10, 5))
    with pytest.raises(ValueError):
        minibatch_index_reference(None, n, 0, 0)
    for rows, parts in ((5, 6), (5, 0), (10 ** 4, 4097)):
        with pytest.raises(ValueError):
            minibatch_index_reference(None, parts, 0, 0, rows=rows)


# ------------------------------------------------------------------------------------------------ 3. the statistic
def _membership_chi_square(part_of_row, draws: int, R: int, n: int) -> float:
    """Chi-square of the row-by-part membership counts over ``draws`` permutations against ``draws / n``;
    ``part_of_row(d)`` gives the part of every row in permutation ``d``."""
    M = np.zeros((R, n), dtype=np.int64)
    for d in range(draws):
        M[np.arange(R), part_of_row(d)] += 1
    expected = draws / n
    return float(((M - expected) ** 2 / expected).sum())


def test_rows_meet_parts_as_evenly_as_under_a_uniform_shuffle():
    """R = 4 096, n = 8, every row live, seed 3, draws 0 ... 255: the chi-square of the membership counts against 32 is at
    most the largest of 20 trials in which ``numpy.random.default_rng(0).permutation`` takes the walk's place."""
    R, n, draws = 4096, 8, 256
    off, cnt = part_bounds(R, n)
    part_at = np.repeat(np.arange(n), cnt)   # the part of every entry of index
    neighbours = [0]

    def ours(d):
        index = minibatch_index_reference(None, n, 3, d, rows=R)[0]
        part = np.empty(R, dtype=np.int64)
        part[index] = part_at
        neighbours[0] += int((part[1:] == part[:-1]).sum())
        return part

    got = _membership_chi_square(ours, draws, R, n)
    rng = np.random.default_rng(0)
    trials = [_membership_chi_square(lambda d: rng.permutation(R) % n, draws, R, n) for _ in range(20)]
    share = neighbours[0] / (draws * (R - 1))
    print(f"chi-square {got:.1f} (expected {R * (n - 1)}); 20 uniform trials {min(trials):.1f} ... {max(trials):.1f}; "
          f"neighbouring rows in one part {share:.4f} (expected {(R / n - 1) / (R - 1):.4f})")
    assert got <= max(trials)


# ------------------------------------------------------------------------------------------------ 4. the sampler, its checkpoint
class _Vec:
    """What a `RolloutBuffer` asks of its adapter, on the CPU."""

    def __init__(self, n):
        self.num_envs, self.obs_names = n, ("a", "b")
        self.env = type("E", (), {"device": torch.device("cpu"), "_backend": None})()


def _finished_buffer(T=5, N=37, seed=0) -> RolloutBuffer:
    buf = RolloutBuffer(_Vec(N), T)
    g = torch.Generator().manual_seed(seed)
    for _ in range(T):
        done = torch.rand(N, generator=g) < 0.2
        buf.add(torch.randn(N, 2, generator=g), torch.randn(N, generator=g), torch.randn(N, generator=g), torch.randn(N, generator=g),
                done, torch.zeros(N, dtype=torch.bool))
    buf.finish(torch.randn(N, generator=g))
    return buf


def test_the_sampler_draws_the_definition_and_its_state_dict_resumes_it(tmp_path):
    buf = _finished_buffer()
    valid = buf.computed["valid"]
    R = valid.numel()
    assert 0 < int(valid.sum()) < R
    whole = MinibatchSampler(buf, 4, seed=2 ** 63 + 12345)
    drawn = []
    for d in range(5):
        parts = whole.draw()
        assert whole.draws == d + 1 and len(parts) == 4 and all(p.dtype == torch.int64 for p in parts)
        index, count, tile_counts, tile_base = minibatch_index_reference(valid.numpy(), 4, 2 ** 63 + 12345, d)
        assert np.array_equal(torch.cat(parts).numpy(), index) and np.array_equal(whole.index.numpy(), index)
        assert [p.shape[0] for p in parts] == [t.shape[0] for t in torch.tensor_split(torch.arange(R), 4)]
        assert whole.count.tolist() == count.tolist() and all(np.array_equal(a, b) for a, b in zip(whole.expected(valid, d), (index, count, tile_counts, tile_base)))
        assert parts[0].data_ptr() == whole.index.data_ptr()   # views, not copies
        mc.check_placement(index, valid.numpy(), 4)
        drawn.append(index)
        if d == 2:
            torch.save({"mb": whole.state_dict()}, tmp_path / "mb.pt")
    assert len({a.tobytes() for a in drawn}) == 5
    # into an object built with another seed and another number of parts, dirtied by draws of its own
    other = MinibatchSampler(buf, 7, seed=1)
    other.draw(), other.draw()
    other.load_state_dict(torch.load(tmp_path / "mb.pt", map_location="cpu", weights_only=True)["mb"])
    assert other.state_dict() == {"seed": 2 ** 63 + 12345, "n_parts": 4, "draws": 3} and whole.state_dict() == dict(other.state_dict(), draws=5)
    for d in (3, 4):
        assert np.array_equal(torch.cat(other.draw()).numpy(), drawn[d])
    # minibatches(n, sampler=) gathers in the sampler's order; without a sampler the method is what it was
    flat = buf.flat()
    got = list(buf.minibatches(4, sampler=other))
    want = minibatch_index_reference(valid.numpy(), 4, other.seed, 5)[0]
    assert other.draws == 6 and np.array_equal(torch.cat([g["reward"] for g in got]).numpy(), flat["reward"].numpy()[want])
    assert set(got[0]) == set(flat)
    plain = list(buf.minibatches(4, generator=torch.Generator().manual_seed(3)))
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(3))
    assert torch.equal(torch.cat([g["reward"] for g in plain]), flat["reward"][perm]) and other.draws == 6
    # refusals
    with pytest.raises(ValueError, match="n_parts"):
        list(buf.minibatches(5, sampler=other))
    with pytest.raises(ValueError, match="this buffer's"):
        list(_finished_buffer(seed=1).minibatches(4, sampler=other))
    for bad in (0, R + 1, 4097):
        with pytest.raises(ValueError):
            MinibatchSampler(buf, bad)
    with pytest.raises(ValueError):
        other.load_state_dict({"seed": 1, "n_parts": R + 1, "draws": 0})
    assert (other.seed, other.n_parts, other.draws) == (2 ** 63 + 12345, 4, 6)
    with pytest.raises(ValueError):
        MinibatchSampler(buf, 2, seed=-1)
    with pytest.raises(ValueError, match="at most"):
        MinibatchSampler(type("B", (), {"num_steps": 2 ** 13, "num_envs": 2 ** 13 + 1, "device": torch.device("cpu")})(), 2)
    buf.add(torch.zeros(37, 2), torch.zeros(37), torch.zeros(37), torch.zeros(37), torch.zeros(37, dtype=torch.bool), torch.zeros(37, dtype=torch.bool))
    with pytest.raises(ValueError, match="not finished"):
        other.draw()


# ------------------------------------------------------------------------------------------------ 5. the stacks
@pytest.mark.parametrize("variant", ("in-kernel", "frozen", "host-reset"))
def test_the_stack_with_a_minibatch_sampler_resumes_byte_for_byte_at_every_cut(variant, tmp_path):
    mc.check_resume_at_every_cut(variant, "cpu", tmp_path)
