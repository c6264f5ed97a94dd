"""The catalogue behind tests/test_registry_host.py and tests/test_registry_coverage.py: for every instantiation of a step
kernel that the library registers (`sparc_amd._lib.registry()`: kernel, lanes per environment, form bits) at least one
recipe -- a handle and a sequence of launches -- that is expected to make `plan_launch` select it.

A recipe names what it forces (kernel, lanes), what it binds, its wire length and the geometry bits that length is there
for; `Recipe.launches()` derives from them, without a device, the instantiation every launch is expected to run.  The GPU
test asserts after every launch that `last_form()` is that instantiation, so a wrong constant here fails at once.

The conditions are those of `choose_kernel` / `plan_launch` (sparc_amd/csrc/wedm_kernels.hip), quoted next to the code
that mirrors them.  The wire lengths come from `build_walk` there: `n1z` (a full tile with exactly one flag change that is
a zone change), `walk_extra` (`n1z`, or a chunk of more than 8 cells with a tail of 1 or 2) and the chunk length C.
"""
from __future__ import annotations

import dataclasses
from typing import FrozenSet, Tuple

from sparc_amd import _abi

K, F = _abi.KERNEL, _abi.FORM

N_ENVS = 100          # not a multiple of 24, 32, 48, 64, 128 or 256: every family's last block is partly dead
TRACE_SIGNALS = ("voltage", "current", "wire_max_temperature")
TRACE_EVERY = 8       # after the bind: the single microsecond (us 1) holds no sample, the launch of 7 (us 2-8) and of 290 do
TRACE_CAPACITY = 64
WIDE_AUTO_MAX_LANES = 65536   # WEDM_WIDE_AUTO_MAX_LANES

# The time grids every recipe runs on: name -> (config.dt [us], config.servo_interval [us]).  On g0 the recipes' 597 steps end
# before the first control step; on g1 and g2 the environments start at staggered `time_since_servo` (`stagger`) and every
# launch gets an action of its own (`action_leaves`), so every launch of every recipe holds control steps.  `plan_launch`
# reads neither value: `Recipe.expected` is the same on every grid.
GRIDS = {"g0": (1, 1000), "g1": (1, 100), "g2": (3, 100)}
ON_TIMES = (2.0, 2.5, 3.0, 4.0)


def steps_per_interval(grid: str) -> int:
    """Physics steps between two latches: the latch tests `time_since_servo >= servo_interval` (wire_edm.py:117)."""
    dt, interval = GRIDS[grid]
    return -(-interval // dt)


def stagger(grid: str, seq: str, n_envs: int):
    """int[n_envs]: `time_since_servo` after the reset, so that environment e first latches in step number
    phase(e) = 7 e mod span of the handle (counted from 0), span = min(steps of the handle's launches, steps between two
    latches): servo_interval - dt * phase, plus e mod dt where dt > 1 (the latch then sees values past the interval).
    Phase 0 starts AT the interval.  Neighbouring lanes of a wave are 7 steps apart: latching and non-latching lanes mix."""
    dt, interval = GRIDS[grid]
    span = min(sum(us for us, _ in SEQS[seq]), steps_per_interval(grid))
    return [interval - dt * ((7 * e) % span) + e % dt for e in range(n_envs)]


def action_leaves(modes, launch: int, n_envs: int):
    """(servo, target voltage, current mode, ON, OFF) of launch number `launch`, one value per environment in every leaf;
    for every environment every leaf differs from its value in the launch before and in launch 0 (ON: four values, the
    offsets 1, 2, 3 in turn; the other leaves differ between any two of a handle's launches, at most 7).
    `modes`: the current modes with crater data."""
    e = range(n_envs)
    servo = [0.05 + 0.002 * ((3 * k + 5 * launch) % 41) + 0.0001 * launch for k in e]
    volt = [70.0 + 0.25 * ((11 * k + 17 * launch) % 120) + 0.01 * launch for k in e]
    mode = [modes[(3 * k + launch) % len(modes)] for k in e]
    on = [ON_TIMES[(k + (1 + (launch - 1) % 3 if launch else 0)) % 4] for k in e]
    off = [10.0 + 0.125 * ((13 * k + 29 * launch) % 160) + 0.01 * launch for k in e]
    return servo, volt, mode, on, off


# launches per handle: (microseconds, trace bound?)
SEQS = {
    "plain": ((1, False), (1, False), (7, False), (290, False), (1, True), (7, True), (290, True)),
    "untraced": ((1, False), (1, False), (7, False), (290, False)),
    # the trace bound before the first launch, whose 8 us hold a sample: a traced launch before any termination was seen
    "trace_first": ((8, True), (290, True)),
    # stencil_mode 1 on the stream kernel: "launches of one microsecond without a trace sample" only
    "singles": ((1, False), (1, False), (1, False)),
    # the batches beyond 65 536 lanes: at most 20 us
    "short": ((1, False), (1, False), (7, False), (1, True), (7, True)),
}


@dataclasses.dataclass(frozen=True)
class Recipe:
    kernel: int                      # forced with set_kernel(kernel, lanes)
    lanes: int
    n_seg: int
    geom: int = 0                    # F.N1 / F.EXTRA / F.CMAX104 / F.CUT: the bit `n_seg` is there for (0: the length without it)
    bind: FrozenSet[str] = frozenset()   # of "pulse", "envp", "wmat", "sig", "f64", "replay"
    seq: str = "plain"
    autoreset: bool = False
    n_envs: int = N_ENVS

    @property
    def id(self) -> str:
        b = "+".join(sorted(self.bind)) or "plain"
        return f"{K(self.kernel).name.lower()}{self.lanes}-n{self.n_seg}-{b}-{self.seq}" + ("-autoreset" if self.autoreset else "") + \
            (f"-{self.n_envs}" if self.n_envs != N_ENVS else "")

    @property
    def oracle_key(self) -> Tuple:
        """What the oracle's half depends on (never the kernel or the lane count)."""
        return (self.n_seg, self.n_envs, self.bind, self.seq, self.autoreset)

    def launches(self):
        """[(microseconds, trace bound, a sample falls into the launch, (kernel, lanes, forms) expected)]"""
        out, pos = [], 0
        for index, (us, traced) in enumerate(SEQS[self.seq]):
            sample = traced and (pos + us) // TRACE_EVERY > pos // TRACE_EVERY
            if traced:
                pos += us
            out.append((us, traced, sample, self.expected(us == 1, sample, index)))
        return out

    def expected(self, single: bool, sample: bool, index: int):
        b, k = self.bind, self.kernel
        # plan_launch: "uint32_t F = (tr ? F_TRACE : 0u) | (f64 ? F_F64 : 0u) | (replay ? F_REPLAY : 0u) | (pulse ? F_PULSE : 0u) |
        #               (envp ? F_ENVP : 0u) | (mat ? F_MAT : 0u) | (sig ? F_SIG : 0u);"
        f = (F.TRACE if sample else 0) | (F.F64 if "f64" in b else 0) | (F.REPLAY if "replay" in b else 0) | \
            (F.PULSE if "pulse" in b else 0) | (F.ENVP if "envp" in b else 0) | (F.MAT if "wmat" in b else 0) | \
            (F.SIG if "sig" in b else 0)
        rows = f & (F.PULSE | F.ENVP | F.MAT | F.SIG)
        # choose_kernel: "const bool fast = !tr && !f64 && !replay; v = fast ? forced : K_GLOBAL;" and
        #                "if ((envp || mat || sig) && pulse) v = K_GLOBAL;"
        if rows and k != K.GLOBAL:
            assert not sample and "f64" not in b and not (rows & F.PULSE and rows & ~F.PULSE), "the launch would run kernel 1"
        # "if (ch.kernel != K_GLOBAL && (F & (F_PULSE | F_ENVP | F_MAT | F_SIG))) F &= ~(F_TRACE | F_F64);"
        if rows and k != K.GLOBAL:
            f &= ~(F.TRACE | F.F64)
        # wedm_step: "frozen_ok = P.autoreset || (ctx->frozen_seen && *ctx->frozen_seen != 0)".  Environment 5 terminates
        # in the first launch; a wave of the second launch "starts with a terminated (frozen) environment" and sets the
        # word (WEDM_REPORT_FROZEN); the test synchronises after every launch, so the third launch reads it.
        frozen = self.autoreset or index >= 2
        if k == K.FUSED:
            # "F |= f64 ? F_FROZEN_OK : (frozen_ok ? F_FROZEN_OK : 0u) | (w->n1z ? F_N1 : 0u);"
            f |= F.FROZEN_OK if "f64" in b else ((F.FROZEN_OK if frozen else 0) | (self.geom & F.N1))
        elif k == K.PACKED:
            # "F |= (frozen_ok ? F_FROZEN_OK : 0u) | (walk_extra(w) ? F_EXTRA : 0u);"
            f |= (F.FROZEN_OK if frozen else 0) | (self.geom & F.EXTRA)
        elif k == K.SERVED:
            assert not sample, "if (v == K_SERVED && tr) v = packed_ok ? K_PACKED : ..."
            f |= self.geom & F.EXTRA   # "F |= walk_extra(w) ? F_EXTRA : 0u;"
        elif k == K.STREAM:
            # "const bool one = single && !tr && w->C <= 64;"
            # "F = (one || f64) ? F_ONE | (F & F_F64) : F | (w->C > 64 ? F_CMAX104 : 0u);"
            one = single and not sample and not (self.geom & F.CMAX104)
            assert one or "f64" not in b, "under stencil_mode 1 the stream kernel runs launches of one microsecond without a trace sample"
            f = (F.ONE | (f & F.F64)) if one else (f | (self.geom & F.CMAX104))
        elif k == K.WIDE:
            # "if ((ctx->p.n_seg & 7) != 0 || tr) F |= F_CUT;"
            assert bool(self.geom & F.CUT) == bool(self.n_seg & 7)
            if (self.geom & F.CUT) or sample:
                f |= F.CUT
            # "if (f64 && (int64_t)n * L > (int64_t)WEDM_WIDE_AUTO_MAX_LANES) F |= F_MINB2;"
            if "f64" in b and self.n_envs * self.lanes > WIDE_AUTO_MAX_LANES:
                f |= F.MINB2
        elif k in (K.LANES_SERVED, K.REGS_SERVED):
            assert not sample, "a trace sample: the unserved forms"
        return (int(k), self.lanes, int(f))


def _subsets(names):
    names = list(names)
    return [frozenset(n for i, n in enumerate(names) if (m >> i) & 1) for m in range(1 << len(names))]


# ------------------------------------------------------------------ wire lengths (build_walk; each with the bit it is there for)
# kernel 3, table of L chunks: n1z.  26 segments: no table of 1 ... 16 chunks has a one-change zone tile.
FUSED_N = {1: {0: 26, F.N1: 71}, 2: {0: 26, F.N1: 71}, 4: {0: 26, F.N1: 71}, 8: {0: 26, F.N1: 71}, 16: {0: 26, F.N1: 143}}
# kernels 4 and 9, table of 2 L chunks: walk_extra.  27 segments: chunks of at most 14 cells without a one-change zone tile
# and tails of 3 to 7 cells or chunks of at most 8; 71 over 2 / 4 / 8 chunks: n1z (and over 8 chunks a chunk of 9: a 1-cell
# tail); 143 over 16 chunks: a chunk of 9 and n1z.
PACKED_N = {1: {0: 27, F.EXTRA: 71}, 2: {0: 27, F.EXTRA: 71}, 4: {0: 27, F.EXTRA: 71}, 8: {0: 27, F.EXTRA: 143}}
# kernel 6, table of L chunks of whole 16-byte words: C = ceil(ceil(n / L) / 4) * 4 in 65 ... 104, else 61 segments (C <= 64)
STREAM_N = {1: {0: 61, F.CMAX104: 101}, 2: {0: 61, F.CMAX104: 170}, 4: {0: 61, F.CMAX104: 301}, 8: {0: 61, F.CMAX104: 601},
            16: {0: 61, F.CMAX104: 1201}}
WIDE_N = {0: 96, F.CUT: 99}          # kernel 8: n_seg & 7
WIDE_BIG_N = {0: 16, F.CUT: 13}      # the same among the 9 to 16 segments of the batches beyond 65 536 lanes
WIDE_BIG_ENVS = {16: 4097, 8: 8193, 4: 16385}   # the smallest batches with num_envs * lanes > 65 536
ANY_N = 99                           # families whose forms do not depend on the table: odd, no multiple of a tile
REGS_N = 99                          # kernels 7 and 12: at most 128 segments
REPLAY_STEPS = 600                   # rows of the injected-variates table: the 597 us of a handle's launches fit


def _catalogue():
    L5, fs = (1, 2, 4, 8, 16), frozenset
    out = {int(k): [] for k in K if k != K.AUTO}
    add = lambda r: out[int(r.kernel)].append(r)  # noqa: E731
    # kernel 1: every subset of TRACE | F64 | PULSE | ENVP | MAT, the same with SIG, and REPLAY with TRACE | PULSE | ENVP
    # (injected variates: a table drawn per environment, read by step and slot on both sides)
    for b in _subsets(("f64", "pulse", "envp", "wmat")):
        add(Recipe(K.GLOBAL, 0, ANY_N, bind=b))
        add(Recipe(K.GLOBAL, 0, ANY_N, bind=b | {"sig"}))
    for b in _subsets(("pulse", "envp")):
        add(Recipe(K.GLOBAL, 0, ANY_N, bind=b | {"replay"}))
    # kernel 2
    for lanes in L5:
        add(Recipe(K.LANES_PK, lanes, ANY_N))
        add(Recipe(K.LANES_PK, lanes, ANY_N, bind=fs({"f64"})))
        for b in ({"pulse"}, {"envp"}, {"wmat"}, {"envp", "wmat"}, {"sig"}, {"sig", "envp"}, {"sig", "wmat"}, {"sig", "envp", "wmat"}):
            add(Recipe(K.LANES_PK, lanes, ANY_N, bind=fs(b), seq="untraced"))
    # kernel 3: without autoreset (no FROZEN_OK before a termination was seen, FROZEN_OK after), traced before and after
    for lanes in L5:
        for bit, n in FUSED_N[lanes].items():
            add(Recipe(K.FUSED, lanes, n, bit))
            add(Recipe(K.FUSED, lanes, n, bit, seq="trace_first"))
        add(Recipe(K.FUSED, lanes, FUSED_N[lanes][F.N1], F.N1, autoreset=True))
        add(Recipe(K.FUSED, lanes, FUSED_N[lanes][F.N1], F.N1, bind=fs({"f64"})))
    # kernel 4
    for lanes in (1, 2, 4, 8):
        for bit, n in PACKED_N[lanes].items():
            add(Recipe(K.PACKED, lanes, n, bit))
            add(Recipe(K.PACKED, lanes, n, bit, seq="trace_first"))
        add(Recipe(K.PACKED, lanes, PACKED_N[lanes][F.EXTRA], F.EXTRA, autoreset=True))
    add(Recipe(K.SPLIT, 0, ANY_N))
    # kernel 6
    for lanes in L5:
        for bit, n in STREAM_N[lanes].items():
            add(Recipe(K.STREAM, lanes, n, bit))
        add(Recipe(K.STREAM, lanes, STREAM_N[lanes][0], bind=fs({"f64"}), seq="singles"))
    # kernel 7
    for lanes in (1, 2):
        add(Recipe(K.REGS, lanes, REGS_N))
        add(Recipe(K.REGS, lanes, REGS_N, bind=fs({"f64"})))
        add(Recipe(K.REGS, lanes, REGS_N, bind=fs({"pulse"}), seq="untraced"))
    # kernel 8
    for lanes in (4, 8, 16):
        for bit, n in WIDE_N.items():
            add(Recipe(K.WIDE, lanes, n, bit))
            add(Recipe(K.WIDE, lanes, n, bit, bind=fs({"f64"})))
            add(Recipe(K.WIDE, lanes, n, bit, bind=fs({"pulse"}), seq="untraced"))
        for bit, n in WIDE_BIG_N.items():
            add(Recipe(K.WIDE, lanes, n, bit, bind=fs({"f64"}), seq="short", n_envs=WIDE_BIG_ENVS[lanes]))
    # kernels 9, 11, 12: no trace point
    for lanes in (4, 8):
        for bit, n in PACKED_N[lanes].items():
            add(Recipe(K.SERVED, lanes, n, bit, seq="untraced"))
    for lanes in L5:
        add(Recipe(K.LANES, lanes, ANY_N))
        add(Recipe(K.LANES, lanes, ANY_N, bind=fs({"f64"})))
    for lanes in (4, 8, 16):
        add(Recipe(K.LANES_SERVED, lanes, ANY_N, seq="untraced"))
    add(Recipe(K.REGS_SERVED, 0, REGS_N, seq="untraced"))
    return out


CATALOGUE = _catalogue()   # kernel number -> its recipes

# Registry entries that no shape and no setting makes plan_launch select: (kernel, lanes, forms) -> the lines of
# choose_kernel / plan_launch that exclude it.  At most 8 (3 % of the registry): beyond that the dead entries leave the
# registry instead.
UNREACHABLE: dict = {}
MAX_UNREACHABLE = 8


def form_names(forms: int) -> str:
    return " | ".join(f"F_{b.name}" for b in F if forms & b) or "none"


def describe(entry) -> str:
    k, lanes, forms = entry
    return f"{K(k).name}<{lanes}> {form_names(forms)}"


def expected_entries(kernel: int) -> set:
    return {e for r in CATALOGUE[int(kernel)] for _, _, _, e in r.launches()}
