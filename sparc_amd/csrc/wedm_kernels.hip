// wedm_kernels.hip — the translation unit(s) of libwedm_hip.so: includes the kernel families, lists their instantiations in one
// registry (compiled in six parts in parallel), and holds the host side of the C-ABI of include/wedm_hip.h (launch plan,
// wedm_create ...).
//
// Device code, by file (DESIGN.md section 4 has the table with what binds each kernel):
//   wedm_device.h         per-lane physics of one microsecond: Env, prelude (quiet / general), epilogue (monitor + motion),
//                         stencil_cell
//   wedm_portable.h       what of it is pure arithmetic: the portable exp / log / cube, CPython's float `//`, Philox and its
//                         variates; wedm_device.h includes it, and so do the families outside the registry that need nothing
//                         else of the physics (wedm_head.h, wedm_geometry.h, wedm_randomize.h, wedm_minibatch.h)
//   wedm_env_rows.h       which Env member holds which state row, when it is final, whether a step reads it and whether a
//                         reference-semantics reset keeps it: the lists load_env / store_env / the trace are expanded from
//   wedm_common.h         build switches, WalkTable, KArgs, trace point, wire accessors, the LDS images' slot maps (ChunkSlot,
//                         PackedSlot) and the block copy of the wire that takes them (copy_wire: every LDS kernel, served or
//                         not), tile_staged / quad_staged
//   wedm_lifecycle.h      an environment's launch lifecycle, each part written once as text the kernels expand (WEDM_ENV_LOAD /
//                         _RESET / _START, _END_US / _STEP_DONE, _CLOSE) and the helpers that wrap it (env_open / env_start,
//                         env_end_us / env_step_done, env_close); launch_hot, stencil_f64_consts (the file's head says who
//                         expands what)
//   wedm_k_global_split.h wedm_step_global (in place in global memory; stencil_mode 1, injected variates, very long wires),
//                         wedm_step_split (single microseconds where the stream kernel does not fit)
//   wedm_k_stream.h       wedm_step_stream<L>: single microseconds (the reference's step() cadence), uniform geometry
//   wedm_k_lanes.h        wedm_step_lanes<L>: any geometry, cell by cell (kernel 10; stencil_mode 1)
//   wedm_lanes2.h         wedm_step_lanes_pk<L>: any geometry, packed float32 walk (kernel 2: BASELINE config 5), and its served form
//   wedm_k_fused.h        wedm_step_fused<L>: uniform geometry, wire chunks in LDS, wave-uniform tile table
//   wedm_fused_walk.inc   the one-chunk LDS walk itself (one microsecond: halos, patched cells, tiles, patches, reduction, trace
//                         point), included as text by wedm_step_fused and by the LDS walk of wedm_step_stream
//   wedm_k_packed.h       wedm_step_packed<L>: the same with two virtual chunks per lane in float2 registers
//   wedm_packed_walk.inc  the packed LDS walk itself (per-lane tile flags; one microsecond: halos, tiles, patches), included as
//                         text by wedm_step_packed and by the walkers of wedm_step_served
//   wedm_served.h         wedm_step_served<L>: the packed walk on three waves of a block, the scalar physics of the block's
//                         environments on the fourth, one microsecond ahead (kernel 9: large batches of long wires); the
//                         LDS mailbox between them and both sides of its protocol, each written once (served_scalar_wave;
//                         WEDM_SV_BOX_INIT / _WAIT_COEF / _TAKE, sv_give, sv_walker_reinit, sv_stamp_row), which
//                         wedm_step_lanes_served (wedm_lanes2.h) and wedm_step_regs_served (here) run as well
//   wedm_k_regs.h         wedm_step_regs<L> (the headline: the wire in the registers of two lanes per environment),
//                         wedm_step_regs_wide<L> (4 / 8 / 16 lanes of a DPP row per environment: small batches)
//                         and, as text (WEDM_REGS_*), what both and wedm_step_regs_served do with the wire around the loop
//   wedm_copy.h           wedm_copy_columns_kernel: environments' columns between or within caller-owned blocks (snapshot,
//                         restore, fork); not a step kernel, not in the registry
//   wedm_profile.h        wedm_wire_profile_kernel: every named environment's wire reduced to zone mean, mean, maximum, hottest
//                         cell and pooled bins; not a step kernel, not in the registry
//   wedm_geometry.h       wedm_derive_geometry_kernel: masked environments' geometry rows derived from (height, diameter
//                         index, material index) with the host derivation's bits; not a step kernel, not in the registry
//   wedm_randomize.h      wedm_draw_episode_kernel: masked environments' physics parameters, material, height and diameter of
//                         their next episode drawn from (seed, global id, draw number) and written with every row that depends
//                         on them; not a step kernel, not in the registry
//   wedm_normalize.h      wedm_norm_reduce / _fold / _apply_kernel: running observation and reward normalisation over all
//                         environments by a fixed pairwise tree, episode statistics; not step kernels, not in the registry
//   wedm_gae.h            wedm_gae_scan / _fold / _apply_kernel: a rollout's advantages, returns, valid mask and standardised
//                         advantages, the time loop in the lane, moments by the same tree; not step kernels, not in the registry
//   wedm_head.h           wedm_head_kernel: a policy's action head (squashed Gaussians and a categorical) -- a seeded draw, its
//                         log-probability and entropy, their gradient; one lane per row; not a step kernel, not in the registry
//   wedm_ppo.h            wedm_ppo_count / _main / _fold_kernel: PPO's clipped loss over a minibatch -- the row's terms, their
//                         means by a fixed pairwise tree over the row number, the gradient; not step kernels, not in the registry
//   wedm_policy_net.h     wedm_net_kernel / wedm_net_fold_kernel: a two-hidden-layer actor-critic MLP, forward and backward as
//                         k-ordered fma chains on the float32 MFMA, the gradient's row sum by the same tree; not in the registry
//   wedm_adam.h           wedm_adam_norm / _decide / _apply_kernel and wedm_adam_one_kernel: Adam with global-norm clipping and a
//                         KL gate over one flat parameter block, the norm by the same tree; not step kernels, not in the registry
//   wedm_minibatch.h      wedm_mb_count / _offsets / _scatter_kernel: a rollout's rows dealt into minibatches by a seeded keyed
//                         bijection of the live rows' ranks, dead rows last in every part; not step kernels, not in the registry
//   wedm_eplog.h          wedm_elog_count / _scatter / _commit_kernel: the finished episodes of a control step appended to a ring
//                         in the order of the global environment index, per-episode sums; not step kernels, not in the registry
//   wedm_reward.h         wedm_reward_kernel: a control step's shaped reward, ten weighted terms of the state blocks (the *_ACC
//                         rows) summed in a fixed order, one lane per environment; not a step kernel, not in the registry
//   wedm_sensor.h         wedm_sensor_kernel: what a machine measures of the observation -- per channel a delayed source column,
//                         the episode's gain and offset error, fresh noise, quantisation, saturation --, one lane per
//                         environment, includes wedm_portable.h alone; not a step kernel, not in the registry
// Host code, in this file's part 0: the launch plan and the entry points that take a handle, then the fourteen stateless entry
// points (wedm_copy_columns ... wedm_sensor) behind what they share, each written once above wedm_copy_columns:
//   Entry                 the entry point's name: bad(msg) refuses with "<name>: <msg>", launched([what]) reports a launch
//   Block, check_blocks   a call's memory by name, inputs and outputs: null or misaligned, then an output on an input
//                         (wedm_gae, wedm_policy_head, wedm_ppo_loss, wedm_policy_net, wedm_adam, wedm_minibatch_index,
//                         wedm_episode_log, wedm_reward, wedm_sensor); check_apart: every written block against every other
//                         one (wedm_adam, wedm_minibatch_index, wedm_reward, wedm_sensor)
//   tile_range, fold_per, fold_padded   the tile range inside the workspace and its tile count; the tiles per lane of a
//                         256-lane fold; the leaves of a pairwise tree over the tiles
//   check_head_params, StagedRows   n_modes, strides and bounds of a head; which rows go through LDS and the LDS for it
//                         (wedm_policy_head, wedm_ppo_loss)
// The wire block is quad-interleaved, T[seg >> 2][env][seg & 3] (include/wedm_hip.h, ABI v4): a lane that owns a run of
// segments of one environment moves it with global_load / store_dwordx4, a wavefront still touches contiguous 1-KB runs.
// Every kernel is a template <int L, uint32_t F> (or <uint32_t F>) over its lanes per environment and a set of form bits (F_*
// of wedm_device.h: signal trace point, FROZEN_OK for autoreset handles, N1 / EXTRA for tile tables with one-change tiles or
// short tails, the bound per-environment blocks ...): code that costs the other launches 1-2 % by its mere presence lives in
// its own form.  The registry below lists the instantiations; plan_launch() computes a launch's form and looks it up there.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math (see
// __graft_entry__.build()).  -ffp-contract=off is part of the numerics contract.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstddef>
#include <type_traits>
#include <utility>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>
#include <string>

#include "wedm_device.h"

using namespace wedm;

#include "wedm_common.h"
#include "wedm_k_global_split.h"
#include "wedm_k_lanes.h"
#include "wedm_k_fused.h"
#include "wedm_k_stream.h"
#include "wedm_k_regs.h"
#include "wedm_k_packed.h"
#include "wedm_served.h"
#include "wedm_lanes2.h"
#if !defined(WEDM_PART) || WEDM_PART == 0
#include "wedm_copy.h"
#include "wedm_profile.h"
#include "wedm_geometry.h"
#include "wedm_randomize.h"
#include "wedm_normalize.h"
#include "wedm_gae.h"
#include "wedm_head.h"
#include "wedm_ppo.h"
#include "wedm_policy_net.h"
#include "wedm_adam.h"
#include "wedm_minibatch.h"
#include "wedm_eplog.h"
#include "wedm_reward.h"
#include "wedm_sensor.h"
#endif

// ------------------------------------------------------------ the registry of instantiations
// Every instantiation of a step kernel, written once as data: per family its lane counts and its forms.  They are 317
// (wedm_debug_registry counts them), which take hipcc minutes in one translation unit, so __graft_entry__.build_hip() compiles this file six times in
// parallel (__graft_entry__.BUILD_UNITS lists the six): -DWEDM_PART=N defines registry_partN(), which instantiates what it lists (1: the packed kernel, 2: the fused
// kernel, 3: the served kernels and kernel 2's float32 forms, 4: the float64-typed forms of kernels 2, 6, 7 and 8 and the
// PULSE forms of 7 and 8, 5: the SIG forms of kernels 1 and 2, 0: the rest); -DWEDM_PART=0 also holds the host code and the
// reset and debug kernels, and registry() there joins the six slices.  The six objects link into the one shared library.  Without -DWEDM_PART the file
// is one self-contained translation unit (the diagnostic builds of tools/ use it that way).

// kernel numbers of wedm_set_kernel (include/wedm_hip.h; the ABI carries them as int32_t)
enum Kernel : int32_t {
    K_AUTO = 0, K_GLOBAL = 1, K_LANES_PK = 2, K_FUSED = 3, K_PACKED = 4, K_SPLIT = 5, K_STREAM = 6, K_REGS = 7, K_WIDE = 8,
    K_SERVED = 9, K_LANES = 10, K_LANES_SERVED = 11, K_REGS_SERVED = 12
};

struct KernelForm {
    Kernel kernel;
    int lanes;       // lanes per environment (0: a family without that choice)
    uint32_t forms;  // F_* bits
    const void* fn;
};
typedef std::vector<KernelForm> Slice;

// kernel K's instantiation for (L, F)
template <Kernel K, int L, uint32_t F> static const void* instantiation() {
    if constexpr (K == K_GLOBAL) return (const void*)wedm_step_global<F>;
    else if constexpr (K == K_LANES_PK) return (const void*)wedm_step_lanes_pk<L, F>;
    else if constexpr (K == K_FUSED) return (const void*)wedm_step_fused<L, F>;
    else if constexpr (K == K_PACKED) return (const void*)wedm_step_packed<L, F>;
    else if constexpr (K == K_SPLIT) return (const void*)wedm_step_split<F>;
    else if constexpr (K == K_STREAM) return (const void*)wedm_step_stream<L, F>;
    else if constexpr (K == K_REGS) return (const void*)wedm_step_regs<L, F>;
    else if constexpr (K == K_WIDE) return (const void*)wedm_step_regs_wide<L, F>;
    else if constexpr (K == K_SERVED) return (const void*)wedm_step_served<L, F>;
    else if constexpr (K == K_LANES) return (const void*)wedm_step_lanes<L, F>;
    else if constexpr (K == K_LANES_SERVED) return (const void*)wedm_step_lanes_served<L, F>;
    else {
        static_assert(K == K_REGS_SERVED, "a kernel family");
        return (const void*)wedm_step_regs_served<F>;
    }
}

template <int... Ls> using Lanes = std::integer_sequence<int, Ls...>;
template <uint32_t... Fs> using Forms = std::integer_sequence<uint32_t, Fs...>;
using L5 = Lanes<1, 2, 4, 8, 16>;
using NoLanes = Lanes<0>;
// subset i of the bits of `set` (bit b of i selects the b-th lowest bit of `set`)
constexpr uint32_t subset(uint32_t set, uint32_t i) {
    uint32_t r = 0;
    for (; set; set &= set - 1, i >>= 1)
        if (i & 1u) r |= set & (0u - set);
    return r;
}
template <uint32_t SET, uint32_t WITH, uint32_t... I>
Forms<(WITH | subset(SET, I))...> subsets(std::integer_sequence<uint32_t, I...>);
// every subset of the bits of SET, each with the bits of WITH
template <uint32_t SET, uint32_t WITH = 0>
using Every = decltype(subsets<SET, WITH>(std::make_integer_sequence<uint32_t, 1u << __builtin_popcount(SET)>{}));

// appends kernel K's instantiations for every L of Ls and every F of Fs
template <Kernel K, int... Ls, uint32_t... Fs>
static void add(Slice& s, Lanes<Ls...>, Forms<Fs...>) {
    const auto with_lanes = [&](auto l) {
        constexpr int L = decltype(l)::value;
        (s.push_back({K, L, Fs, instantiation<K, L, Fs>()}), ...);
    };
    (with_lanes(std::integral_constant<int, Ls>{}), ...);
}

Slice registry_part0();
Slice registry_part1();
Slice registry_part2();
Slice registry_part3();
Slice registry_part4();
Slice registry_part5();

#if !defined(WEDM_PART) || WEDM_PART == 1
Slice registry_part1() {
    Slice s;
    add<K_PACKED>(s, Lanes<1, 2, 4, 8>{}, Every<F_TRACE | F_FROZEN_OK | F_EXTRA>{});
    return s;
}
#endif

#if !defined(WEDM_PART) || WEDM_PART == 2
Slice registry_part2() {
    Slice s;
    add<K_FUSED>(s, L5{}, Every<F_TRACE | F_FROZEN_OK | F_N1>{});
    add<K_FUSED>(s, L5{}, Every<F_TRACE, F_FROZEN_OK | F_F64>{});  // stencil_mode 1 on the tile walk
    return s;
}
#endif

#if !defined(WEDM_PART) || WEDM_PART == 3
Slice registry_part3() {
    Slice s;
    add<K_LANES_PK>(s, L5{}, Forms<0, F_TRACE, F_PULSE, F_ENVP, F_MAT, F_ENVP | F_MAT>{});
    add<K_SERVED>(s, Lanes<4, 8>{}, Every<F_EXTRA>{});
    add<K_LANES_SERVED>(s, Lanes<4, 8, 16>{}, Forms<0>{});
    add<K_REGS_SERVED>(s, NoLanes{}, Forms<0>{});
    return s;
}
#endif

#if !defined(WEDM_PART) || WEDM_PART == 4
Slice registry_part4() {
    Slice s;
    add<K_LANES_PK>(s, L5{}, Every<F_TRACE, F_F64>{});
    add<K_STREAM>(s, L5{}, Forms<F_ONE | F_F64>{});
    add<K_REGS>(s, Lanes<1, 2>{}, Forms<F_F64, F_TRACE | F_F64, F_PULSE>{});
    // the float64 wide forms at one or two blocks per CU; a traced launch runs the CUT form
    add<K_WIDE>(s, Lanes<4, 8, 16>{}, Every<F_CUT | F_MINB2, F_F64>{});
    add<K_WIDE>(s, Lanes<4, 8, 16>{}, Every<F_MINB2, F_CUT | F_TRACE | F_F64>{});
    add<K_WIDE>(s, Lanes<4, 8, 16>{}, Every<F_CUT, F_PULSE>{});
    return s;
}
#endif

#if !defined(WEDM_PART) || WEDM_PART == 5
// signal statistics (wedm_bind_signal_stats): kernel 1 with every other binding but injected variates, kernel 2's packed
// form with or without the per-environment rows
Slice registry_part5() {
    Slice s;
    add<K_GLOBAL>(s, NoLanes{}, Every<F_TRACE | F_F64 | F_PULSE | F_ENVP | F_MAT, F_SIG>{});
    add<K_LANES_PK>(s, L5{}, Every<F_ENVP | F_MAT, F_SIG>{});
    return s;
}
#endif

#if !defined(WEDM_PART) || WEDM_PART == 0
Slice registry_part0() {
    Slice s;
    add<K_GLOBAL>(s, NoLanes{}, Every<F_TRACE | F_F64 | F_PULSE | F_ENVP | F_MAT>{});
    add<K_GLOBAL>(s, NoLanes{}, Every<F_TRACE | F_PULSE | F_ENVP, F_REPLAY>{});  // injected variates: float32, no MAT
    add<K_LANES>(s, L5{}, Every<F_TRACE | F_F64>{});
    add<K_STREAM>(s, L5{}, Every<F_TRACE | F_CMAX104>{});
    add<K_STREAM>(s, L5{}, Forms<F_ONE>{});
    add<K_SPLIT>(s, NoLanes{}, Every<F_TRACE>{});
    add<K_REGS>(s, Lanes<1, 2>{}, Every<F_TRACE>{});
    add<K_WIDE>(s, Lanes<4, 8, 16>{}, Forms<0, F_CUT, F_CUT | F_TRACE>{});
    return s;
}

// every instantiation: the slices of the six parts
static const Slice& registry() {
    static const Slice all = [] {
        Slice a;
        for (Slice (*part)() : {registry_part0, registry_part1, registry_part2, registry_part3, registry_part4, registry_part5}) {
            const Slice s = part();
            a.insert(a.end(), s.begin(), s.end());
        }
        return a;
    }();
    return all;
}
// kernel k's instantiation for L lanes per environment and the forms F; nullptr if there is none
static const void* find_instantiation(Kernel k, int L, uint32_t F) {
    for (const KernelForm& f : registry())
        if (f.kernel == k && f.lanes == L && f.forms == F) return f.fn;
    return nullptr;
}
// kernel k (as wedm_set_kernel numbers it) has a form with the bit `form`; kernel 0, the automatic choice, has every form
static bool has_form(int32_t k, uint32_t form) {
    if (k == K_AUTO) return true;
    for (const KernelForm& f : registry())
        if (f.kernel == k && (f.forms & form)) return true;
    return false;
}
// the F_* bits' names, by bit number (wedm_debug_form_name hands them out: tests/test_registry_host.py ties them to the enum)
static const char* const form_bit_names[] = {"TRACE", "F64", "REPLAY", "PULSE", "ENVP", "MAT", "FROZEN_OK",
                                             "N1", "EXTRA", "CUT", "ONE", "CMAX104", "MINB2", "SIG"};
static std::string form_names(uint32_t F) {
    std::string s;
    for (int b = 0; b < (int)(sizeof(form_bit_names) / sizeof(form_bit_names[0])); ++b)
        if ((F >> b) & 1u) s += (s.empty() ? "F_" : " | F_") + std::string(form_bit_names[b]);
    return s.empty() ? "none" : s;
}

__global__ void __launch_bounds__(256)
wedm_reset_kernel(const wedm_params p, const wedm_state_ptrs s, int32_t num_envs, int32_t n_seg_max,
                  const uint8_t* mask, uint32_t key_lo, uint32_t key_hi, int32_t reseed) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= num_envs) return;
    if (mask && !mask[e]) return;
    const int64_t stride = s.stride;
    int32_t episode = *WEDM_ROW(s.i32, WEDM_I_EPISODE);
    int32_t klo = *WEDM_ROW(s.i32, WEDM_I_KEY_LO), khi = *WEDM_ROW(s.i32, WEDM_I_KEY_HI);
    // reset_semantics 1 = the reference's own reset(): a new EDMState only (wire_edm.py:106-114).  The rows that mirror what
    // its MODULE objects hold survive: `prev_accel` (mechanics.py:60), the debris volume and the flow / density caches
    // (dielectric.py:69-80), the convection cache and coefficients (wire.py:205,224), the short timers and the current
    // cache (ignition.py:75-81), the crater list and its statistics (material.py:133).
    const bool keep_modules = p.reset_semantics != 0 && !(reseed & WEDM_RESET_FRESH);
    // (which rows those are: the `owner` column of wedm_env_rows.h)
    constexpr uint32_t module_f64 = WEDM_F64_ROWS(ROW_MODULE) WEDM_UNHELD_F64(WEDM_UNHELD_MODULE_BIT),
                       module_i32 = WEDM_I32_ROWS(ROW_MODULE) WEDM_UNHELD_I32(WEDM_UNHELD_MODULE_BIT),
                       module_i8 = WEDM_I8_ROWS(ROW_MODULE) WEDM_UNHELD_I8(WEDM_UNHELD_MODULE_BIT);
    for (int f = 0; f < WEDM_F64_COUNT; ++f)
        if (!(keep_modules && ((module_f64 >> f) & 1u))) *WEDM_ROW(s.f64, f) = 0.0;
    for (int f = 0; f < WEDM_I32_COUNT; ++f)
        if (!(keep_modules && ((module_i32 >> f) & 1u))) *WEDM_ROW(s.i32, f) = 0;
    for (int f = 0; f < WEDM_I8_COUNT; ++f)
        if (!(keep_modules && ((module_i8 >> f) & 1u))) *WEDM_ROW(s.i8, f) = 0;
    if (s.stats && !keep_modules) {
        *WEDM_ROW(s.stats, WEDM_S_CRATER_SUM) = 0.0; *WEDM_ROW(s.stats, WEDM_S_CRATER_SUMSQ) = 0.0;
        *WEDM_ROW(s.stats, WEDM_S_CRATER_MIN) = __builtin_inf(); *WEDM_ROW(s.stats, WEDM_S_CRATER_MAX) = -__builtin_inf();
    }
    if (reseed & WEDM_RESET_RESEED) {
        *WEDM_ROW(s.i32, WEDM_I_EPISODE) = 0;
        *WEDM_ROW(s.i32, WEDM_I_KEY_LO) = (int32_t)key_lo;
        *WEDM_ROW(s.i32, WEDM_I_KEY_HI) = (int32_t)key_hi;
    } else {
        *WEDM_ROW(s.i32, WEDM_I_EPISODE) = episode + 1;
        *WEDM_ROW(s.i32, WEDM_I_KEY_LO) = klo;
        *WEDM_ROW(s.i32, WEDM_I_KEY_HI) = khi;
    }
    // state.current_mode = None: 0, or -1 where the surviving module's current cache names a mode (ignition.py:98-113:
    // None then resolves through default_current_mode instead of the fresh cache's 60 A)
    if (keep_modules && *WEDM_ROW(s.i8, WEDM_B_MODE_CACHED)) *WEDM_ROW(s.i32, WEDM_I_CURRENT_MODE) = -1;
    *WEDM_ROW(s.f64, WEDM_F_WORKPIECE_POS) = p.initial_gap;            // wire_edm.py:111
    *WEDM_ROW(s.f64, WEDM_F_TARGET_POS) = p.target_cutting_distance;   // wire_edm.py:112
    *WEDM_ROW(s.f64, WEDM_F_UNWIND_VEL) = 0.2;                         // state.py:55
    *WEDM_ROW(s.f64, WEDM_F_SPARK_Y) = __builtin_nan("");              // [0, None, 0]
    if (!keep_modules) {
        *WEDM_ROW(s.f64, WEDM_F_LAST_GAP) = -1.0;                      // dielectric.py:78
        *WEDM_ROW(s.f64, WEDM_F_LAST_DENSITY) = -1.0;                  // dielectric.py:79
    }
    const float spool = (float)p.spool_T;
    *WEDM_ROW(s.f64, WEDM_F_TMAX) = (double)spool;
    for (int q = 0; q < WEDM_T_QUADS(n_seg_max); ++q)  // wire.py:264-269 (whole 16-byte words: padding cells included)
        *(f4v*)(s.T + (((int64_t)q * stride + e) << 2)) = f4v{spool, spool, spool, spool};
    if (s.obs)
        for (int c = 0; c < p.obs_dim; ++c) s.obs[(int64_t)c * stride + e] = 0.0f;
    if (s.reward) s.reward[e] = 0.0f;
}

// wedm_reset's part for the pulse-statistics block (wedm_bind_pulse_stats): its own launch, so that wedm_reset_kernel stays as
// it is for handles without the block
__global__ void __launch_bounds__(256)
wedm_reset_pulse_kernel(int32_t* rows, int64_t stride, int32_t num_envs, const uint8_t* mask) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= num_envs) return;
    if (mask && !mask[e]) return;
    for (int q = 0; q < WEDM_PULSE_COUNT; ++q) *WEDM_ROW(rows, q) = 0;
}

// wedm_reset's part for the signal-statistics block (wedm_bind_signal_stats), in its own launch for the same reason: the
// accumulators to their identities, the published rows to zero
__global__ void __launch_bounds__(256)
wedm_reset_signal_kernel(double* rows, int64_t stride, int32_t num_envs, const uint8_t* mask) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= num_envs) return;
    if (mask && !mask[e]) return;
    for (int q = 0; q < WEDM_SIG_COUNT; ++q) *WEDM_ROW(rows, q) = 0.0;
    *WEDM_ROW(rows, WEDM_SG_GAP_MIN_ACC) = __builtin_inf();
    *WEDM_ROW(rows, WEDM_SG_TMAX_PEAK_ACC) = -__builtin_inf();
}

// Probe of the device math the physics relies on (test hook; see wedm_debug_math).
__global__ void wedm_debug_math_kernel(int32_t kind, const double* a, const double* b, double* out, int32_t n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = a[i], y = b ? b[i] : 0.0;
    double r = 0.0;
    switch (kind) {
        case 0: r = portable_exp(x); break;
        case 1: r = portable_log(x); break;
        case 2: r = cube_cr(x); break;
        case 3: r = sqrt(x); break;
        case 4: r = py_floordiv(x, y); break;
        case 5: r = x / y; break;
        case 6: {  // x = time, y = env id, key fixed; all four step uniforms observable
            W4 w = philox4(0x12345678u, 0x9abcdef0u, (uint32_t)x, 3u, (uint32_t)y, 0u);
            r = u32_to_unit(w.x) + 2.0 * u32_to_unit(w.y) + 4.0 * u32_to_unit(w.z) + 8.0 * u32_to_unit(w.w);
            break;
        }
        case 7: r = philox_std_normal(0x12345678u, 0x9abcdef0u, (uint32_t)x, 3u, (uint32_t)y); break;
        case 8: r = (double)spark_cell_offset(x, y); break;
        default: break;
    }
    out[i] = r;
}

// Fills every CU's LDS with `value` (test hook; see wedm_debug_poison_lds): rows of the LDS image that a kernel never
// stages (cells past a wire's end) then hold a conspicuous value instead of whatever the previous kernel left there.
__global__ void __launch_bounds__(256) wedm_debug_poison_lds_kernel(float value, int32_t n_floats) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    for (int i = threadIdx.x; i < n_floats; i += 256) lds[i] = value;
    __syncthreads();
    if (lds[(threadIdx.x * 97) % n_floats] != value) __builtin_trap();  // keeps the stores observable
}

// =================================================================== C-ABI
struct LaunchPlan {
    bool valid = false;
    const void* fn = nullptr;
    int grid = 0;
    int block = 256;
    size_t lds = 0;
    const WalkTable* walk = nullptr;
    char name[160] = {0};
    // the registry entry `fn` is (wedm_debug_last_form)
    int32_t kernel = 0, lanes = 0;
    uint32_t forms = 0;
};

// What the planner knows of a walk table (wedm_create builds them; wedm_ctx::walk_dev holds the tables, same index).
struct WalkInfo {
    bool ok = false;      // built: the chunk and its halo row fit WEDM_MAX_C
    int32_t C = 0;        // cells per chunk
    uint32_t kind_s = 0;  // tiles with several flag changes (the stream kernel's register walk has no code for them)
    bool n1z = false;     // a one-change tile with a zone change (see WalkTable::kind_n1_mask)
};
// walk table indices: L = 1, 2, 4, 8, 16 chunks (LDS kernels) from W_LDS, the same with chunks of whole 16-byte words (stream
// kernel) from W_STREAM, two chunks of exactly 64 cells and four of 32 (register kernels)
enum : int { W_LDS = 0, W_STREAM = 5, W_REGS2 = 10, W_REGS4 = 11, W_COUNT = 12 };

struct wedm_ctx {
    wedm_params p;
    int32_t num_envs = 0, n_seg_max = 0;
    int device = -1;
    bool bound = false, geom_bound = false;
    wedm_state_ptrs s{};
    wedm_geom_ptrs g{};
    void* tables_dev = nullptr;
    wedm_params* params_dev = nullptr;  // "cold" parameters, read through rare branches only
    Tables tb{};
    int32_t variant = 0;
    int32_t lanes = 0;                 // lanes per environment for the fused kernel (0 = auto)
    unsigned long long* dbg = nullptr; // diagnostic builds: phase stamp buffer
    int lds_limit = 0;
    WalkTable* walk_dev = nullptr;     // [W_COUNT] walk tables (uniform geometry only)
    WalkInfo walk[W_COUNT];
    // signal trace (wedm_bind_trace): descriptor, microseconds stepped and samples written since the bind
    const double* replay = nullptr;    // wedm_bind_rng_replay
    int64_t replay_steps = 0;
    bool trace_on = false;
    wedm_trace_desc trace{};
    int64_t trace_us = 0, trace_count = 0;
    int32_t* pulse = nullptr;          // wedm_bind_pulse_stats: [WEDM_PULSE_COUNT][stride] or NULL
    const double* envp = nullptr;      // wedm_bind_env_params: [WEDM_ENVP_COUNT][stride] or NULL
    const double* wmat = nullptr;      // wedm_bind_wire_material: [WEDM_WMAT_COUNT][stride] or NULL
    double* sig = nullptr;             // wedm_bind_signal_stats: [WEDM_SIG_COUNT][stride] or NULL
    std::string err;
    std::string last_kernel;
    LaunchPlan plans[2][2][2];         // [single microsecond][trace point][frozen-lane tile code]: cached launch decisions
    int32_t* frozen_seen = nullptr;    // pinned host word the kernels set (Cold::frozen_seen), and its device alias
    int32_t* frozen_seen_dev = nullptr;
    const LaunchPlan* last_plan = nullptr;
    int32_t last_n_sub = 0;
    void invalidate_plans() { for (auto& a : plans) for (auto& b : a) for (auto& pl : b) pl.valid = false; }
};

static int32_t fail(wedm_ctx* ctx, int32_t code, const std::string& msg) {
    if (ctx) ctx->err = msg;
    return code;
}
static int32_t hip_fail(wedm_ctx* ctx, hipError_t e, const char* what) {
    return fail(ctx, WEDM_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}


// Walk table for L lanes per environment (uniform geometry): for every chunk-local cell j
// which chunks have that cell inside the zone / between the contacts / interior / valid, and
// per 8-cell tile whether it needs the per-cell (SPECIAL) path.
// `align`: the chunk length is rounded up to a multiple of it (4 for the stream kernel, whose lanes load their chunk in
// 16-byte words of the quad-interleaved block: every chunk then starts on a word; chunks may end up partly or wholly
// past the wire's end, which the valid / interior masks express like any ragged tail).
static bool build_walk(const wedm_params& p, int L, WalkTable& t, int align = 1) {
    std::memset(&t, 0, sizeof(t));
    const int n = p.n_seg;
    const int C = ((n + L - 1) / L + align - 1) / align * align;
    if (C + 1 > WEDM_MAX_C) return false;  // +1: the halo row
    const int cb = p.contact_bottom, ct = p.contact_top, zs = p.az_start, ze = p.az_end;
    t.C = C;
    t.n_tiles = (C + 7) / 8;
    const uint16_t all = (uint16_t)((1u << L) - 1u);
    for (int j = 0; j < t.n_tiles * 8; ++j) {
        uint16_t zone = 0, joule = 0, inter = 0, valid = 0;
        for (int c = 0; c < L && j < C; ++c) {
            const int i = c * C + j;
            if (zs < ze && i >= zs && i < ze) zone |= (uint16_t)(1u << c);
            if (i >= cb && i <= ct) joule |= (uint16_t)(1u << c);
            if (i >= 1 && i <= n - 2) inter |= (uint16_t)(1u << c);
            if (i < n) valid |= (uint16_t)(1u << c);
        }
        t.zj[j] = (uint32_t)zone | ((uint32_t)joule << 16);
        t.iv[j] = (uint32_t)inter | ((uint32_t)valid << 16);
    }
    for (int tile = 0; tile < t.n_tiles; ++tile) {
        const int j0 = 8 * tile, j1 = std::min(j0 + 8, C);
        bool all_interior = (j1 - j0 == 8);
        int changes = 0, split = 8;
        for (int j = j0; j < j1; ++j) {
            if ((t.iv[j] & 0xffffu) != all) all_interior = false;
            if (j > j0 && t.zj[j] != t.zj[j - 1]) { ++changes; split = j - j0; }
        }
        // regular apart from the wire's two end cells / apart from the contact flag?
        bool ends_only = (j1 - j0 == 8);
        int zone_changes = 0;
        for (int j = j0; j < j1; ++j) {
            uint16_t ends = 0;
            for (int c = 0; c < L; ++c) {
                const int i = c * C + j;
                if (i == 0 || i == n - 1) ends |= (uint16_t)(1u << c);
            }
            if ((t.iv[j] >> 16) != all) ends_only = false;                          // a cell past the wire's end
            if ((uint16_t)((t.iv[j] & 0xffffu) | ends) != all) ends_only = false;   // non-interior and not an end cell
            if (j > j0 && (t.zj[j] & 0xffffu) != (t.zj[j - 1] & 0xffffu)) ++zone_changes;
        }
        // (an end cell inside a full tile sits at its first / last position: cell 0 is j = 0 of chunk 0, and cell n-1
        // can only be followed by cells past the wire's end, which a tile with ends_only does not have)
        if (n < 2) ends_only = false;
        if (ends_only && !all_interior && changes == 0) t.kind_ne_mask |= 1u << tile;
        if (ends_only && zone_changes == 0 && changes > 0) t.kind_nj_mask |= 1u << tile;
        if (ends_only && changes == 1) t.kind_n1_mask |= (1u << tile) | (zone_changes == 1 ? 0x80000000u : 0u);
        // cells past the chunk keep the last real cell's flags so that zj[8t+7] is the tile's "hi" set
        for (int j = j1; j < j0 + 8; ++j) t.zj[j] = t.zj[j1 - 1];
        t.split[tile] = (uint32_t)split;
        if (changes > 1) t.kind[tile] = TILE_S;
        else if (all_interior && changes == 0) t.kind[tile] = TILE_N;
        else t.kind[tile] = TILE_B;
    }
    for (int tile = 0; tile < t.n_tiles; ++tile) {
        const uint32_t lo = t.zj[8 * tile], hi = t.zj[8 * tile + 7];
        for (int c = 0; c < 16; ++c) {
            t.chunk_flags[c][0] |= ((lo >> c) & 1u) << tile;
            t.chunk_flags[c][1] |= ((lo >> (16 + c)) & 1u) << tile;
            t.chunk_flags[c][2] |= ((hi >> c) & 1u) << tile;
            t.chunk_flags[c][3] |= ((hi >> (16 + c)) & 1u) << tile;
        }
        t.kind_n_mask |= (t.kind[tile] == TILE_N ? 1u : 0u) << tile;
        t.kind_s_mask |= (t.kind[tile] == TILE_S ? 1u : 0u) << tile;
        t.split_pack[tile >> 3] |= (t.split[tile] & 15u) << ((tile & 7) * 4);
    }
    return true;
}

// A handle belongs to the device that was current in wedm_create: its parameter / table / walk buffers
// live there and its launches must go to a stream of that device.  Launching with another device
// current would hand hipLaunchKernel a foreign stream (hipErrorInvalidResourceHandle at best).
static int32_t check_device(wedm_ctx* ctx, const char* who) {
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipGetDevice");
    if (dev != ctx->device)
        return fail(ctx, WEDM_ERR_BAD_ARG, std::string(who) + ": handle was created on device " + std::to_string(ctx->device) +
                                               " but device " + std::to_string(dev) + " is current (hipSetDevice first)");
    return WEDM_OK;
}

static int lanes_index(int L) { return L == 1 ? 0 : L == 2 ? 1 : L == 4 ? 2 : L == 8 ? 3 : L == 16 ? 4 : -1; }

// blocks of `per_block` environments that cover the batch
static int blocks(int64_t num_envs, int per_block) { return (int)((num_envs + per_block - 1) / per_block); }

// ------------------------------------------------------------ per-family fits: the LDS image in bytes (0: it does not fit)
// and the lanes per environment, each written once for the choice and the launch
static size_t fits(const wedm_ctx* c, size_t bytes) { return bytes <= (size_t)c->lds_limit ? bytes : 0; }
// a walk table of L chunks from `base` (W_LDS, W_STREAM), or nullptr
static const WalkInfo* walk_of(const wedm_ctx* c, int base, int L) {
    const int i = lanes_index(L);
    return i >= 0 && c->walk[base + i].ok ? &c->walk[base + i] : nullptr;
}
// kernel 3 (fused): one chunk of the L-chunk table per lane, + the halo row
static size_t fused_lds(const wedm_ctx* c, int L) {
    const WalkInfo* w = walk_of(c, W_LDS, L);
    return w ? fits(c, ((size_t)w->C + 1) * 1024) : 0;
}
// kernel 4 (packed): two chunks per lane, the table of 2L chunks
static size_t packed_lds(const wedm_ctx* c, int L) {
    const WalkInfo* w = walk_of(c, W_LDS, 2 * L);
    return w ? fits(c, (2 * (size_t)w->C + 2) * 1024) : 0;
}
// tables with a one-change boundary tile or a 1- / 2-cell tail: the EXTRA instantiation of kernels 4 and 9
static bool walk_extra(const WalkInfo* w) { return w->n1z || (w->C > 8 && (w->C & 7) >= 1 && (w->C & 7) <= 2); }
// kernel 9 (served): kernel 4's image staged by three walker waves, + the scalar wave's box of 48 / 24 environments
static size_t served_lds(const wedm_ctx* c, int L) {
    const WalkInfo* w = walk_of(c, W_LDS, 2 * L);
    return w ? fits(c, (2 * (size_t)w->C + 2) * 768 + (L == 8 ? sizeof(ServedBox<24>) : sizeof(ServedBox<48>))) : 0;
}
// kernel 6 (stream): the table of L chunks of whole 16-byte words, + the halo row
static size_t stream_lds(const wedm_ctx* c, int L) {
    const WalkInfo* w = walk_of(c, W_STREAM, L);
    return w ? fits(c, ((size_t)w->C + 1) * 1024) : 0;
}
// kernel 10 (lanes, any geometry): a chunk of ceil(n_seg_max / L) cells per lane
static size_t lanes_lds(const wedm_ctx* c, int L) { return fits(c, (size_t)((c->n_seg_max + L - 1) / L) * 1024); }
// kernel 2 (lanes_pk, either typing of the stencil): two virtual chunks of ceil(n_seg_max / 2L) cells per lane
static size_t lanes_pk_rows(const wedm_ctx* c, int L) { return 2 * (size_t)((c->n_seg_max + 2 * L - 1) / (2 * L)) + 2; }
static size_t lanes_pk_lds(const wedm_ctx* c, int L) { return fits(c, lanes_pk_rows(c, L) * 1024); }
// kernel 11 (lanes_served): those rows staged by three walker waves, + the scalar wave's box of 192 / L environments (the
// lane choice sizes the box for 48 whatever L)
static size_t lanes_served_lds(const wedm_ctx* c, int L, bool choice = false) {
    const size_t box = (L == 4 || choice) ? sizeof(ServedBox<48>) : L == 8 ? sizeof(ServedBox<24>) : sizeof(ServedBox<12>);
    return fits(c, lanes_pk_rows(c, L) * 768 + box);
}

// The lanes per environment of kernels 2, 10 and 11: the caller's count if its image fits, else the smallest L of `Ls`
// whose image fits, raised until `fills(c, L, image)` says the launch fills the chip; 0 if none fits.
template <class Image, class Fills>
static int fit_lanes(const wedm_ctx* c, std::initializer_list<int> Ls, Image image, Fills fills) {
    int lanes = 0;
    for (const int L : Ls) {
        const size_t b = image(c, L);
        if (!b) continue;
        if (c->lanes) { if (L == c->lanes) lanes = L; continue; }
        lanes = L;
        if (fills(c, L, b)) break;
    }
    return lanes;
}
// ~2 waves per SIMD (blocks of 256 lanes)
static bool fills_waves(const wedm_ctx* c, int L, size_t) { return (long)blocks(c->num_envs, 256 / L) * 4 >= 2048; }

static bool uniform_geometry(const wedm_ctx* c) { return !c->p.per_env_geometry && c->walk_dev; }

// kernel 6 (stream, single microseconds, uniform geometry): the caller's lane count, else -- among the L whose chunk
// has at most 64 cells (the registers a lane holds its chunk in) -- the largest one whose blocks are all resident at
// once (2 048 waves): a launch of one microsecond is one dependent chain per wave, and a shorter chunk is a shorter
// chain (4 096 x 400: 26.3 / 18.8 / 14.4 us with 4 / 8 / 16 lanes); a batch too large for one round takes the
// smallest such L (65 536 x 128: 2 lanes); failing all that a chunk of at most 104 cells
static int stream_lanes(const wedm_ctx* c) {
    if (!uniform_geometry(c) || (uint64_t)WEDM_T_QUADS(c->n_seg_max) * (uint64_t)c->s.stride * 16ull >= (1ull << 32)) return 0;
    for (const int cmax : {64, 104}) {
        int lanes = 0;
        for (const int L : {1, 2, 4, 8, 16}) {
            if (!stream_lds(c, L) || walk_of(c, W_STREAM, L)->C > cmax) continue;
            if (c->lanes && L != c->lanes) continue;
            if (lanes && (cmax > 64 || (long)blocks(c->num_envs, 256 / L) * 4 > 2048)) break;
            lanes = L;
        }
        if (lanes) return lanes;
    }
    return 0;
}

// kernel 8 (wide register kernel): 4, 8 or 16 lanes per environment (the fewest that hold the wire, or the caller's if they
// do), 32 cells each in registers; uniform geometry, 9 to 512 segments; 0 where it cannot run
static int wide_lanes(const wedm_ctx* c) {
    const wedm_params& P = c->p;
    const int wl_min = P.n_seg <= 128 ? 4 : P.n_seg <= 256 ? 8 : 16;
    const int wl = (c->lanes == 4 || c->lanes == 8 || c->lanes == 16) ? c->lanes : wl_min;
    const bool ok = uniform_geometry(c) && P.n_seg >= 9 && P.n_seg <= 512 && !c->replay && (c->lanes == 0 || (wl == c->lanes && wl >= wl_min));
    return ok ? wl : 0;
}

// kernel 7 (register kernel): one or two lanes per environment (default 2: two waves per SIMD) with the wire in their
// registers; wires of at most 128 segments, uniform geometry; 0 where it cannot run
static int regs_lanes(const wedm_ctx* c) {
    const bool ok = uniform_geometry(c) && c->walk[W_REGS2].ok && c->walk[W_REGS4].ok && c->n_seg_max <= 128 && !c->replay;
    return ok ? (c->lanes == 1 ? 1 : 2) : 0;
}

// tiles a chunk of C cells costs: its full tiles, a whole tile for a partial one, a quarter for a 1- / 2-cell tail
// (computed with the patched cells) -- 32 768 x 400: fused<8> 3.60e9, packed<8> 3.75e9 measured
static double eff_tiles(int C) {
    const int rest = C & 7;
    return (double)(C / 8) + (rest == 0 ? 0.0 : (C > 8 && rest <= 2) ? 0.25 : 1.0);
}

// kernel 9 (served packed kernel, wedm_served.h): the packed walk on three waves of a block, the scalar physics on the fourth;
// 4 or 8 lanes per environment.  Cost model (cycles per microsecond of the whole batch, same unit as the model of kernels
// 3 / 4; fitted to profiles/r4/plan_sweep.txt): a block's chain c = 1300 + 950 x tiles per lane; j blocks resident together
// on a CU take c x f(j), f = 1, 1.49, 1.80 (three fit the 168-register budget, fewer where the LDS image is large); blocks
// are dispatched as CUs free up, so the busiest CU runs b = ceil(blocks / 256) of them in groups of at most `rb`.
static double served_cost(const wedm_ctx* c, int L) {
    const size_t lds = served_lds(c, L);
    if (!lds) return 1e300;
    const long rb = std::min<long>(3, (long)(160 * 1024 / lds));
    const long b = (blocks(c->num_envs, 192 / L) + 255) / 256;
    static const double f[4] = {0.0, 1.0, 1.49, 1.80};
    // (a partial tile of 3 ... 7 cells runs the boundary-tile code for every lane: two tiles' worth -- 16 384 x 200 over 8 lanes,
    // chunks of 13 cells: 5.3 ms against 3.4 ms over 4 lanes)
    const int Cv = walk_of(c, W_LDS, 2 * L)->C, rest = Cv & 7;
    const double tiles = eff_tiles(Cv) + ((rest >= 3 || (rest && Cv < 8)) ? 1.0 : 0.0);
    const double cc = 1300.0 + 950.0 * tiles;
    return (double)(b / rb) * cc * f[rb] + ((b % rb) ? cc * f[b % rb] : 0.0);
}
// the served kernel's lanes: the caller's 4 or 8, else the cheaper by the model; 0 where it cannot run
static int served_lanes(const wedm_ctx* c) {
    const int L = (c->lanes == 4 || c->lanes == 8) ? c->lanes : (served_cost(c, 4) < served_cost(c, 8) ? 4 : 8);
    const bool ok = uniform_geometry(c) && c->p.stencil_mode == 0 && !c->replay && !c->p.keep_stepping_terminated &&
                    (c->lanes == 0 || c->lanes == L) && served_lds(c, L);
    return ok ? L : 0;
}

struct Choice {
    Kernel kernel = K_AUTO;
    int lanes = 0;  // lanes per environment (0: the family has no such choice)
};

// The kernel wedm_step launches for (single microsecond?, trace point?) under the handle's settings, and its lanes per
// environment; every refusal of a forced kernel or of a binding it has no form for.
static int32_t choose_kernel(wedm_ctx* ctx, bool single, bool tr, Choice& out) {
    const wedm_params& P = ctx->p;
    const bool uniform = uniform_geometry(ctx), f64 = P.stencil_mode != 0, replay = ctx->replay != nullptr;
    const bool pulse = ctx->pulse != nullptr, envp = ctx->envp != nullptr, mat = ctx->wmat != nullptr;
    const bool sig = ctx->sig != nullptr;
    // kernel 3 (one chunk per lane) and kernel 4 (two packed chunks per lane, table of 2L chunks).
    // Auto-selection by a small cost model fitted to measurements:
    //   cycles per step ~ rounds * (4500 + tiles_per_lane * 8 * cell_cost),  tiles_per_lane: see eff_tiles,
    //   rounds = ceil(blocks / (256 CUs * resident blocks per CU)), resident = min(2 [VGPRs], LDS fit),
    //   cell_cost = 90 per cell, a packed pair = 2 * 90 * 0.93.
    double best3 = 1e300, best4 = 1e300;  // cycles per microsecond of the whole batch, by the model above
    int l3 = 0, l4 = 0;
    for (const int L : {1, 2, 4, 8, 16}) {
        if (!uniform) break;
        const long nb = blocks(ctx->num_envs, 256 / L);
        auto rounds = [&](size_t lds) {
            const long rb = std::min<long>(2, (long)(160 * 1024 / lds));
            return (nb + 256 * rb - 1) / (256 * rb);
        };
        if (const size_t lds = fused_lds(ctx, L)) {
            const double cost = rounds(lds) * (4500.0 + eff_tiles(walk_of(ctx, W_LDS, L)->C) * 8 * 90.0);
            if (cost < best3) { best3 = cost; l3 = L; }
        }
        if (const size_t lds = packed_lds(ctx, L)) {
            const double cost = rounds(lds) * (4500.0 + eff_tiles(walk_of(ctx, W_LDS, 2 * L)->C) * 8 * 2 * 90.0 * 0.93);
            if (cost < best4) { best4 = cost; l4 = L; }
        }
    }
    const int lanes = ctx->lanes ? ctx->lanes : l3, planes = ctx->lanes ? ctx->lanes : l4;
    const bool fused_ok = uniform && fused_lds(ctx, lanes), packed_ok = uniform && packed_lds(ctx, planes);
    // kernel 10 (any geometry) and kernel 2, its packed form: the smallest L whose chunk fits in LDS, raised until the
    // launch has ~2 waves per SIMD
    const int glanes = fit_lanes(ctx, {1, 2, 4, 8, 16}, lanes_lds, fills_waves);
    const int pklanes = fit_lanes(ctx, {1, 2, 4, 8, 16}, lanes_pk_lds, fills_waves);
    const bool lanes_ok = glanes > 0;
    const bool use_pk = !replay && pklanes > 0;  // (kernel 2 is the packed form where it applies, both typings of the stencil)
    // kernel 11 (wedm_step_lanes_served: 4, 8 or 16 lanes per environment, three walker waves + the scalar wave per block, three
    // blocks per CU where the LDS image allows): the fewest lanes whose blocks fill the chip at three per CU
    const int svgl = fit_lanes(ctx, {4, 8, 16}, [](const wedm_ctx* c, int L) { return lanes_served_lds(c, L, true); },
                               [](const wedm_ctx* c, int L, size_t b) { return blocks(c->num_envs, 192 / L) >= 768 && 3 * b <= 160 * 1024; });
    const bool lanes_sv_ok = svgl > 0 && !replay && !f64 && !P.keep_stepping_terminated;
    const int slanes = stream_lanes(ctx), wl = wide_lanes(ctx), rl = regs_lanes(ctx), svl = served_lanes(ctx);
    const int stream_C = slanes ? walk_of(ctx, W_STREAM, slanes)->C : 0;
    const bool stream_auto = slanes && stream_C <= 64 && (long)blocks(ctx->num_envs, 256 / slanes) * 4 <= 2048;
    // the stream kernel under stencil_mode 1: its single-microsecond instantiation only (chunks of at most 64 cells, no trace sample)
    const bool stream_f64_ok = slanes && single && !tr && stream_C <= 64;
    // kernel 8 by itself for a batch that one round of blocks covers at one wave per SIMD: such a launch is one wave's
    // dependent chain per microsecond whatever the kernel, and this one's is the shortest (measured, 4 096 x 400 and
    // 16 384 x 128: DESIGN.md 4.1b).  (stencil_mode 1, a short wire in a tiny batch: 256 waves of this kernel over 4 lanes
    // against 1 024 of the tile walk over 16 -- 2.81 against 2.47 ms at 4 096 x 128, profiles/r4/plan_sweep_f64.txt)
    const bool f64_tiny = f64 && P.n_seg <= 128 && ctx->num_envs <= 4096;
    const bool wide_auto = !single && wl && !f64_tiny && ctx->lanes == 0 && (int64_t)ctx->num_envs * wl <= (int64_t)WEDM_WIDE_AUTO_MAX_LANES;
    // kernel 7 for fused launches of a batch that gives most CUs a block of the register kernel (measured, 128 segments, two
    // lanes per environment against the best LDS kernel: 8 192 environments 2.8e9 vs 3.5e9, 16 384: 5.5e9 vs 6.1e9,
    // 24 576: 8.3e9 vs 7.4e9, 32 768: 1.10e10 vs 9.9e9, 65 536: 1.67e10 vs 1.44e10, 131 072: 1.76e10 vs 1.50e10;
    // up to 16 384 environments the wide register kernel has taken the launch: 8.1e9 there)
    // (stencil_mode 1: single microseconds too -- 34 us against the cell-by-cell LDS kernel's 44 at 65 536 x 128)
    const bool regs_auto = (!single || f64) && rl && ctx->lanes == 0 && ctx->num_envs >= 20480;

    // the caller's kernel, and what refuses it outright
    int32_t forced = ctx->variant;
    // per-environment wire material: kernels 1 and 2 only (the other families take uniform geometry, or have no MAT form),
    // and no injected variates
    if (mat && replay)
        return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: injected variates (wedm_bind_rng_replay) and a per-environment wire material (wedm_bind_wire_material) cannot be combined");
    if (mat && !has_form(forced, F_MAT))
        return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: with a per-environment wire material bound (wedm_bind_wire_material) only kernels 0 (auto), 1 and 2 run");
    // signal statistics: kernels 1 and 2 only, and no injected variates
    if (sig && replay)
        return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: injected variates (wedm_bind_rng_replay) and signal statistics (wedm_bind_signal_stats) cannot be combined");
    if (sig && !has_form(forced, F_SIG))
        return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: with signal statistics bound (wedm_bind_signal_stats) only kernels 0 (auto), 1 and 2 run");
    if (replay) {
        if (forced != K_AUTO && forced != K_GLOBAL)
            return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: injected variates (wedm_bind_rng_replay) run on kernel 1 only");
        if (f64) return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: injected variates and stencil_mode 1 cannot be combined");
        forced = K_GLOBAL;
    }
    if (envp && !has_form(forced, F_ENVP))
        return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: with per-environment physics parameters bound (wedm_bind_env_params) only kernels 0 (auto), 1 and 2 run");
    // Numba's typing of the stencil: the register kernels (uniform geometry; at most 128 / 512 segments), the fused tile walk
    // (uniform geometry), the predicated LDS kernel (any geometry), or in place in global memory; no packed LDS form, no served
    // form, no stream / split kernel
    if (f64 && !has_form(forced, F_F64))
        return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: stencil_mode 1 (float64 stencil expressions) runs on kernels 1, 2 (10), 3, 6 (single microseconds without a trace sample), 7 and 8 only");
    if (f64 && forced == K_STREAM && !stream_f64_ok)
        return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: under stencil_mode 1 the stream kernel runs launches of one microsecond without a trace sample, chunks of at most 64 cells");
    if (forced == K_WIDE && !wl)
        return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: wide register kernel needs uniform geometry, 9 to 512 segments and lanes 0, 4, 8 or 16 with 32 cells per lane covering the wire");
    if (pulse && !has_form(forced, F_PULSE))
        return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: with pulse statistics bound (wedm_bind_pulse_stats) only kernels 0 (auto), 1, 2, 7 and 8 run");

    int32_t v = forced;
    if (pulse || envp || mat || sig) {
        // bound rows: the float32 stencil without a trace sample or injected variates runs the caller's kernel, and a fused
        // launch under auto what the automatic choice takes among the forms there are (pulse: 8 or 7, else kernel 2's packed
        // form; envp, mat, sig: kernel 2's packed form); every other launch runs kernel 1, and so does every launch with pulse
        // statistics and rows or signal statistics bound (kernel 2's ENVP, MAT and SIG forms count no pulses; kernels 7 and 8
        // have no SIG form)
        const bool fast = !tr && !f64 && !replay;
        v = fast ? forced : K_GLOBAL;
        if (v == K_AUTO && !single)
            v = pulse && sig ? K_GLOBAL : pulse && wide_auto ? K_WIDE : pulse && regs_auto ? K_REGS : use_pk ? K_LANES_PK : K_GLOBAL;
        if (v == K_AUTO) v = K_GLOBAL;
        if (v == K_LANES_PK && !use_pk && pulse)
            return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: with pulse statistics bound kernel 2 runs its packed form only, and no lane count puts its chunks in LDS");
        if (v == K_LANES_PK && !use_pk && envp)
            return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: with per-environment physics parameters bound kernel 2 runs its packed form only, and no lane count puts its chunks in LDS");
        if (v == K_LANES_PK && !use_pk && mat)
            return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: with a per-environment wire material bound kernel 2 runs its packed form only, and no lane count puts its chunks in LDS");
        if (v == K_LANES_PK && !use_pk)
            return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: with signal statistics bound kernel 2 runs its packed form only, and no lane count puts its chunks in LDS");
        if ((envp || mat || sig) && pulse) v = K_GLOBAL;
    } else if (v == K_AUTO) {
        // (stencil_mode 1, single microseconds: the stream kernel where the float32 launch takes it too and every tile of
        // the table has register-walk code)
        if (f64 && stream_f64_ok && stream_auto && walk_of(ctx, W_STREAM, slanes)->kind_s == 0u) v = K_STREAM;
        else if (wide_auto) v = K_WIDE;
        else if (regs_auto) v = K_REGS;
        // stencil_mode 1, longer wires, any batch: the wide register kernel (two blocks per CU beyond one wave per SIMD) -- 18 - 20
        // float64 operations per cell leave the LDS round trips of the tile walk nothing to hide behind (32 768 x 400: 1.93e9
        // against the fused kernel's 1.49e9; 8 192 x 400: 1.5e9 against 1.2e9 already at one block per CU)
        else if (f64 && !single && wl && !f64_tiny && ctx->lanes == 0) v = K_WIDE;
        // the served kernel where its model beats what the choice so far would take (measured over 2 048 ... 131 072 environments x
        // 128 ... 512 segments, profiles/r4/plan_sweep.txt: blocks of 24 / 48 environments, three to a CU, fill the chip where
        // blocks of 32 ... 128 leave a ragged second round, and a sixth fewer instructions)
        if (!single && !tr && svl && ctx->lanes == 0 && P.n_seg <= 512 /* the range the model was fitted on */ &&
            (v == K_AUTO || v == K_REGS)) {
            double other = std::min(best3, best4);
            if (v == K_REGS) {  // the two-lane register kernel: 128 environments per block, two blocks per CU (6 050 / 7 800 cycles)
                const long b = (blocks(ctx->num_envs, 128) + 255) / 256;
                other = (double)(b / 2) * 7800.0 + (double)(b % 2) * 6050.0;
            }
            if (served_cost(ctx, svl) < other) v = K_SERVED;
        }
        // single-microsecond launches: the stream kernel where one round of blocks covers the batch with chunks of
        // at most 64 cells (measured: 27.5 vs 30.3 us at 65 536 x 128, 20.5 vs 24.9 us at 4 096 x 400), else the
        // split global-memory kernel (32.7 vs 48.9 us at 32 768 x 400, where the stream kernel needs two rounds)
        if (v == K_AUTO) {
            if (f64) v = (!single && fused_ok) ? K_FUSED : (lanes_ok || use_pk) ? K_LANES_PK : K_GLOBAL;
            else if (single) v = stream_auto ? K_STREAM : K_SPLIT;
            else if (packed_ok && (best4 <= best3 || !fused_ok)) v = K_PACKED;
            else if (fused_ok) v = K_FUSED;
            else v = (lanes_ok || use_pk) ? K_LANES_PK : K_GLOBAL;
        }
    }
    if (v == K_SERVED && !svl)
        return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: served kernel needs uniform geometry, the float32 stencil, lanes 4 or 8, two chunks that fit in LDS and freeze_terminated");
    // (no trace point in the served kernel)
    if (v == K_SERVED && tr) v = packed_ok ? K_PACKED : fused_ok ? K_FUSED : (lanes_ok || use_pk) ? K_LANES_PK : K_GLOBAL;
    // kernel 12 (served register kernel): the register kernel's conditions + what the served scalar wave does not do
    if (v == K_REGS_SERVED && (!rl || f64 || tr || P.keep_stepping_terminated))
        return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: served register kernel needs uniform geometry, at most 128 segments, the float32 stencil, no trace sample in the launch and freeze_terminated");
    if (v == K_REGS && !rl)
        return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: register kernel needs uniform geometry and at most 128 segments");
    if (v == K_FUSED && !fused_ok)
        return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: fused kernel needs uniform geometry and a chunk that fits in LDS");
    if (v == K_PACKED && !packed_ok)
        return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: packed kernel needs uniform geometry, lanes in {1,2,4,8} and two chunks that fit in LDS");
    // (kernel 11 by name only: at 16 384 environments x <= 450 segments it measures 2.39e9 against the packed form's 2.48e9 -
    // 2.62e9; a trace sample, stencil_mode 1, keep-stepping: the unserved forms)
    if (v == K_LANES_SERVED && (!lanes_sv_ok || tr)) v = K_LANES_PK;
    if ((v == K_LANES_PK && !use_pk && !lanes_ok) || (v == K_LANES && !lanes_ok))
        return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: no lane count puts a chunk of the wire in LDS");
    if (v == K_STREAM && !slanes)
        return fail(ctx, WEDM_ERR_UNSUPPORTED, "wedm_step: stream kernel needs uniform geometry and lanes in {1,2,4,8,16} with a chunk of at most 104 cells");
    if (v == K_LANES_PK && !use_pk) v = K_LANES;  // kernel 2 without a packed fit: its cell-by-cell form
    out.kernel = (Kernel)v;
    switch (out.kernel) {
        case K_LANES_PK: out.lanes = pklanes; break;
        case K_FUSED: out.lanes = lanes; break;
        case K_PACKED: out.lanes = planes; break;
        case K_STREAM: out.lanes = slanes; break;
        case K_REGS: out.lanes = rl; break;
        case K_WIDE: out.lanes = wl; break;
        case K_SERVED: out.lanes = svl; break;
        case K_LANES: out.lanes = glanes; break;
        case K_LANES_SERVED: out.lanes = svgl; break;
        default: out.lanes = 0; break;
    }
    return WEDM_OK;
}

static const char* const kernel_names[] = {"", "wedm_step_global", "wedm_step_lanes_pk", "wedm_step_fused", "wedm_step_packed",
                                           "wedm_step_split", "wedm_step_stream", "wedm_step_regs", "wedm_step_regs_wide",
                                           "wedm_step_served", "wedm_step_lanes", "wedm_step_lanes_served", "wedm_step_regs_served"};

// What wedm_step launches for (single microsecond?, trace point?) under the handle's current settings: decided once
// and cached (the decision walks a cost model over five lane counts; on the one-launch-per-microsecond path that and
// a hipFuncSetAttribute per call were a measurable part of the host time per launch).  The choice, then per family the
// form of the launch, its grid, block, LDS image and walk table; the instantiation is the registry's entry for the form.
static int32_t plan_launch(wedm_ctx* ctx, bool single, bool tr, bool frozen_ok, LaunchPlan& out) {
    Choice ch;
    if (int32_t rc = choose_kernel(ctx, single, tr, ch)) return rc;
    const int L = ch.lanes, n = ctx->num_envs;
    const bool f64 = ctx->p.stencil_mode != 0, replay = ctx->replay != nullptr, pulse = ctx->pulse != nullptr, envp = ctx->envp != nullptr;
    const bool mat = ctx->wmat != nullptr;  // (never with injected variates, never with pulse statistics on kernel 2: choose_kernel)
    const bool sig = ctx->sig != nullptr;   // (the same)
    // the form: the launch's trace point and the handle's bindings (kernel 1 has a form for each such set; the PULSE, ENVP
    // and MAT forms of the other families carry neither TRACE nor F64), then each family's own bits below
    uint32_t F = (tr ? F_TRACE : 0u) | (f64 ? F_F64 : 0u) | (replay ? F_REPLAY : 0u) | (pulse ? F_PULSE : 0u) |
                 (envp ? F_ENVP : 0u) | (mat ? F_MAT : 0u) | (sig ? F_SIG : 0u);
    if (ch.kernel != K_GLOBAL && (F & (F_PULSE | F_ENVP | F_MAT | F_SIG))) F &= ~(F_TRACE | F_F64);
    const WalkInfo* w = nullptr;  // the walk table the launch reads
    bool fz = false;              // the FROZEN_OK form (named in the kernel string)
    int grid = blocks(n, 256 / std::max(L, 1)), block = 256;
    size_t fl = 0;
    switch (ch.kernel) {
        case K_LANES_PK: fl = lanes_pk_lds(ctx, L); break;
        case K_LANES: fl = lanes_lds(ctx, L); break;
        case K_FUSED:
            // handles with in-launch autoreset expect terminations, and so do handles whose kernels have reported a frozen
            // environment (wedm_ctx::frozen_seen): the form that tolerates frozen lanes; N1: the table has a one-change
            // tile that is a boundary tile in every microsecond.  (stencil_mode 1: FROZEN_OK always, no N1)
            w = walk_of(ctx, W_LDS, L);
            fl = fused_lds(ctx, L);
            fz = frozen_ok;
            F |= f64 ? F_FROZEN_OK : (frozen_ok ? F_FROZEN_OK : 0u) | (w->n1z ? F_N1 : 0u);
            break;
        case K_PACKED:
            w = walk_of(ctx, W_LDS, 2 * L);
            fl = packed_lds(ctx, L);
            fz = frozen_ok;
            F |= (frozen_ok ? F_FROZEN_OK : 0u) | (walk_extra(w) ? F_EXTRA : 0u);
            break;
        case K_SERVED:  // three walker waves + the scalar wave
            w = walk_of(ctx, W_LDS, 2 * L);
            fl = served_lds(ctx, L);
            grid = blocks(n, 192 / L);
            F |= walk_extra(w) ? F_EXTRA : 0u;
            break;
        case K_LANES_SERVED:
            fl = lanes_served_lds(ctx, L);
            grid = blocks(n, 192 / L);
            break;
        case K_STREAM: {
            // launches of one microsecond without a trace sample, chunks of at most 64 cells: the form without the loop
            // (stencil_mode 1: the only one); else the rows a lane holds in registers: 64 (128 segments over 2 lanes, 400
            // over 8) or 104 (400 over 4)
            w = walk_of(ctx, W_STREAM, L);
            fl = stream_lds(ctx, L);
            const bool one = single && !tr && w->C <= 64;
            F = (one || f64) ? F_ONE | (F & F_F64) : F | (w->C > 64 ? F_CMAX104 : 0u);
            break;
        }
        case K_SPLIT: grid = blocks(n, 64); break;
        case K_REGS:  // the table of two chunks of 64 cells (one lane) / four of 32 (two lanes)
            w = &ctx->walk[L == 1 ? W_REGS2 : W_REGS4];
            break;
        case K_WIDE:
            // CUT: wires whose length is not a multiple of 8, and every traced launch.  (stencil_mode 1: a batch of more than
            // one wave per SIMD runs the two-blocks-per-CU form -- 32 768 x 400: 1.93e9 against 1.52e9; 4 096 x 400:
            // 1.33e9 against 1.45e9)
            if ((ctx->p.n_seg & 7) != 0 || tr) F |= F_CUT;
            if (f64 && (int64_t)n * L > (int64_t)WEDM_WIDE_AUTO_MAX_LANES) F |= F_MINB2;
            break;
        case K_REGS_SERVED:  // two walker waves + the scalar wave; the table of four chunks of 32 cells
            w = &ctx->walk[W_REGS4];
            fl = sizeof(ServedBox<64>);
            grid = blocks(n, 64);
            block = 192;
            break;
        case K_GLOBAL:
        case K_AUTO: break;
    }
    const void* fn = find_instantiation(ch.kernel, L, F);
    if (!fn)  // (an internal error: choose_kernel leaves no launch without its form)
        return fail(ctx, WEDM_ERR_UNSUPPORTED, std::string("wedm_step: internal error: no instantiation of ") + kernel_names[ch.kernel] +
                                                   " for " + std::to_string(L) + " lanes and the forms " + form_names(F));
    if (fl) {
        // The attribute belongs to the kernel FUNCTION, not to this handle or plan: two live handles with different wire
        // lengths can resolve to the same instantiation, and a later plan with a smaller image must not lower the limit
        // under an earlier plan that is still cached.  Every function is therefore opened up to the device's limit.
        hipError_t ea = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
        if (ea != hipSuccess) return hip_fail(ctx, ea, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
    }
    char lanes_s[16] = "", lds_s[32] = "";
    if (L) std::snprintf(lanes_s, sizeof(lanes_s), "<%d>", L);
    if (fl) std::snprintf(lds_s, sizeof(lds_s), ",%zuB", fl);
    std::snprintf(out.name, sizeof(out.name), "%s%s%s%s%s%s%s<<<%d,%d%s>>>", kernel_names[ch.kernel], lanes_s,
                  replay ? "[injected variates]" : f64 ? "[f64 stencil]" : fz ? "[frozen lanes ok]" : "", pulse ? "[pulse]" : "",
                  envp ? "[envp]" : "", mat ? "[wmat]" : "", sig ? "[sig]" : "", grid, block, lds_s);
    out.fn = fn;
    out.kernel = ch.kernel;
    out.lanes = L;
    out.forms = F;
    out.grid = grid;
    out.block = block;
    out.lds = fl;
    out.walk = w ? ctx->walk_dev + (w - ctx->walk) : nullptr;
    out.valid = true;
    return WEDM_OK;
}

static thread_local std::string g_create_error;

extern "C" {

int32_t wedm_abi_version(void) { return WEDM_ABI_VERSION; }
#ifndef WEDM_BUILD_ID
#define WEDM_BUILD_ID "unknown"
#endif
const char* wedm_build_id(void) { return WEDM_BUILD_ID; }
int64_t wedm_sizeof_params(void) { return (int64_t)sizeof(wedm_params); }

const char* wedm_last_error(wedm_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }
const char* wedm_last_kernel(wedm_ctx* ctx) {
    if (!ctx) return "";
    if (ctx->last_plan) ctx->last_kernel = std::string(ctx->last_plan->name) + " n_sub=" + std::to_string(ctx->last_n_sub);
    return ctx->last_kernel.c_str();
}

int32_t wedm_last_occupancy(wedm_ctx* ctx) {
    if (!ctx || !ctx->last_plan) return WEDM_ERR_BAD_ARG;
    int n = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, ctx->last_plan->fn, ctx->last_plan->block, ctx->last_plan->lds);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipOccupancyMaxActiveBlocksPerMultiprocessor");
    return (int32_t)n;
}

int32_t wedm_create(const wedm_params* params, int32_t num_envs, int32_t n_seg_max, wedm_ctx** out) {
    if (!params || !out || num_envs <= 0 || n_seg_max <= 0) {
        g_create_error = "wedm_create: null pointer or non-positive size";
        return WEDM_ERR_BAD_ARG;
    }
    if (!params->per_env_geometry && (params->n_seg < 1 || params->n_seg > n_seg_max)) {
        g_create_error = "wedm_create: params.n_seg outside [1, n_seg_max]";
        return WEDM_ERR_BAD_ARG;
    }
    if (params->servo_interval <= 0 || params->dt_us <= 0 || (params->control_mode != 0 && params->control_mode != 1)) {
        g_create_error = "wedm_create: servo_interval/dt must be positive, control_mode 0 or 1";
        return WEDM_ERR_BAD_ARG;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_create_error = std::string("wedm_create: no HIP device visible (") + hipGetErrorString(e) + ")";
        return WEDM_ERR_NO_DEVICE;
    }
    int dev = 0;
    if ((e = hipGetDevice(&dev)) != hipSuccess) {
        g_create_error = std::string("hipGetDevice: ") + hipGetErrorString(e);
        return WEDM_ERR_HIP;
    }
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, dev)) != hipSuccess) {
        g_create_error = std::string("hipGetDeviceProperties: ") + hipGetErrorString(e);
        return WEDM_ERR_HIP;
    }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_error = std::string("wedm_create: device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
        return WEDM_ERR_NO_DEVICE;
    }
    wedm_ctx* ctx = new (std::nothrow) wedm_ctx();
    if (!ctx) return WEDM_ERR_BAD_ARG;
    // a failure from here on frees what has been allocated (wedm_destroy frees the non-null members)
    auto hip_error = [&](const char* what) {
        g_create_error = std::string(what) + ": " + hipGetErrorString(e);
        (void)wedm_destroy(ctx);
        return WEDM_ERR_HIP;
    };
    ctx->p = *params;
    ctx->num_envs = num_envs;
    ctx->n_seg_max = n_seg_max;
    ctx->device = dev;
    ctx->lds_limit = (int)prop.sharedMemPerBlock;
    int optin = 0;
    if (hipDeviceGetAttribute(&optin, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess && optin > ctx->lds_limit)
        ctx->lds_limit = optin;
    // per-mode tables -> one small device buffer (per-lane indexed loads)
    const size_t n = WEDM_MAX_MODE + 1;
    const size_t bytes = 4 * n * sizeof(double) + n * sizeof(int32_t);
    if ((e = hipMalloc(&ctx->tables_dev, bytes)) != hipSuccess) return hip_error("hipMalloc(tables)");
    char host[4 * 20 * 8 + 20 * 4];
    std::memcpy(host + 0 * n * 8, params->mode_current, n * 8);
    std::memcpy(host + 1 * n * 8, params->crater_mean, n * 8);
    std::memcpy(host + 2 * n * 8, params->crater_std, n * 8);
    std::memcpy(host + 3 * n * 8, params->crater_depth, n * 8);
    std::memcpy(host + 4 * n * 8, params->crater_valid, n * 4);
    if ((e = hipMemcpy(ctx->tables_dev, host, bytes, hipMemcpyHostToDevice)) != hipSuccess) return hip_error("hipMemcpy(tables)");
    const double* d = (const double*)ctx->tables_dev;
    ctx->tb.mode_current = d;
    ctx->tb.crater_mean = d + n;
    ctx->tb.crater_std = d + 2 * n;
    ctx->tb.crater_depth = d + 3 * n;
    ctx->tb.crater_valid = (const int32_t*)(d + 4 * n);
    if ((e = hipMalloc((void**)&ctx->params_dev, sizeof(wedm_params))) != hipSuccess ||
        (e = hipMemcpy(ctx->params_dev, params, sizeof(wedm_params), hipMemcpyHostToDevice)) != hipSuccess)
        return hip_error("params copy");
    if (!params->per_env_geometry) {
        std::vector<WalkTable> host_tabs(W_COUNT);
        auto build = [&](int w, int L, int align) {
            WalkInfo& info = ctx->walk[w];
            info.ok = build_walk(*params, L, host_tabs[w], align);
            info.C = host_tabs[w].C;
            info.kind_s = host_tabs[w].kind_s_mask;
            info.n1z = info.ok && (host_tabs[w].kind_n1_mask & 0x80000000u);
        };
        const int Ls[5] = {1, 2, 4, 8, 16};
        for (int i = 0; i < 5; ++i) {
            build(W_LDS + i, Ls[i], 1);
            build(W_STREAM + i, Ls[i], 4);
        }
        if (params->n_seg <= 128)  // the register kernels' tables: two chunks of exactly 64 cells, four of 32
            for (const int w : {W_REGS2, W_REGS4}) {
                const int L = w == W_REGS2 ? 2 : 4;
                build(w, L, 128 / L);
                ctx->walk[w].ok = ctx->walk[w].ok && ctx->walk[w].C == 128 / L;
            }
        const size_t tab_bytes = host_tabs.size() * sizeof(WalkTable);
        if ((e = hipMalloc((void**)&ctx->walk_dev, tab_bytes)) != hipSuccess ||
            (e = hipMemcpy(ctx->walk_dev, host_tabs.data(), tab_bytes, hipMemcpyHostToDevice)) != hipSuccess)
            return hip_error("walk tables");
    }
    // (optional: without it every handle without autoreset simply keeps the instantiation without the frozen-lane code)
    if (hipHostMalloc((void**)&ctx->frozen_seen, sizeof(int32_t), hipHostMallocMapped) == hipSuccess) {
        *ctx->frozen_seen = 0;
        if (hipHostGetDevicePointer((void**)&ctx->frozen_seen_dev, ctx->frozen_seen, 0) != hipSuccess) {
            (void)hipHostFree(ctx->frozen_seen);
            ctx->frozen_seen = ctx->frozen_seen_dev = nullptr;
        }
    } else {
        (void)hipGetLastError();
        ctx->frozen_seen = nullptr;
    }
    *out = ctx;
    return WEDM_OK;
}

int32_t wedm_destroy(wedm_ctx* ctx) {
    if (!ctx) return WEDM_ERR_BAD_ARG;
    if (ctx->frozen_seen) (void)hipHostFree(ctx->frozen_seen);
    if (ctx->tables_dev) (void)hipFree(ctx->tables_dev);
    if (ctx->walk_dev) (void)hipFree(ctx->walk_dev);
    if (ctx->params_dev) (void)hipFree(ctx->params_dev);
    delete ctx;
    return WEDM_OK;
}

int32_t wedm_bind_state(wedm_ctx* ctx, const wedm_state_ptrs* state) {
    if (!ctx) return WEDM_ERR_BAD_ARG;
    if (!state || !state->f64 || !state->i32 || !state->i8 || !state->T)
        return fail(ctx, WEDM_ERR_BAD_ARG, "wedm_bind_state: null state block");
    if (state->stride < ctx->num_envs) return fail(ctx, WEDM_ERR_BAD_ARG, "wedm_bind_state: stride < num_envs");
    if (ctx->p.obs_dim > 0 && !state->obs) return fail(ctx, WEDM_ERR_BAD_ARG, "wedm_bind_state: obs_dim > 0 but obs is null");
    ctx->s = *state;
    ctx->bound = true;
    ctx->invalidate_plans();
    return WEDM_OK;
}

int32_t wedm_bind_geometry(wedm_ctx* ctx, const wedm_geom_ptrs* geom) {
    if (!ctx) return WEDM_ERR_BAD_ARG;
    if (!geom || !geom->f64 || !geom->i32) return fail(ctx, WEDM_ERR_BAD_ARG, "wedm_bind_geometry: null geometry block");
    ctx->g = *geom;
    ctx->geom_bound = true;
    ctx->invalidate_plans();
    return WEDM_OK;
}

int32_t wedm_bind_trace(wedm_ctx* ctx, const wedm_trace_desc* desc) {
    if (!ctx) return WEDM_ERR_BAD_ARG;
    ctx->trace_on = false;
    ctx->trace_us = ctx->trace_count = 0;
    if (!desc) return WEDM_OK;
    const uint32_t f64_all = (1u << WEDM_F64_COUNT) - 1u, i32_all = (1u << WEDM_I32_COUNT) - 1u,
                   i8_all = (1u << WEDM_I8_COUNT) - 1u;
    if ((desc->f64_mask & ~f64_all) || (desc->i32_mask & ~i32_all) || (desc->i8_mask & ~i8_all))
        return fail(ctx, WEDM_ERR_BAD_ARG, "wedm_bind_trace: mask names a row that does not exist");
    // a sample is taken from the registers: the rows that no register holds (wedm_env_rows.h) cannot be traced.  MODE_CACHED has
    // always been accepted all the same (its samples are 0: DESIGN.md section 3, open points); that stays until it is decided.
#define WEDM_REFUSE(row, owner, why) if (mask & (1u << row)) return fail(ctx, WEDM_ERR_BAD_ARG, "wedm_bind_trace: " why " (read it from the state block)");
    { const uint32_t mask = desc->i32_mask; WEDM_UNHELD_I32(WEDM_REFUSE) }
    { const uint32_t mask = desc->f64_mask; WEDM_UNHELD_F64(WEDM_REFUSE) }
    { const uint32_t mask = desc->i8_mask & ~(1u << WEDM_B_MODE_CACHED); WEDM_UNHELD_I8(WEDM_REFUSE) }
#undef WEDM_REFUSE
    if ((desc->f64_mask != 0) != (desc->f64 != nullptr) || (desc->i32_mask != 0) != (desc->i32 != nullptr) ||
        (desc->i8_mask != 0) != (desc->i8 != nullptr))
        return fail(ctx, WEDM_ERR_BAD_ARG, "wedm_bind_trace: a buffer must be given exactly for the non-empty masks");
    if (!desc->f64_mask && !desc->i32_mask && !desc->i8_mask && !desc->T)
        return fail(ctx, WEDM_ERR_BAD_ARG, "wedm_bind_trace: nothing selected");
    if (desc->every < 1 || desc->capacity < 1)
        return fail(ctx, WEDM_ERR_BAD_ARG, "wedm_bind_trace: every and capacity must be >= 1");
    if (desc->env_lo < 0 || desc->env_count < 1 || (int64_t)desc->env_lo + desc->env_count > ctx->num_envs)
        return fail(ctx, WEDM_ERR_BAD_ARG, "wedm_bind_trace: environment range outside [0, num_envs)");
    ctx->trace = *desc;  // travels by value with every launch: nothing to copy to the device here
    ctx->trace_on = true;
    return WEDM_OK;
}

int64_t wedm_trace_samples(wedm_ctx* ctx) { return ctx ? ctx->trace_count : 0; }

int32_t wedm_bind_rng_replay(wedm_ctx* ctx, const double* table, int64_t n_steps) {
    if (!ctx) return WEDM_ERR_BAD_ARG;
    if (table && n_steps < 1) return fail(ctx, WEDM_ERR_BAD_ARG, "wedm_bind_rng_replay: n_steps must be >= 1");
    ctx->replay = table;
    ctx->replay_steps = table ? n_steps : 0;
    ctx->invalidate_plans();
    return WEDM_OK;
}

int32_t wedm_bind_pulse_stats(wedm_ctx* ctx, int32_t* rows) {
    if (!ctx) return WEDM_ERR_BAD_ARG;
    ctx->pulse = rows;
    ctx->invalidate_plans();
    return WEDM_OK;
}

int32_t wedm_bind_env_params(wedm_ctx* ctx, const double* rows) {
    if (!ctx) return WEDM_ERR_BAD_ARG;
    ctx->envp = rows;
    ctx->invalidate_plans();
    return WEDM_OK;
}

int32_t wedm_bind_wire_material(wedm_ctx* ctx, const double* rows) {
    if (!ctx) return WEDM_ERR_BAD_ARG;
    // the material's conductivity and heat capacity live in the geometry rows (WEDM_G_K_COND, WEDM_G_TUF)
    if (rows && !(ctx->p.per_env_geometry && ctx->geom_bound))
        return fail(ctx, WEDM_ERR_NOT_BOUND, "wedm_bind_wire_material: needs per-environment geometry (per_env_geometry and wedm_bind_geometry): the geometry rows hold the material's conductivity and heat capacity");
    ctx->wmat = rows;
    ctx->invalidate_plans();
    return WEDM_OK;
}

int32_t wedm_bind_signal_stats(wedm_ctx* ctx, double* rows) {
    if (!ctx) return WEDM_ERR_BAD_ARG;
    if (rows && !ctx->bound)  // the block's stride is the state blocks'
        return fail(ctx, WEDM_ERR_NOT_BOUND, "wedm_bind_signal_stats: call wedm_bind_state first");
    ctx->sig = rows;
    ctx->invalidate_plans();
    return WEDM_OK;
}

int32_t wedm_set_kernel(wedm_ctx* ctx, int32_t variant) {
    if (!ctx) return WEDM_ERR_BAD_ARG;
    if (variant < 0 || variant > 12) return fail(ctx, WEDM_ERR_BAD_ARG, "wedm_set_kernel: variant must be 0..12");
    ctx->variant = variant;
    ctx->invalidate_plans();
    return WEDM_OK;
}

#ifdef WEDM_STAMPS
// diagnostic builds only (-DWEDM_STAMPS, tools/stamps*.py): device buffer receiving the phase
// cycle stamps of every wave.  Not part of the shipped library, not declared in the header.
int32_t wedm_debug_set_stamp_buffer(wedm_ctx* ctx, void* buf) {
    if (!ctx) return WEDM_ERR_BAD_ARG;
    ctx->dbg = (unsigned long long*)buf;
    return WEDM_OK;
}
#endif

int32_t wedm_set_lanes(wedm_ctx* ctx, int32_t lanes) {
    if (!ctx) return WEDM_ERR_BAD_ARG;
    if (lanes != 0 && lanes_index(lanes) < 0)
        return fail(ctx, WEDM_ERR_BAD_ARG, "wedm_set_lanes: lanes must be 0 (auto), 1, 2, 4, 8 or 16");
    ctx->lanes = lanes;
    ctx->invalidate_plans();
    return WEDM_OK;
}

int32_t wedm_reset(wedm_ctx* ctx, const uint8_t* mask, uint64_t seed, int32_t reseed, void* stream) {
    if (!ctx) return WEDM_ERR_BAD_ARG;
    if (!ctx->bound) return fail(ctx, WEDM_ERR_NOT_BOUND, "wedm_reset: call wedm_bind_state first");
    if (int32_t rc = check_device(ctx, "wedm_reset")) return rc;
    const int block = 256;
    const int grid = (ctx->num_envs + block - 1) / block;
    hipLaunchKernelGGL(wedm_reset_kernel, dim3(grid), dim3(block), 0, (hipStream_t)stream, ctx->p, ctx->s,
                       ctx->num_envs, ctx->n_seg_max, mask, (uint32_t)seed, (uint32_t)(seed >> 32), reseed);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(ctx, e, "wedm_reset launch");
    if (ctx->pulse) {  // the pulse block is not module state of the reference: cleared by every reset, either semantics
        hipLaunchKernelGGL(wedm_reset_pulse_kernel, dim3(grid), dim3(block), 0, (hipStream_t)stream, ctx->pulse, ctx->s.stride,
                           ctx->num_envs, mask);
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(ctx, e, "wedm_reset launch (pulse statistics)");
    }
    if (ctx->sig) {  // nor is the signal-statistics block: re-initialised by every reset, either semantics
        hipLaunchKernelGGL(wedm_reset_signal_kernel, dim3(grid), dim3(block), 0, (hipStream_t)stream, ctx->sig, ctx->s.stride,
                           ctx->num_envs, mask);
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(ctx, e, "wedm_reset launch (signal statistics)");
    }
    if (!mask && ctx->frozen_seen) *(volatile int32_t*)ctx->frozen_seen = 0;  // every environment reset: none is frozen
    return WEDM_OK;
}

int32_t wedm_step(wedm_ctx* ctx, int32_t n_substeps, const wedm_action_ptrs* action, void* stream) {
    if (!ctx) return WEDM_ERR_BAD_ARG;
    if (!ctx->bound) return fail(ctx, WEDM_ERR_NOT_BOUND, "wedm_step: call wedm_bind_state first");
    if (!action || !action->servo || !action->target_voltage || !action->on_time || !action->off_time ||
        !action->current_mode)
        return fail(ctx, WEDM_ERR_BAD_ARG, "wedm_step: null action leaf");
    if (n_substeps < 0) return fail(ctx, WEDM_ERR_BAD_ARG, "wedm_step: n_substeps < 0");
    if (ctx->p.per_env_geometry && !ctx->geom_bound)
        return fail(ctx, WEDM_ERR_NOT_BOUND, "wedm_step: per_env_geometry set but wedm_bind_geometry not called");
    if (n_substeps == 0) return WEDM_OK;
    if ((uint64_t)n_substeps * (uint64_t)ctx->p.dt_us >= (1ull << 31))
        return fail(ctx, WEDM_ERR_BAD_ARG, "wedm_step: n_substeps * dt_us must stay below 2^31 us per launch (the clock's high word is carried per launch)");
    if (int32_t rc = check_device(ctx, "wedm_step")) return rc;

    const wedm_params& P = ctx->p;
    KArgs k;
    Hot& h = k.hot;
    h.hard_short_gap = P.hard_short_gap; h.base_critical_density = P.base_critical_density;
    h.gap_coefficient = P.gap_coefficient; h.max_critical_density = P.max_critical_density;
    h.sigmoid_steepness = P.sigmoid_steepness;
    h.ignition_a = P.ignition_a; h.ignition_b = P.ignition_b; h.ignition_c = P.ignition_c; h.ln2 = P.ln2;
    h.default_target_voltage = P.default_target_voltage; h.default_on_time = P.default_on_time;
    h.default_off_time = P.default_off_time; h.spark_voltage_factor = P.spark_voltage_factor;
    h.debris_removal_per_us = P.debris_removal_per_us;
    h.dt_s = P.dt_s; h.damping_coeff = P.damping_coeff; h.stiffness_coeff = P.stiffness_coeff;
    h.omega_n = P.omega_n; h.max_acceleration = P.max_acceleration; h.max_jerk_dt = P.max_jerk_dt;
    h.max_speed = P.max_speed;
    h.spool = (float)P.spool_T; h.tref = (float)P.temp_ref; h.alpha = (float)P.alpha_rho;
    h.tdiel = (float)P.dielectric_temperature;
    h.tcrit = (float)P.critical_temperature; h.tbreak = (float)P.breaking_temperature;
    h.servo_interval = P.servo_interval; h.dt_us = P.dt_us; h.control_mode = P.control_mode;
    h.disable_ignition = P.disable_ignition;
    h.has_random_short = P.random_short_max_probability != 0.0 ? 1 : 0;
    h.per_env_geometry = P.per_env_geometry; h.env_id_offset = P.env_id_offset; h.n_seg = P.n_seg;
    h.done_value = P.keep_stepping_terminated ? 0 : 1;
    k.cold.p = ctx->params_dev;
    k.cold.g = ctx->g;
    k.cold.a = *action;
    k.cold.s = ctx->s;
    k.cold.tb = ctx->tb;
    k.cold.replay = ctx->replay;
    k.cold.replay_steps = ctx->replay_steps;
    k.cold.frozen_seen = ctx->frozen_seen_dev;
    k.num_envs = ctx->num_envs;
    k.n_substeps = n_substeps;
    k.n_seg_max = ctx->n_seg_max;
    k.walk = nullptr;
    k.dbg = ctx->dbg;
    k.pulse = ctx->pulse;
    k.envp = ctx->envp;
    k.wmat = ctx->wmat;
    k.sig = ctx->sig;
    k.trace = ctx->trace;
    k.trace_next = INT32_MAX;
    k.trace_slot = 0;
    if (ctx->trace_on) {
        const int64_t every = ctx->trace.every;
        k.trace_next = (int32_t)(every - ctx->trace_us % every - 1);  // 0-based substep of the next sample
        k.trace_slot = (int32_t)(ctx->trace_count % ctx->trace.capacity);
    }

    const bool tr = ctx->trace_on && k.trace_next < n_substeps;  // a sample falls into this launch
    // frozen-lane tile code: handles with in-launch autoreset, and any handle one of whose launches has found a terminated
    // environment.  The kernels set the host-visible word; the host reads it without synchronising, so the switch comes as
    // late as the host runs ahead of the device: every launch ENQUEUED before the first kernel that sets the word has run
    // still takes the instantiation without the frozen-lane code (whose waves with a frozen lane walk cell by cell: slower,
    // same results).  A reset of every environment clears the word on the host while kernels queued earlier may still
    // set it again, and masked resets never clear it: both only keep the FROZEN_OK instantiation (2 % slower on a batch
    // without frozen environments) longer than needed.  Speed only; no result depends on the word.
    const bool frozen_ok = P.autoreset || (ctx->frozen_seen && *(volatile int32_t*)ctx->frozen_seen != 0);
    LaunchPlan& plan = ctx->plans[n_substeps <= 1 ? 1 : 0][tr ? 1 : 0][frozen_ok ? 1 : 0];
    if (!plan.valid) {
        if (int32_t rc = plan_launch(ctx, n_substeps <= 1, tr, frozen_ok, plan)) return rc;
    }
    k.walk = plan.walk;
    void* kargs[] = {(void*)&k};
    hipError_t el = hipLaunchKernel(plan.fn, dim3(plan.grid), dim3(plan.block), kargs, plan.lds, (hipStream_t)stream);
    if (el != hipSuccess) return hip_fail(ctx, el, "wedm_step launch");
    ctx->last_plan = &plan;
    ctx->last_n_sub = n_substeps;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(ctx, e, "wedm_step launch");
    if (ctx->trace_on) {
        const int64_t every = ctx->trace.every;
        ctx->trace_count += (ctx->trace_us % every + n_substeps) / every;
        ctx->trace_us += n_substeps;
    }
    return WEDM_OK;
}

// ------------------------------------------------------------ the stateless entry points: what they share
// No handle: the text of a refusal goes where wedm_create's goes (wedm_last_error(NULL)).

// An entry point by name: how it refuses a call and how it reports a launch.
struct Entry {
    const char* name;
    int32_t bad(const std::string& msg) const {
        g_create_error = std::string(name) + ": " + msg;
        return WEDM_ERR_BAD_ARG;
    }
    // after every launch; `what` names it where the entry point has several
    int32_t launched(const char* what = nullptr) const {
        const hipError_t e = hipGetLastError();
        if (e == hipSuccess) return WEDM_OK;
        g_create_error = std::string(name) + ": " + (what ? std::string(what) + " launch: " : "launch: ") + hipGetErrorString(e);
        return WEDM_ERR_HIP;
    }
};

// A block of the caller's memory by name: first byte, bytes from there to one past the last the call may touch (0: the call
// leaves the block alone, so only its alignment counts), element size, whether NULL is refused; two blocks that `may_alias`
// may be the same memory; plane >= 0 puts "plane <n>" before the name.
struct Block {
    const char* name;
    uintptr_t lo, bytes, elem;
    bool needed;
    bool may_alias = false;
    int32_t plane = -1;
    std::string text() const { return plane < 0 ? name : "plane " + std::to_string(plane) + name; }
};

// The first reason why a call cannot use its blocks: an input, then an output, that is null though needed or not aligned to
// its element; then an output that overlaps an input (outputs in the outer loop).  WEDM_OK where there is none.
static int32_t check_blocks(const Entry& E, const Block* in, size_t n_in, const Block* out, size_t n_out) {
    const auto unusable = [](const Block& b) { return (b.needed && !b.lo) || b.lo % b.elem != 0; };
    for (const Block* b = in; b < in + n_in; ++b)
        if (unusable(*b)) return E.bad(b->text() + " is null or not aligned to its element");
    for (const Block* b = out; b < out + n_out; ++b)
        if (unusable(*b)) return E.bad(b->text() + " is null or not aligned to its element");
    for (const Block* o = out; o < out + n_out; ++o) {
        for (const Block* i = in; i < in + n_in; ++i) {
            if (!o->lo || !i->lo || !o->bytes || !i->bytes || (o->may_alias && i->may_alias)) continue;
            if (o->lo < i->lo + i->bytes && i->lo < o->lo + o->bytes) return E.bad(o->text() + " overlaps " + i->text());
        }
    }
    return WEDM_OK;
}

// Every block that is written against every other one (wedm_adam, wedm_minibatch_index): the first pair that shares a byte.
static int32_t check_apart(const Entry& E, const Block* out, size_t n_out) {
    for (const Block* a = out; a < out + n_out; ++a)
        for (const Block* b = a + 1; b < out + n_out; ++b)
            if (a->lo && b->lo && a->bytes && b->bytes && a->lo < b->lo + b->bytes && b->lo < a->lo + a->bytes)
                return E.bad(b->text() + " overlaps " + a->text());
    return WEDM_OK;
}

// The tiles of a batch of num_envs >= 1 environments, or 0 after refusing a tile range that leaves the workspace.
static int64_t tile_range(const Entry& E, int32_t num_envs, int32_t tile_offset, int32_t n_tiles_total) {
    const int64_t tiles = ((int64_t)num_envs + WEDM_NORM_TILE - 1) / WEDM_NORM_TILE;
    if (tile_offset >= 0 && n_tiles_total >= 1 && n_tiles_total <= WEDM_NORM_MAX_TILES && tile_offset + tiles <= n_tiles_total)
        return tiles;
    E.bad("tile range outside the workspace: tile_offset + ceil(num_envs / 256) <= n_tiles_total <= " +
          std::to_string(WEDM_NORM_MAX_TILES) + " must hold");
    return 0;
}

// Tiles per lane of a fold by 256 lanes: the smallest power of two with 256 * per >= n.
static int32_t fold_per(int64_t n) {
    int32_t per = 1;
    while (256 * per < n) per *= 2;
    return per;
}

// The leaves of a pairwise tree over `tiles` tiles: the smallest power of two >= tiles.
static int32_t fold_padded(int64_t tiles) {
    int32_t padded = 1;
    while (padded < tiles) padded *= 2;
    return padded;
}

static bool finite_f64(double x) { return x - x == 0.0; }

// What wedm_policy_head and wedm_ppo_loss ask of a head's parameters, in two parts, since the loss checks its coefficients
// between them: HEAD_SHAPE (n_modes, both strides against 8 + n_modes) and HEAD_BOUNDS (lo, hi, log_span of the four axes).
enum HeadPart { HEAD_SHAPE = 1, HEAD_BOUNDS = 2 };
static int32_t check_head_params(const Entry& E, int parts, int32_t n_modes, int64_t param_stride, int64_t grad_stride,
                                 const double* lo, const double* hi, const double* log_span) {
    if (parts & HEAD_SHAPE) {
        if (n_modes < 1 || n_modes > WEDM_HEAD_MAX_MODES) return E.bad("n_modes outside [1, " + std::to_string(WEDM_HEAD_MAX_MODES) + "]");
        if (param_stride < 8 + n_modes || grad_stride < 8 + n_modes) return E.bad("a stride is smaller than 8 + n_modes");
    }
    for (int i = 0; (parts & HEAD_BOUNDS) && i < 4; ++i) {
        if (!finite_f64(lo[i]) || !finite_f64(hi[i]) || !finite_f64(log_span[i])) return E.bad("a bound or log_span is not finite");
        if (!(hi[i] > lo[i])) return E.bad("hi <= lo");
    }
    return WEDM_OK;
}

// Whether a kernel stages the parameter rows (in) and the gradient rows (out; `grad` NULL: there are none) through LDS -- dense
// rows of P floats from a 16-byte boundary -- and the LDS that takes for a block of `block` rows.
struct StagedRows {
    bool in, out;
    size_t lds;
    StagedRows(const void* params, int64_t param_stride, const void* grad, int64_t grad_stride, int64_t P, int block)
        : in(param_stride == P && (uintptr_t)params % 16 == 0), out(grad && grad_stride == P && (uintptr_t)grad % 16 == 0),
          lds(in || out ? (size_t)block * (size_t)head_pitch((int)P) * 4 : 0) {}
};

int32_t wedm_copy_columns(const wedm_copy_plane* planes, int32_t n_planes, const int32_t* src_idx, const int32_t* dst_idx,
                          int32_t count, int32_t* status, void* stream) {
    const Entry E{"wedm_copy_columns"};
    if (!planes || n_planes < 1 || n_planes > WEDM_COPY_MAX_PLANES)
        return E.bad("null pointer or n_planes outside [1, " + std::to_string(WEDM_COPY_MAX_PLANES) + "]");
    if (count < 0 || (count > 0 && (!src_idx || !dst_idx))) return E.bad("negative count or null index list");
    wedm_copy_args a;
    std::memset(&a, 0, sizeof(a));
    int64_t items = 0;
    for (int32_t k = 0; k < n_planes; ++k) {
        const wedm_copy_plane& pl = planes[k];
        const std::string who = "plane " + std::to_string(k) + ": ";
        const int32_t w = pl.elem_bytes;
        if (w != 1 && w != 4 && w != 8 && w != 16) return E.bad(who + "elem_bytes must be 1, 4, 8 or 16");
        if (!pl.src || !pl.dst || (uintptr_t)pl.src % (uintptr_t)w || (uintptr_t)pl.dst % (uintptr_t)w)
            return E.bad(who + "null base pointer or one not aligned to elem_bytes");
        if (pl.rows < 0 || pl.src_cols < 0 || pl.dst_cols < 0) return E.bad(who + "negative rows or column count");
        if (pl.src_stride < pl.src_cols || pl.dst_stride < pl.dst_cols) return E.bad(who + "stride smaller than the column count");
        a.plane[k] = pl;
        items += (pl.rows + WEDM_COPY_ROWS - 1) / WEDM_COPY_ROWS;
        if (items > INT32_MAX) return E.bad("more rows than one call can hold");
        a.item_end[k] = (int32_t)items;
    }
    a.n_planes = n_planes;
    if (count == 0 || items == 0) return WEDM_OK;
    const int64_t max_y = 65535;
    for (int64_t item0 = 0; item0 < items; item0 += max_y) {
        a.item0 = (int32_t)item0;
        const dim3 grid((uint32_t)(((int64_t)count + 255) / 256), (uint32_t)std::min(max_y, items - item0));
        hipLaunchKernelGGL(wedm_copy_columns_kernel, grid, dim3(256), 0, (hipStream_t)stream, a, src_idx, dst_idx, count, status);
        if (const int32_t rc = E.launched()) return rc;
    }
    return WEDM_OK;
}

int32_t wedm_wire_profile(const wedm_profile_desc* desc, const int32_t* env_idx, int32_t count, int32_t* status, void* stream) {
    const Entry E{"wedm_wire_profile"};
    if (!desc) return E.bad("null descriptor");
    const wedm_profile_desc& d = *desc;
    if (!d.T || !d.out || (uintptr_t)d.T % 16) return E.bad("T or out is null, or T is not 16-byte aligned");
    if (d.bins < 0 || d.bins > WEDM_PROFILE_MAX_BINS) return E.bad("bins outside [0, " + std::to_string(WEDM_PROFILE_MAX_BINS) + "]");
    if (d.num_envs < 1 || d.n_seg_max < 1) return E.bad("num_envs and n_seg_max must be positive");
    if (d.stride < d.num_envs) return E.bad("stride smaller than num_envs");
    if (d.out_cols < 0 || d.out_cols > d.out_stride) return E.bad("out_cols outside [0, out_stride]");
    if (count < 0 || count > d.out_cols) return E.bad("count outside [0, out_cols]");
    if (!d.geom_i32 && (d.n_seg < 1 || d.n_seg > d.n_seg_max)) return E.bad("n_seg outside [1, n_seg_max] (uniform geometry)");
    if (!env_idx && count > d.num_envs) return E.bad("count exceeds num_envs without an index list");
    if (count == 0) return WEDM_OK;
    // waves per block = pieces a wire is cut into: four, and more while the launch has fewer than WEDM_PROFILE_WAVES_PER_SIMD
    // waves for each of the device's 1024 SIMDs and every piece keeps a whole batch of loads
    const int32_t quads = WEDM_T_QUADS(d.n_seg_max);
    const int64_t groups = ((int64_t)count + 63) / 64;
    int32_t waves = 4;
    while (waves < WEDM_PROFILE_MAX_WAVES && groups * waves < 1024 * WEDM_PROFILE_WAVES_PER_SIMD &&
           quads >= 2 * waves * WEDM_PROFILE_LOADS)
        waves *= 2;
    wedm_profile_args a;
    std::memset(&a, 0, sizeof(a));
    a.d = d;
    a.count = count;
    a.chunk = (quads + waves - 1) / waves;
    a.inv_b = d.bins > 0 ? ((1u << 20) + (uint32_t)d.bins - 1) / (uint32_t)d.bins : 0u;
    const dim3 grid((uint32_t)groups), block((uint32_t)waves * 64);
    const size_t lds = WEDM_PROFILE_LDS_BYTES(d.bins);
    if (d.geom_i32)
        hipLaunchKernelGGL((wedm_wire_profile_kernel<true>), grid, block, lds, (hipStream_t)stream, a, env_idx, status);
    else
        hipLaunchKernelGGL((wedm_wire_profile_kernel<false>), grid, block, lds, (hipStream_t)stream, a, env_idx, status);
    return E.launched();
}

int32_t wedm_normalize(const wedm_norm_desc* desc, void* stream) {
    const Entry E{"wedm_normalize"};
    if (!desc) return E.bad("null descriptor");
    const wedm_norm_desc& d = *desc;
    const int32_t all = WEDM_NORM_UPDATE | WEDM_NORM_STEP | WEDM_NORM_REDUCE | WEDM_NORM_APPLY;
    if (d.flags & ~all) return E.bad("undefined flag bits");
    const bool update = d.flags & WEDM_NORM_UPDATE, step = d.flags & WEDM_NORM_STEP;
    const bool both = !(d.flags & (WEDM_NORM_REDUCE | WEDM_NORM_APPLY));
    const bool reduce = both || (d.flags & WEDM_NORM_REDUCE), apply = both || (d.flags & WEDM_NORM_APPLY);
    if (d.num_envs < 1) return E.bad("num_envs must be positive");
    if (d.plane[0].n_rows < 0 || d.plane[1].n_rows < 0) return E.bad("negative n_rows");
    const int64_t D = (int64_t)d.plane[0].n_rows + d.plane[1].n_rows;
    if (D < 1 || D > WEDM_NORM_MAX_COLUMNS - 1) return E.bad("D outside [1, " + std::to_string(WEDM_NORM_MAX_COLUMNS - 1) + "]");
    for (int k = 0; k < 2; ++k) {
        if (d.plane[k].n_rows == 0) continue;
        if (!d.plane[k].rows || (uintptr_t)d.plane[k].rows % 4) return E.bad("plane " + std::to_string(k) + ": rows is null or misaligned");
        if (d.plane[k].stride < d.num_envs) return E.bad("plane " + std::to_string(k) + ": stride smaller than num_envs");
    }
    const int64_t tiles = tile_range(E, d.num_envs, d.tile_offset, d.n_tiles_total);
    if (!tiles) return WEDM_ERR_BAD_ARG;
    if (update && (!d.partials || (uintptr_t)d.partials % 8)) return E.bad("partials is null or misaligned (UPDATE)");
    if (step && (!d.reward || !d.ret || (uintptr_t)d.reward % 4 || (uintptr_t)d.ret % 8)) return E.bad("reward or ret is null or misaligned (STEP)");
    const int64_t C = D + 1;
    if (apply) {
        if (!d.obs_out || !d.stats_in || !d.stats_out || (uintptr_t)d.obs_out % 4 || (uintptr_t)d.stats_in % 8 || (uintptr_t)d.stats_out % 8)
            return E.bad("obs_out, stats_in or stats_out is null or misaligned (APPLY)");
        const uintptr_t a = (uintptr_t)d.stats_in, b = (uintptr_t)d.stats_out, bytes = (uintptr_t)(WEDM_NORM_MOMENTS * C * 8);
        if (a < b + bytes && b < a + bytes) return E.bad("stats_in and stats_out overlap");
        if (step) {
            if (!d.terminated || !d.truncated || !d.reward_out || !d.ep_return || !d.last_return || !d.ep_length || !d.last_length ||
                !d.ep_count || !d.finished)
                return E.bad("terminated, truncated, reward_out or a per-environment row is null (APPLY with STEP)");
            if ((uintptr_t)d.reward_out % 4 || (uintptr_t)d.ep_return % 8 || (uintptr_t)d.last_return % 8 || (uintptr_t)d.ep_length % 4 ||
                (uintptr_t)d.last_length % 4 || (uintptr_t)d.ep_count % 4)
                return E.bad("reward_out or a per-environment row is not aligned to its element");
        }
    }
    const dim3 grid((uint32_t)tiles), block(WEDM_NORM_TILE);
    if (reduce && (update || step)) {
        // a wave per tile and column group; in evaluation mode one wave per tile, which only moves the return on
        const int32_t c_first = update ? 0 : (int32_t)D;
        const dim3 rgrid((uint32_t)tiles, (uint32_t)((C - c_first + WEDM_NORM_GROUP - 1) / WEDM_NORM_GROUP));
        hipLaunchKernelGGL(wedm_norm_reduce_kernel, rgrid, dim3(64), 0, (hipStream_t)stream, d, (int32_t)D, c_first);
        if (const int32_t rc = E.launched("reduce")) return rc;
    }
    if (apply) {
        hipLaunchKernelGGL(wedm_norm_fold_kernel, dim3((uint32_t)C), dim3(256), 0, (hipStream_t)stream, d, (int32_t)C,
                           fold_per(d.n_tiles_total));
        if (const int32_t rc = E.launched("fold")) return rc;
        hipLaunchKernelGGL(wedm_norm_apply_kernel, grid, block, 0, (hipStream_t)stream, d, (int32_t)D);
        if (const int32_t rc = E.launched("apply")) return rc;
    }
    return WEDM_OK;
}

int32_t wedm_gae(const wedm_gae_desc* desc, void* stream) {
    const Entry E{"wedm_gae"};
    if (!desc) return E.bad("null descriptor");
    const wedm_gae_desc& d = *desc;
    const int32_t all = WEDM_GAE_SKIP_AFTER_DONE | WEDM_GAE_NORMALIZE | WEDM_GAE_SCAN | WEDM_GAE_APPLY;
    if (d.flags & ~all) return E.bad("undefined flag bits");
    const bool normalize = d.flags & WEDM_GAE_NORMALIZE;
    const bool both = !(d.flags & (WEDM_GAE_SCAN | WEDM_GAE_APPLY));
    const bool scan = both || (d.flags & WEDM_GAE_SCAN), apply = (both || (d.flags & WEDM_GAE_APPLY)) && normalize;
    if (d.num_envs < 1) return E.bad("num_envs must be positive");
    if (d.T < 1 || d.T > WEDM_GAE_MAX_STEPS) return E.bad("T outside [1, " + std::to_string(WEDM_GAE_MAX_STEPS) + "]");
    if (d.in_stride < d.num_envs || d.out_stride < d.num_envs) return E.bad("a stride is smaller than num_envs");
    const int64_t tiles = tile_range(E, d.num_envs, d.tile_offset, d.n_tiles_total);
    if (!tiles) return WEDM_ERR_BAD_ARG;
    if (!finite_f64(d.gamma) || !finite_f64(d.lam) || !finite_f64(d.eps)) return E.bad("gamma, lam and eps must be finite");
    const uintptr_t rows_in = (uintptr_t)((int64_t)(d.T - 1) * d.in_stride + d.num_envs);
    const uintptr_t rows_out = (uintptr_t)((int64_t)(d.T - 1) * d.out_stride + d.num_envs), n = (uintptr_t)d.num_envs;
    const Block in[] = {
        {"reward", (uintptr_t)d.reward, rows_in * 4, 4, scan},       {"value", (uintptr_t)d.value, rows_in * 4, 4, scan},
        {"last_value", (uintptr_t)d.last_value, n * 4, 4, scan},     {"terminated", (uintptr_t)d.terminated, rows_in, 1, scan},
        {"truncated", (uintptr_t)d.truncated, rows_in, 1, scan},     {"prev_done_in", (uintptr_t)d.prev_done_in, n, 1, false, true},
    };
    const Block out[] = {
        {"advantage", (uintptr_t)d.advantage, rows_out * 4, 4, scan || apply},
        {"returns", (uintptr_t)d.returns, rows_out * 4, 4, scan},
        {"valid", (uintptr_t)d.valid, rows_out, 1, scan || apply},
        {"advantage_norm", (uintptr_t)d.advantage_norm, rows_out * 4, 4, apply},
        {"prev_done_out", (uintptr_t)d.prev_done_out, n, 1, false, true},  // (may be prev_done_in)
        {"partials", (uintptr_t)d.partials, (uintptr_t)d.n_tiles_total * WEDM_NORM_MOMENTS * 8, 8, normalize && (scan || apply)},
        {"moments", (uintptr_t)d.moments, WEDM_NORM_MOMENTS * 8, 8, apply},
    };
    if (const int32_t rc = check_blocks(E, in, std::size(in), out, std::size(out))) return rc;
    if (scan) {
        hipLaunchKernelGGL(wedm_gae_scan_kernel, dim3((uint32_t)tiles), dim3(WEDM_NORM_TILE), 0, (hipStream_t)stream, d);
        if (const int32_t rc = E.launched("scan")) return rc;
    }
    if (apply) {
        hipLaunchKernelGGL(wedm_gae_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, d, fold_per(d.n_tiles_total));
        if (const int32_t rc = E.launched("fold")) return rc;
        const dim3 grid((uint32_t)tiles, (uint32_t)((d.T + WEDM_GAE_APPLY_ROWS - 1) / WEDM_GAE_APPLY_ROWS));
        hipLaunchKernelGGL(wedm_gae_apply_kernel, grid, dim3(WEDM_NORM_TILE), 0, (hipStream_t)stream, d);
        if (const int32_t rc = E.launched("apply")) return rc;
    }
    return WEDM_OK;
}

int32_t wedm_policy_head(const wedm_head_desc* desc, void* stream) {
    const Entry E{"wedm_policy_head"};
    if (!desc) return E.bad("null descriptor");
    const wedm_head_desc& d = *desc;
    if (d.op != WEDM_HEAD_SAMPLE && d.op != WEDM_HEAD_EVALUATE && d.op != WEDM_HEAD_BACKWARD) return E.bad("undefined op");
    if (d.flags & ~(int32_t)WEDM_HEAD_DETERMINISTIC) return E.bad("undefined flag bits");
    if (d.flags && d.op != WEDM_HEAD_SAMPLE) return E.bad("a flag with another op than SAMPLE");
    if (d.rows < 1) return E.bad("rows must be positive");
    const bool sample = d.op == WEDM_HEAD_SAMPLE, backward = d.op == WEDM_HEAD_BACKWARD;
    if (const int32_t rc = check_head_params(E, HEAD_SHAPE | HEAD_BOUNDS, d.n_modes, d.param_stride,
                                             backward ? d.grad_stride : d.param_stride, d.lo, d.hi, d.log_span))
        return rc;
    const int64_t P = 8 + d.n_modes;
    // rows of the blocks only SAMPLE, only BACKWARD, all but BACKWARD touch: none for the other ops, which leave them alone
    const uintptr_t n = (uintptr_t)d.rows, ns = sample ? n : 0, nb = backward ? n : 0, nf = backward ? 0 : n;
    const uintptr_t row_bytes = (uintptr_t)((int64_t)(d.rows - 1) * d.param_stride + P) * 4;
    const uintptr_t grad_bytes = backward ? (uintptr_t)((int64_t)(d.rows - 1) * d.grad_stride + P) * 4 : 0;
    const Block blocks[] = {
        {"params", (uintptr_t)d.params, row_bytes, 4, true},
        {"u", (uintptr_t)d.u, n * 16, 16, true},
        {"mode_index", (uintptr_t)d.mode_index, n * 4, 4, true},
        {"g_log_prob", (uintptr_t)d.g_log_prob, nb * 4, 4, backward},
        {"g_entropy", (uintptr_t)d.g_entropy, nb * 4, 4, false},
        {"action[0]", (uintptr_t)d.action[0], ns * 8, 8, sample},
        {"action[1]", (uintptr_t)d.action[1], ns * 8, 8, sample},
        {"action[2]", (uintptr_t)d.action[2], ns * 8, 8, sample},
        {"action[3]", (uintptr_t)d.action[3], ns * 8, 8, sample},
        {"current_mode", (uintptr_t)d.current_mode, ns * 4, 4, sample},
        {"log_prob", (uintptr_t)d.log_prob, nf * 4, 4, !backward},
        {"entropy", (uintptr_t)d.entropy, nf * 4, 4, !backward},
        {"grad_params", (uintptr_t)d.grad_params, grad_bytes, 4, backward},
    };
    // what the op reads comes first: params; u and mode_index, SAMPLE's outputs, for the others; the two gradients for BACKWARD
    const size_t n_in = sample ? 1 : backward ? 5 : 3;
    if (const int32_t rc = check_blocks(E, blocks, n_in, blocks + n_in, std::size(blocks) - n_in)) return rc;
    const StagedRows staged(d.params, d.param_stride, backward ? d.grad_params : nullptr, d.grad_stride, P, WEDM_HEAD_BLOCK);
    const dim3 grid((uint32_t)(((int64_t)d.rows + WEDM_HEAD_BLOCK - 1) / WEDM_HEAD_BLOCK)), block(WEDM_HEAD_BLOCK);
    const hipStream_t s = (hipStream_t)stream;
    if (sample) {
        if (staged.in) hipLaunchKernelGGL((wedm_head_kernel<WEDM_HEAD_SAMPLE, true, false>), grid, block, staged.lds, s, d);
        else hipLaunchKernelGGL((wedm_head_kernel<WEDM_HEAD_SAMPLE, false, false>), grid, block, staged.lds, s, d);
    } else if (!backward) {
        if (staged.in) hipLaunchKernelGGL((wedm_head_kernel<WEDM_HEAD_EVALUATE, true, false>), grid, block, staged.lds, s, d);
        else hipLaunchKernelGGL((wedm_head_kernel<WEDM_HEAD_EVALUATE, false, false>), grid, block, staged.lds, s, d);
    } else if (staged.in) {
        if (staged.out) hipLaunchKernelGGL((wedm_head_kernel<WEDM_HEAD_BACKWARD, true, true>), grid, block, staged.lds, s, d);
        else hipLaunchKernelGGL((wedm_head_kernel<WEDM_HEAD_BACKWARD, true, false>), grid, block, staged.lds, s, d);
    } else {
        if (staged.out) hipLaunchKernelGGL((wedm_head_kernel<WEDM_HEAD_BACKWARD, false, true>), grid, block, staged.lds, s, d);
        else hipLaunchKernelGGL((wedm_head_kernel<WEDM_HEAD_BACKWARD, false, false>), grid, block, staged.lds, s, d);
    }
    return E.launched();
}

int32_t wedm_ppo_loss(const wedm_ppo_desc* desc, void* stream) {
    const Entry E{"wedm_ppo_loss"};
    if (!desc) return E.bad("null descriptor");
    const wedm_ppo_desc& d = *desc;
    if (d.flags & ~(int32_t)(WEDM_PPO_CLIP_VALUE | WEDM_PPO_COUNT | WEDM_PPO_MAIN | WEDM_PPO_FOLD)) return E.bad("undefined flag bits");
    if (d.rows < 1) return E.bad("rows must be positive");
    const int64_t tiles = ((int64_t)d.rows + WEDM_PPO_BLOCK - 1) / WEDM_PPO_BLOCK;
    if (tiles > WEDM_NORM_MAX_TILES)
        return E.bad("a minibatch holds at most " + std::to_string(WEDM_NORM_MAX_TILES * WEDM_PPO_BLOCK) + " rows (" +
                     std::to_string(WEDM_NORM_MAX_TILES) + " tiles of 256)");
    if (d.n_src < 1) return E.bad("n_src must be positive");
    if (const int32_t rc = check_head_params(E, HEAD_SHAPE, d.n_modes, d.param_stride, d.grad_stride, d.lo, d.hi, d.log_span)) return rc;
    const int64_t P = 8 + d.n_modes;
    if (!finite_f64(d.clip) || !finite_f64(d.vf_coef) || !finite_f64(d.ent_coef) || !finite_f64(d.clip_value))
        return E.bad("clip, vf_coef, ent_coef and clip_value must be finite");
    if (d.clip < 0.0 || d.clip_value < 0.0) return E.bad("clip and clip_value must not be negative");
    if (const int32_t rc = check_head_params(E, HEAD_BOUNDS, d.n_modes, d.param_stride, d.grad_stride, d.lo, d.hi, d.log_span)) return rc;
    const bool all = !(d.flags & (WEDM_PPO_COUNT | WEDM_PPO_MAIN | WEDM_PPO_FOLD));
    const bool counted = d.valid || d.index;  // the number of live rows is not the host's to know
    const bool count = (all || (d.flags & WEDM_PPO_COUNT)) && counted, rows_pass = all || (d.flags & WEDM_PPO_MAIN);
    const bool fold = all || (d.flags & WEDM_PPO_FOLD), clip_value = d.flags & WEDM_PPO_CLIP_VALUE;
    const uintptr_t n = (uintptr_t)d.rows, ns = (uintptr_t)d.n_src;
    const Block in[] = {
        {"params", (uintptr_t)d.params, (uintptr_t)((int64_t)(d.rows - 1) * d.param_stride + P) * 4, 4, rows_pass},
        {"value", (uintptr_t)d.value, n * 4, 4, rows_pass},
        {"index", (uintptr_t)d.index, n * 8, 8, false},
        {"u", (uintptr_t)d.u, ns * 16, 16, rows_pass},
        {"mode_index", (uintptr_t)d.mode_index, ns * 4, 4, rows_pass},
        {"old_log_prob", (uintptr_t)d.old_log_prob, ns * 4, 4, rows_pass},
        {"advantage", (uintptr_t)d.advantage, ns * 4, 4, rows_pass},
        {"returns", (uintptr_t)d.returns, ns * 4, 4, rows_pass},
        {"old_value", (uintptr_t)d.old_value, ns * 4, 4, rows_pass && clip_value},
        {"valid", (uintptr_t)d.valid, ns, 1, false},
    };
    const Block out[] = {
        {"grad_params", (uintptr_t)d.grad_params, (uintptr_t)((int64_t)(d.rows - 1) * d.grad_stride + P) * 4, 4, false},
        {"grad_value", (uintptr_t)d.grad_value, n * 4, 4, false},
        {"partials", (uintptr_t)d.partials, (uintptr_t)tiles * WEDM_PPO_SUMS * 8, 8, rows_pass || fold},
        {"stats", (uintptr_t)d.stats, WEDM_PPO_STATS * 8, 8, fold},
        {"count", (uintptr_t)d.count, WEDM_PPO_COUNT_WORDS * 4, 4, counted && (count || rows_pass)},
    };
    if (const int32_t rc = check_blocks(E, in, std::size(in), out, std::size(out))) return rc;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((uint32_t)tiles), block(WEDM_PPO_BLOCK);
    if (count) {
        hipLaunchKernelGGL(wedm_ppo_zero_kernel, dim3(1), dim3(64), 0, s, d);
        if (const int32_t rc = E.launched("zero")) return rc;
        hipLaunchKernelGGL(wedm_ppo_count_kernel, dim3((uint32_t)std::min<int64_t>(tiles, WEDM_PPO_COUNT_BLOCKS)), block, 0, s, d);
        if (const int32_t rc = E.launched("count")) return rc;
    }
    if (rows_pass) {
        const StagedRows staged(d.params, d.param_stride, d.grad_params, d.grad_stride, P, WEDM_PPO_BLOCK);
        const int32_t n_known = counted ? -1 : d.rows;
        if (staged.in) {
            if (staged.out) hipLaunchKernelGGL((wedm_ppo_main_kernel<true, true>), grid, block, staged.lds, s, d, n_known);
            else hipLaunchKernelGGL((wedm_ppo_main_kernel<true, false>), grid, block, staged.lds, s, d, n_known);
        } else {
            if (staged.out) hipLaunchKernelGGL((wedm_ppo_main_kernel<false, true>), grid, block, staged.lds, s, d, n_known);
            else hipLaunchKernelGGL((wedm_ppo_main_kernel<false, false>), grid, block, staged.lds, s, d, n_known);
        }
        if (const int32_t rc = E.launched("main")) return rc;
    }
    if (fold) {
        hipLaunchKernelGGL(wedm_ppo_fold_kernel, dim3(1), dim3(256), 0, s, d, (int32_t)tiles, fold_padded(tiles), fold_per(tiles));
        if (const int32_t rc = E.launched("fold")) return rc;
    }
    return WEDM_OK;
}

int32_t wedm_policy_net(const wedm_net_desc* desc, void* stream) {
    const Entry E{"wedm_policy_net"};
    if (!desc) return E.bad("null descriptor");
    const wedm_net_desc& d = *desc;
    const int32_t phases = WEDM_NET_FORWARD | WEDM_NET_BACKWARD | WEDM_NET_FOLD;
    if (d.flags & ~(int32_t)(phases | WEDM_NET_ACCUMULATE)) return E.bad("undefined flag bits");
    if (!(d.flags & phases)) return E.bad("no phase: FORWARD, BACKWARD or FOLD must be set");
    if (d.rows < 1) return E.bad("rows must be positive");
    const int64_t tiles = ((int64_t)d.rows + WEDM_NORM_TILE - 1) / WEDM_NORM_TILE;
    if (tiles > WEDM_NORM_MAX_TILES)
        return E.bad("a minibatch holds at most " + std::to_string(WEDM_NORM_MAX_TILES * WEDM_NORM_TILE) + " rows (" +
                     std::to_string(WEDM_NORM_MAX_TILES) + " tiles of 256)");
    if (d.n_src < 1) return E.bad("n_src must be positive");
    if (d.obs_dim < 1 || d.obs_dim > WEDM_NORM_MAX_COLUMNS) return E.bad("obs_dim outside [1, " + std::to_string(WEDM_NORM_MAX_COLUMNS) + "]");
    for (const int32_t h : {d.hidden1, d.hidden2})
        if (h < 16 || h > WEDM_NET_MAX_HIDDEN || h % 16) return E.bad("a hidden width is not a multiple of 16 in [16, " + std::to_string(WEDM_NET_MAX_HIDDEN) + "]");
    if (d.n_modes < 1 || d.n_modes > WEDM_HEAD_MAX_MODES) return E.bad("n_modes outside [1, " + std::to_string(WEDM_HEAD_MAX_MODES) + "]");
    if (d.activation != WEDM_NET_RELU && d.activation != WEDM_NET_TANH) return E.bad("activation is neither WEDM_NET_RELU nor WEDM_NET_TANH");
    const bool fwd = d.flags & WEDM_NET_FORWARD, bwd = d.flags & WEDM_NET_BACKWARD, fold = d.flags & WEDM_NET_FOLD;
    const int64_t P = 8 + d.n_modes;
    if ((fwd || bwd) && d.obs_stride < d.obs_dim) return E.bad("obs_stride is smaller than obs_dim");
    if ((fwd && d.param_stride < P) || (bwd && d.grad_stride < P)) return E.bad("a stride is smaller than 8 + n_modes");
    const net_shape F = net_make_shape(d.obs_dim, d.hidden1, d.hidden2, (int)P + 1, false);
    const net_shape B = net_make_shape(d.obs_dim, d.hidden1, d.hidden2, (int)P + 1, true);
    const uintptr_t n = (uintptr_t)d.rows, nt = (uintptr_t)F.n_theta;
    const Block in[] = {
        {"theta", (uintptr_t)d.theta, nt * 4, 4, fwd || bwd},
        {"obs", (uintptr_t)d.obs, (fwd || bwd) ? (uintptr_t)((d.n_src - 1) * d.obs_stride + d.obs_dim) * 4 : 0, 4, fwd || bwd},
        {"index", (uintptr_t)d.index, n * 8, 8, false},
        {"grad_params", (uintptr_t)d.grad_params, bwd ? (uintptr_t)((int64_t)(d.rows - 1) * d.grad_stride + P) * 4 : 0, 4, bwd},
        {"grad_value", (uintptr_t)d.grad_value, bwd ? n * 4 : 0, 4, bwd},
    };
    const Block out[] = {
        {"params", (uintptr_t)d.params, fwd ? (uintptr_t)((int64_t)(d.rows - 1) * d.param_stride + P) * 4 : 0, 4, fwd},
        {"value", (uintptr_t)d.value, fwd ? n * 4 : 0, 4, fwd},
        {"partials", (uintptr_t)d.partials, (bwd || fold) ? (uintptr_t)tiles * nt * 4 : 0, 4, bwd || fold},
        {"grad_theta", (uintptr_t)d.grad_theta, fold ? nt * 4 : 0, 4, fold},
    };
    if (const int32_t rc = check_blocks(E, in, std::size(in), out, std::size(out))) return rc;
    const hipStream_t s = (hipStream_t)stream;
    const bool tanh_act = d.activation == WEDM_NET_TANH;
    const auto lds_ok = [&](const void* fn, size_t bytes) {  // a block's LDS above the default limit has to be asked for
        return bytes <= 64 * 1024 || hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, WEDM_NET_LDS_LIMIT) == hipSuccess;
    };
    const auto launch = [&](auto bwd_tag, const net_shape& S, const dim3 grid, const char* what) -> int32_t {
        constexpr bool BWD = decltype(bwd_tag)::value;
        const size_t lds = (size_t)S.lds_floats * 4;
        void (*fn)(const wedm_net_desc) =
            S.wts >= 0 ? (tanh_act ? wedm_net_kernel<BWD, true, true> : wedm_net_kernel<BWD, false, true>)
                       : (tanh_act ? wedm_net_kernel<BWD, true, false> : wedm_net_kernel<BWD, false, false>);
        if (!lds_ok((const void*)fn, lds)) return E.launched(what);
        hipLaunchKernelGGL(fn, grid, dim3(WEDM_NET_BLOCK), lds, s, d);
        return E.launched(what);
    };
    if (fwd)
        if (const int32_t rc = launch(std::false_type{}, F, dim3((uint32_t)(((int64_t)d.rows + WEDM_NET_PASS - 1) / WEDM_NET_PASS)), "forward")) return rc;
    if (bwd)
        if (const int32_t rc = launch(std::true_type{}, B, dim3((uint32_t)tiles), "main")) return rc;
    if (fold) {
        hipLaunchKernelGGL(wedm_net_fold_kernel, dim3((uint32_t)((F.n_theta + WEDM_NET_FOLD_PARAMS - 1) / WEDM_NET_FOLD_PARAMS)), dim3(256), 0, s, d,
                           (int32_t)F.n_theta, (int32_t)tiles, std::max(fold_padded(tiles) / 8, 1), (int32_t)((d.flags & WEDM_NET_ACCUMULATE) != 0));
        if (const int32_t rc = E.launched("fold")) return rc;
    }
    return WEDM_OK;
}

int32_t wedm_adam(const wedm_opt_desc* desc, void* stream) {
    const Entry E{"wedm_adam"};
    if (!desc) return E.bad("null descriptor");
    const wedm_opt_desc& d = *desc;
    const int32_t phases = WEDM_OPT_NORM | WEDM_OPT_DECIDE | WEDM_OPT_APPLY;
    if (d.flags & ~(int32_t)(phases | WEDM_OPT_CLIP | WEDM_OPT_KL_GATE | WEDM_OPT_NEW_UPDATE)) return E.bad("undefined flag bits");
    if (d.n < 1) return E.bad("n must be positive");
    const int64_t tiles = ((int64_t)d.n + WEDM_ADAM_BLOCK - 1) / WEDM_ADAM_BLOCK;
    if (tiles > WEDM_NORM_MAX_TILES)
        return E.bad("a parameter block holds at most " + std::to_string(WEDM_NORM_MAX_TILES * WEDM_ADAM_BLOCK) + " entries (" +
                     std::to_string(WEDM_NORM_MAX_TILES) + " tiles of 256)");
    const bool clip = d.flags & WEDM_OPT_CLIP, gate = d.flags & WEDM_OPT_KL_GATE;
    if (!finite_f64(d.lr) || d.lr < 0.0) return E.bad("lr must be finite and not negative");
    if (!(d.beta1 >= 0.0 && d.beta1 < 1.0) || !(d.beta2 >= 0.0 && d.beta2 < 1.0)) return E.bad("beta1 and beta2 must lie in [0, 1)");
    if (!finite_f64(d.eps) || !(d.eps > 0.0)) return E.bad("eps must be finite and positive");
    if (!finite_f64(d.weight_decay) || d.weight_decay < 0.0) return E.bad("weight_decay must be finite and not negative");
    if (clip && (!finite_f64(d.max_norm) || !(d.max_norm > 0.0))) return E.bad("max_norm must be finite and positive");
    if (gate && (!finite_f64(d.kl_limit) || d.kl_limit < 0.0)) return E.bad("kl_limit must be finite and not negative");
    const bool all = !(d.flags & phases);
    const bool norm = all || (d.flags & WEDM_OPT_NORM), decide = all || (d.flags & WEDM_OPT_DECIDE), apply = all || (d.flags & WEDM_OPT_APPLY);
    const uintptr_t n = (uintptr_t)d.n;
    const Block in[] = {
        {"grad", (uintptr_t)d.grad, (norm || apply) ? n * 4 : 0, 4, norm || apply},
        {"kl", (uintptr_t)d.kl, (uintptr_t)((decide && gate) ? 8 : 0), 8, decide && gate},
    };
    const Block out[] = {
        {"theta", (uintptr_t)d.theta, apply ? n * 4 : 0, 4, apply},
        {"m", (uintptr_t)d.m, apply ? n * 4 : 0, 4, apply},
        {"v", (uintptr_t)d.v, apply ? n * 4 : 0, 4, apply},
        {"partials", (uintptr_t)d.partials, (norm || decide) ? (uintptr_t)tiles * 8 : 0, 8, norm || decide},
        {"state", (uintptr_t)d.state, (uintptr_t)(decide ? WEDM_OPT_STATE * 8 : 0), 8, decide},
        {"info", (uintptr_t)d.info, (uintptr_t)((decide || apply) ? WEDM_OPT_INFO * 8 : 0), 8, decide || apply},
    };
    if (const int32_t rc = check_blocks(E, in, std::size(in), out, std::size(out))) return rc;
    if (const int32_t rc = check_apart(E, out, std::size(out))) return rc;
    const hipStream_t s = (hipStream_t)stream;
    const int32_t padded = fold_padded(tiles);
    if (all && d.n <= WEDM_OPT_ONE_BLOCK_MAX) {
        const uint32_t lanes = (uint32_t)std::min<int64_t>(tiles * WEDM_ADAM_BLOCK, WEDM_ADAM_ONE_BLOCK);
        hipLaunchKernelGGL(wedm_adam_one_kernel, dim3(1), dim3(lanes), 0, s, d, (int32_t)tiles, padded);
        return E.launched("one-block");
    }
    if (norm) {
        hipLaunchKernelGGL(wedm_adam_norm_kernel, dim3((uint32_t)tiles), dim3(WEDM_ADAM_BLOCK), 0, s, d);
        if (const int32_t rc = E.launched("norm")) return rc;
    }
    if (decide) {
        hipLaunchKernelGGL(wedm_adam_decide_kernel, dim3(1), dim3(64), 0, s, d, (int32_t)tiles, padded);
        if (const int32_t rc = E.launched("decide")) return rc;
    }
    if (apply) {
        hipLaunchKernelGGL(wedm_adam_apply_kernel, dim3((uint32_t)tiles), dim3(WEDM_ADAM_BLOCK), 0, s, d);
        if (const int32_t rc = E.launched("apply")) return rc;
    }
    return WEDM_OK;
}

int32_t wedm_minibatch_index(const wedm_mb_desc* desc, void* stream) {
    const Entry E{"wedm_minibatch_index"};
    if (!desc) return E.bad("null descriptor");
    const wedm_mb_desc& d = *desc;
    const int32_t phases = WEDM_MB_COUNT | WEDM_MB_OFFSETS | WEDM_MB_SCATTER;
    if (d.flags & ~phases) return E.bad("undefined flag bits");
    if (d.rows < 1 || d.rows > WEDM_MB_MAX_ROWS) return E.bad("rows outside [1, " + std::to_string(WEDM_MB_MAX_ROWS) + "]");
    if (d.n_parts < 1 || d.n_parts > std::min<int32_t>(d.rows, WEDM_MB_MAX_PARTS))
        return E.bad("n_parts outside [1, min(rows, " + std::to_string(WEDM_MB_MAX_PARTS) + ")]");
    const bool every = !(d.flags & phases);
    const bool count = every || (d.flags & WEDM_MB_COUNT), offsets = every || (d.flags & WEDM_MB_OFFSETS);
    const bool scatter = every || (d.flags & WEDM_MB_SCATTER);
    const int32_t tiles = (d.rows + WEDM_MB_TILE - 1) / WEDM_MB_TILE;
    const uintptr_t rows = (uintptr_t)d.rows, ws = (uintptr_t)tiles * 4;
    const Block in[] = {{"valid", (uintptr_t)d.valid, (count || scatter) ? rows : 0, 1, false}};
    const Block out[] = {
        {"index", (uintptr_t)d.index, scatter ? rows * 8 : 0, 8, scatter},
        {"count", (uintptr_t)d.count, (uintptr_t)((offsets || scatter) ? 16 : 0), 8, offsets || scatter},
        {"tile_counts", (uintptr_t)d.tile_counts, (count || offsets) ? ws : 0, 4, count || offsets},
        {"tile_base", (uintptr_t)d.tile_base, (offsets || scatter) ? ws : 0, 4, offsets || scatter},
    };
    if (const int32_t rc = check_blocks(E, in, std::size(in), out, std::size(out))) return rc;
    if (const int32_t rc = check_apart(E, out, std::size(out))) return rc;
    const hipStream_t s = (hipStream_t)stream;
    if (count) {
        hipLaunchKernelGGL(wedm_mb_count_kernel, dim3((uint32_t)tiles), dim3(WEDM_MB_BLOCK), 0, s, d);
        if (const int32_t rc = E.launched("count")) return rc;
    }
    if (offsets) {
        hipLaunchKernelGGL(wedm_mb_offsets_kernel, dim3(1), dim3(WEDM_MB_SCAN_BLOCK), 0, s, d, tiles);
        if (const int32_t rc = E.launched("offsets")) return rc;
    }
    if (scatter) {
        hipLaunchKernelGGL(wedm_mb_scatter_kernel, dim3((uint32_t)tiles), dim3(WEDM_MB_BLOCK), 0, s, d);
        if (const int32_t rc = E.launched("scatter")) return rc;
    }
    return WEDM_OK;
}

int32_t wedm_episode_log(const wedm_elog_desc* desc, void* stream) {
    const Entry E{"wedm_episode_log"};
    if (!desc) return E.bad("null descriptor");
    const wedm_elog_desc& d = *desc;
    const int32_t phases = WEDM_ELOG_COUNT | WEDM_ELOG_SCATTER | WEDM_ELOG_COMMIT;
    if (d.flags & ~phases) return E.bad("undefined flag bits");
    const bool every = !(d.flags & phases);
    const bool count = every || (d.flags & WEDM_ELOG_COUNT), scatter = every || (d.flags & WEDM_ELOG_SCATTER);
    const bool commit = every || (d.flags & WEDM_ELOG_COMMIT);
    if (d.num_envs < 1) return E.bad("num_envs must be positive");
    if (d.capacity < 1) return E.bad("capacity must be positive");
    const int64_t tiles = tile_range(E, d.num_envs, d.tile_offset, d.n_tiles_total);
    if (!tiles) return WEDM_ERR_BAD_ARG;
    if (d.n_planes < 1 || d.n_planes > WEDM_ELOG_MAX_PLANES)
        return E.bad("n_planes outside [1, " + std::to_string(WEDM_ELOG_MAX_PLANES) + "]");
    std::vector<Block> in, out;
    const uintptr_t n = (uintptr_t)d.num_envs, cap = (uintptr_t)d.capacity;
    int64_t rows_in_all = 0;
    for (int32_t p = 0; p < d.n_planes; ++p) {
        const wedm_elog_plane& pl = d.plane[p];
        const std::string who = "plane " + std::to_string(p);
        if (pl.n_rows < 1) return E.bad(who + ": n_rows must be positive");
        rows_in_all += pl.n_rows;
        if (pl.kind < WEDM_ELOG_LAST || pl.kind > WEDM_ELOG_SUM_I32) return E.bad(who + ": kind is not defined");
        const bool sum = pl.kind != WEDM_ELOG_LAST;
        if (sum ? pl.elem_bytes != (pl.kind == WEDM_ELOG_SUM_F64 ? 8 : 4) : (pl.elem_bytes != 1 && pl.elem_bytes != 4 && pl.elem_bytes != 8))
            return E.bad(who + ": elem_bytes is not one its kind takes (LAST: 1, 4 or 8; SUM_F32 and SUM_I32: 4; SUM_F64: 8)");
        if (pl.src_stride < d.num_envs) return E.bad(who + ": stride smaller than num_envs");
        const uintptr_t eb = (uintptr_t)pl.elem_bytes, r1 = (uintptr_t)(pl.n_rows - 1);
        in.push_back({".src", (uintptr_t)pl.src, (r1 * (uintptr_t)pl.src_stride + n) * eb, eb, scatter, false, p});
        out.push_back({".dst", (uintptr_t)pl.dst, (r1 * cap + cap) * (sum ? 8 : eb), sum ? 8 : eb, scatter, false, p});
        if (sum) out.push_back({".acc", (uintptr_t)pl.acc, (r1 * n + n) * 8, 8, scatter, false, p});
    }
    if (rows_in_all > WEDM_ELOG_MAX_ROWS) return E.bad("more than " + std::to_string(WEDM_ELOG_MAX_ROWS) + " rows in all");
    in.push_back({"terminated", (uintptr_t)d.terminated, n, 1, count || scatter});
    in.push_back({"truncated", (uintptr_t)d.truncated, n, 1, false});
    in.push_back({"mask", (uintptr_t)d.mask, n, 1, false});
    out.push_back({"env_out", (uintptr_t)d.env_out, cap * 8, 8, scatter});
    out.push_back({"stamp_out", (uintptr_t)d.stamp_out, cap * 8, 8, scatter});
    out.push_back({"head", (uintptr_t)d.head, 16, 8, scatter || commit});
    out.push_back({"tile_counts", (uintptr_t)d.tile_counts, (uintptr_t)d.n_tiles_total * 4, 4, true});
    if (const int32_t rc = check_blocks(E, in.data(), in.size(), out.data(), out.size())) return rc;
    const hipStream_t s = (hipStream_t)stream;
    if (count) {
        hipLaunchKernelGGL(wedm_elog_count_kernel, dim3((uint32_t)tiles), dim3(WEDM_NORM_TILE), 0, s, d);
        if (const int32_t rc = E.launched("count")) return rc;
    }
    if (scatter) {
        hipLaunchKernelGGL(wedm_elog_scatter_kernel, dim3((uint32_t)tiles, (uint32_t)d.n_planes), dim3(WEDM_NORM_TILE), 0, s, d);
        if (const int32_t rc = E.launched("scatter")) return rc;
    }
    if (commit) {
        hipLaunchKernelGGL(wedm_elog_commit_kernel, dim3(1), dim3(64), 0, s, d);
        if (const int32_t rc = E.launched("commit")) return rc;
    }
    return WEDM_OK;
}

int32_t wedm_reward(const wedm_reward_desc* desc, void* stream) {
    const Entry E{"wedm_reward"};
    if (!desc) return E.bad("null descriptor");
    const wedm_reward_desc& d = *desc;
    if (d.num_envs < 1) return E.bad("num_envs must be positive");
    if (d.stride < d.num_envs) return E.bad("stride smaller than num_envs");
    if (d.terms_out && d.terms_stride < d.num_envs) return E.bad("terms_stride smaller than num_envs");
    for (int k = 0; k < WEDM_RW_COUNT; ++k)
        if (!finite_f64(d.weight[k])) return E.bad("weight " + std::to_string(k) + " is not finite");
    if (!finite_f64(d.pos_restart) || !finite_f64(d.gap_floor) || !finite_f64(d.tmax_ceiling))
        return E.bad("pos_restart, gap_floor or tmax_ceiling is not finite");
    const auto on = [&d](int k) { return d.weight[k] != 0.0; };
    const bool progress = on(WEDM_RW_PROGRESS), flags = on(WEDM_RW_WIRE_BREAK) || on(WEDM_RW_TARGET);
    const bool pulse = on(WEDM_RW_SPARKS) || on(WEDM_RW_SHORTS) || on(WEDM_RW_SHORT_STEPS);
    const bool sig = on(WEDM_RW_ENERGY) || on(WEDM_RW_GAP_BELOW) || on(WEDM_RW_TMAX_ABOVE);
    const uintptr_t n = (uintptr_t)d.num_envs, S = (uintptr_t)d.stride;
    // rows [first, last] of a state block of `elem`-byte elements: from the first row's first byte to the last row's column n
    const auto rows = [n, S](const char* name, const void* base, int first, int last, uintptr_t elem, bool needed) {
        return Block{name, base ? (uintptr_t)base + (uintptr_t)first * S * elem : 0, ((uintptr_t)(last - first) * S + n) * elem, elem, needed};
    };
    const Block in[] = {
        rows("f64", d.f64, WEDM_F_WORKPIECE_POS, WEDM_F_WORKPIECE_POS, 8, progress),
        rows("i8", d.i8, WEDM_B_WIRE_BROKEN, WEDM_B_TARGET_REACHED, 1, flags),
        rows("pulse", d.pulse, WEDM_P_SPARK_ACC, WEDM_P_SHORT_STEPS_ACC, 4, pulse),
        rows("sig", d.sig, WEDM_SG_SAMPLES_ACC, WEDM_SG_TMAX_PEAK_ACC, 8, sig),
        {"pos_before", (uintptr_t)d.pos_before, n * 8, 8, progress},
        {"restart", (uintptr_t)d.restart, n, 1, false},
        {"mask", (uintptr_t)d.mask, n, 1, false},
    };
    const Block out[] = {
        {"reward_out", (uintptr_t)d.reward_out, n * 4, 4, true},
        {"terms_out", (uintptr_t)d.terms_out, ((uintptr_t)(WEDM_RW_COUNT - 1) * (uintptr_t)d.terms_stride + n) * 8, 8, false},
    };
    if (const int32_t rc = check_blocks(E, in, std::size(in), out, std::size(out))) return rc;
    if (const int32_t rc = check_apart(E, out, std::size(out))) return rc;
    hipLaunchKernelGGL(wedm_reward_kernel, dim3((uint32_t)((d.num_envs + WEDM_RW_BLOCK - 1) / WEDM_RW_BLOCK)), dim3(WEDM_RW_BLOCK), 0,
                       (hipStream_t)stream, d);
    return E.launched();
}

int32_t wedm_sensor(const wedm_sensor_desc* desc, void* stream) {
    const Entry E{"wedm_sensor"};
    if (!desc) return E.bad("null descriptor");
    const wedm_sensor_desc& d = *desc;
    if (d.flags != 0) return E.bad("undefined flag bits");
    if (d.num_envs < 1) return E.bad("num_envs must be positive");
    if (d.plane[0].n_rows < 0 || d.plane[1].n_rows < 0) return E.bad("negative n_rows");
    const int64_t C_in = (int64_t)d.plane[0].n_rows + d.plane[1].n_rows, C_out = d.n_out;
    const std::string columns = " outside [1, " + std::to_string(WEDM_NORM_MAX_COLUMNS - 1) + "]";
    if (C_in < 1 || C_in > WEDM_NORM_MAX_COLUMNS - 1) return E.bad("C_in" + columns);
    if (C_out < 1 || C_out > WEDM_NORM_MAX_COLUMNS - 1) return E.bad("n_out" + columns);
    const int64_t L = d.ring_len;
    if (L < 1 || L > WEDM_SENSOR_MAX_DELAY + 1) return E.bad("ring_len outside [1, " + std::to_string(WEDM_SENSOR_MAX_DELAY + 1) + "]");
    const bool ringed = L > 1;
    if (ringed && !d.ring) return E.bad("ring is null though ring_len > 1");
    for (int k = 0; k < 2; ++k)
        if (d.plane[k].n_rows > 0 && d.plane[k].stride < d.num_envs) return E.bad("plane " + std::to_string(k) + ": stride smaller than num_envs");
    if (d.out_stride < d.num_envs) return E.bad("out_stride smaller than num_envs");
    if (ringed && d.ring_stride < d.num_envs) return E.bad("ring_stride smaller than num_envs");
    const uintptr_t n = (uintptr_t)d.num_envs;
    // a struct-of-arrays block of `rows` float32 rows: from its first byte to column n of its last row
    const auto soa = [n](uintptr_t rows, int64_t stride) { return rows ? ((rows - 1) * (uintptr_t)stride + n) * 4 : (uintptr_t)0; };
    const auto plane = [&](int k) {
        const wedm_norm_plane& p = d.plane[k];
        const bool used = p.n_rows > 0;
        return Block{" rows", used ? (uintptr_t)p.rows : 0, used ? soa((uintptr_t)p.n_rows, p.stride) : 0, 4, used, false, k};
    };
    const Block in[] = {
        plane(0), plane(1),
        {"chan", (uintptr_t)d.chan, (uintptr_t)(WEDM_SENSOR_FIELDS * C_out * 8), 8, true},
        {"route", (uintptr_t)d.route, (uintptr_t)(WEDM_SENSOR_ROUTES * C_out * 4), 4, true},
        {"first", (uintptr_t)d.first, n, 1, false},
        {"mask", (uintptr_t)d.mask, n, 1, false},
        {"episode", (uintptr_t)d.episode, n * 8, 8, false},
    };
    const Block out[] = {
        {"out", (uintptr_t)d.out, soa((uintptr_t)C_out, d.out_stride), 4, true},
        {"ring", ringed ? (uintptr_t)d.ring : 0, ringed ? soa((uintptr_t)(L * C_in), d.ring_stride) : 0, 4, false},
        {"pos", (uintptr_t)d.pos, n * 4, 4, true},
        {"age", (uintptr_t)d.age, n * 4, 4, true},
    };
    if (const int32_t rc = check_blocks(E, in, std::size(in), out, std::size(out))) return rc;
    if (const int32_t rc = check_apart(E, out, std::size(out))) return rc;
    hipLaunchKernelGGL(wedm_sensor_kernel, dim3((uint32_t)((d.num_envs + WEDM_SN_BLOCK - 1) / WEDM_SN_BLOCK)), dim3(WEDM_SN_BLOCK), 0,
                       (hipStream_t)stream, d, d.chan, d.route);
    return E.launched();
}

// why a descriptor cannot be followed (wedm_derive_geometry, and wedm_draw_episode for its `geom`), or NULL
static const char* geom_derive_desc_error(const wedm_geom_derive_desc& d) {
    if (!d.combo || !d.geom_f64 || !d.geom_i32) return "null combination table or geometry block";
    if ((uintptr_t)d.geom_f64 % 8 || (uintptr_t)d.combo % 8 || (uintptr_t)d.geom_i32 % 4) return "a pointer is not aligned to its element";
    if (d.num_envs < 1) return "num_envs must be positive";
    if (d.stride < d.num_envs) return "stride smaller than num_envs";
    if (d.n_seg_max < 1 || d.n_seg_max > (1 << 29)) return "n_seg_max outside [1, 2^29]";
    if (d.n_diameters < 1 || d.n_materials < 1) return "n_diameters and n_materials must be positive";
    if (!finite_f64(d.segment_len) || !(d.segment_len > 0.0)) return "segment_len must be finite and positive";
    if (!finite_f64(d.buffer_len_bottom) || !finite_f64(d.buffer_len_top) || d.buffer_len_bottom < 0.0 || d.buffer_len_top < 0.0)
        return "buffer lengths must be finite and not negative";
    if (!finite_f64(d.contact_offset_top)) return "contact_offset_top must be finite";
    // (2^29 each: zone_start0 + floor(h / seg) <= 2^29 + n_seg_max stays inside int32 in the kernel)
    if (d.zone_start0 < 0 || d.zone_start0 > (1 << 29) || d.contact_bottom0 < 0 || d.contact_bottom0 > (1 << 29))
        return "zone_start0 or contact_bottom0 outside [0, 2^29]";
    return nullptr;
}

int32_t wedm_derive_geometry(const wedm_geom_derive_desc* desc, const double* height, const int32_t* diameter_idx,
                             const int32_t* material_idx, const uint8_t* mask, int32_t* status, void* stream) {
    const Entry E{"wedm_derive_geometry"};
    if (!desc) return E.bad("null descriptor");
    const wedm_geom_derive_desc& d = *desc;
    if (!height || !diameter_idx) return E.bad("null height or diameter index array");
    if ((uintptr_t)height % 8 || (uintptr_t)diameter_idx % 4 || (uintptr_t)material_idx % 4)
        return E.bad("a pointer is not aligned to its element");
    if (const char* why = geom_derive_desc_error(d)) return E.bad(why);
    const dim3 grid((uint32_t)(((int64_t)d.num_envs + 255) / 256));
    hipLaunchKernelGGL(wedm_derive_geometry_kernel, grid, dim3(256), 0, (hipStream_t)stream, d, height, diameter_idx,
                       material_idx, mask, status);
    return E.launched();
}

int32_t wedm_draw_episode(const wedm_draw_desc* desc, const uint8_t* mask, int32_t* draw_count, void* stream) {
    const Entry E{"wedm_draw_episode"};
    if (!desc) return E.bad("null descriptor");
    const wedm_draw_desc& d = *desc;
    if (!draw_count || (uintptr_t)draw_count % 4) return E.bad("draw_count is null or not aligned to its element");
    if (d.num_envs < 1) return E.bad("num_envs must be positive");
    if (d.stride < d.num_envs) return E.bad("stride smaller than num_envs");
    if (d.dynamic != 0 && d.dynamic != 1) return E.bad("dynamic must be 0 or 1");
    bool envp = false;
    for (int s = 0; s < WEDM_DRAW_SLOTS; ++s) {
        const wedm_draw_slot& sl = d.slot[s];
        const bool choice = s == WEDM_DS_MATERIAL || s == WEDM_DS_DIAMETER;
        const std::string name = "slot " + std::to_string(s);
        if (sl.kind == WEDM_DRAW_NONE) continue;
        if (sl.kind != (choice ? WEDM_DRAW_CHOICE : WEDM_DRAW_UNIFORM)) return E.bad(name + ": a kind this slot does not take");
        if (choice) {
            if (sl.k < 1) return E.bad(name + ": a choice needs k >= 1");
        } else {
            if (!finite_f64(sl.lo) || !finite_f64(sl.hi) || !finite_f64(sl.span)) return E.bad(name + ": bounds must be finite");
            if (sl.lo > sl.hi) return E.bad(name + ": lo > hi");
        }
        envp |= s < WEDM_DRAW_ENVP_SLOTS;
    }
    const auto misplaced = [](const void* p, size_t align) { return !p || (uintptr_t)p % align; };
    if (envp) {
        if (misplaced(d.envp_src, 8) || misplaced(d.envp_rows, 8)) return E.bad("envp_src or envp_rows is null or misaligned");
        if (!finite_f64(d.base_flow_rate) || !finite_f64(d.dt_s)) return E.bad("base_flow_rate and dt_s must be finite");
    }
    const bool has_mat = d.slot[WEDM_DS_MATERIAL].kind != WEDM_DRAW_NONE, has_h = d.slot[WEDM_DS_HEIGHT].kind != WEDM_DRAW_NONE,
               has_dia = d.slot[WEDM_DS_DIAMETER].kind != WEDM_DRAW_NONE;
    if (has_mat) {
        if (misplaced(d.material_index, 8) || misplaced(d.wmat_table, 8) || misplaced(d.wmat_rows, 8))
            return E.bad("material_index, wmat_table or wmat_rows is null or misaligned");
        if (!d.dynamic && (misplaced(d.wmat_geom_table, 8) || misplaced(d.geom_f64, 8)))
            return E.bad("wmat_geom_table or geom_f64 is null or misaligned");
    }
    if ((has_h || has_dia) && !d.dynamic) return E.bad("height and diameter are drawn with dynamic geometry only");
    if (d.dynamic && (has_mat || has_h || has_dia)) {
        const wedm_geom_derive_desc& g = d.geom;
        if (const char* why = geom_derive_desc_error(g)) return E.bad(std::string("geom: ") + why);
        if (g.num_envs != d.num_envs || g.stride != d.stride) return E.bad("geom: num_envs or stride differs from the descriptor's");
        if (misplaced(d.height, 8) || misplaced(d.diameter_index, 4)) return E.bad("height or diameter_index is null or misaligned");
        if ((uintptr_t)d.material_index % 8 || (uintptr_t)d.geom_status % 4) return E.bad("material_index or geom_status is misaligned");
        if (has_mat && d.slot[WEDM_DS_MATERIAL].k != g.n_materials) return E.bad("k of the material slot is not geom.n_materials");
        if (has_dia && d.slot[WEDM_DS_DIAMETER].k > g.n_diameters) return E.bad("k of the diameter slot exceeds geom.n_diameters");
        if (has_h) {  // the kernel's own capacity test on the largest height: cells is monotone in h, so no draw is refused
            const wedm_draw_slot& sl = d.slot[WEDM_DS_HEIGHT];
            const double cells = ((g.buffer_len_bottom + sl.hi) + g.buffer_len_top) / g.segment_len;
            if (!(sl.lo > 0.0)) return E.bad("height range must have lo > 0");
            if (!(cells < (double)g.n_seg_max + 1.0)) return E.bad("height range reaches past n_seg_max cells");
        }
    }
    const dim3 grid((uint32_t)(((int64_t)d.num_envs + 255) / 256));
    hipLaunchKernelGGL(wedm_draw_episode_kernel, grid, dim3(256), 0, (hipStream_t)stream, d, mask, draw_count);
    return E.launched();
}

int32_t wedm_debug_registry(int32_t index, int32_t* kernel, int32_t* lanes, uint32_t* forms) {
    const Slice& r = registry();
    if (index == -1) {
        if (!kernel) return WEDM_ERR_BAD_ARG;
        *kernel = (int32_t)r.size();
        return WEDM_OK;
    }
    if (index < 0 || index >= (int32_t)r.size() || !kernel || !lanes || !forms) return WEDM_ERR_BAD_ARG;
    *kernel = r[index].kernel;
    *lanes = r[index].lanes;
    *forms = r[index].forms;
    return WEDM_OK;
}

int32_t wedm_debug_last_form(wedm_ctx* ctx, int32_t* kernel, int32_t* lanes, uint32_t* forms) {
    if (!ctx || !kernel || !lanes || !forms) return WEDM_ERR_BAD_ARG;
    if (!ctx->last_plan) return fail(ctx, WEDM_ERR_BAD_ARG, "wedm_debug_last_form: no launch yet");
    *kernel = ctx->last_plan->kernel;
    *lanes = ctx->last_plan->lanes;
    *forms = ctx->last_plan->forms;
    return WEDM_OK;
}

const char* wedm_debug_form_name(int32_t bit) {
    return bit >= 0 && bit < (int32_t)(sizeof(form_bit_names) / sizeof(form_bit_names[0])) ? form_bit_names[bit] : "";
}

int32_t wedm_debug_math(int32_t kind, const double* a, const double* b, double* out, int32_t n, void* stream) {
    if (!a || !out || n <= 0 || kind < 0 || kind > 8) return WEDM_ERR_BAD_ARG;
    hipLaunchKernelGGL(wedm_debug_math_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, kind, a, b,
                       out, n);
    return hipGetLastError() == hipSuccess ? WEDM_OK : WEDM_ERR_HIP;
}

int32_t wedm_debug_poison_lds(float value, void* stream) {
    int dev = 0, lds = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return WEDM_ERR_HIP;
    (void)hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (lds <= 0 || cus <= 0) return WEDM_ERR_HIP;
    if (hipFuncSetAttribute((const void*)wedm_debug_poison_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return WEDM_ERR_HIP;
    // one block per CU holds the whole LDS; a few rounds so that every CU gets one whatever the dispatch order
    hipLaunchKernelGGL(wedm_debug_poison_lds_kernel, dim3(4 * cus), dim3(256), (size_t)lds, (hipStream_t)stream, value, lds / 4);
    return hipGetLastError() == hipSuccess ? WEDM_OK : WEDM_ERR_HIP;
}

}  // extern "C"

#endif  // WEDM_PART

