#!/usr/bin/env python
"""Phase stamps and the wave census of the register kernel wedm_step_regs from a -DWEDM_STAMPS build (diagnostic, never the
shipped library):
* cycles per wave and microsecond in prelude / walk / reduction / epilogue, for the microseconds the quiet prelude handled
  and, separately, for those that took the general path;
* the census: how the launch's waves pair up on SIMDs, when the first- and the second-arrived wave of a SIMD end (from the
  start of the kernel, on the 100 MHz clock all XCDs share), and the share of the launch during which a SIMD held one wave only;
* the candidates for the pair bit of wedm_step_regs<2, *>'s priority tie-break (the grid half, the bits of HW_ID's wave
  slot): on how many SIMDs the two waves differ in it, and on how many of those the bit is set in the later-arrived wave.
usage: WEDM_HIP_LIB=build/ablate/libwedm_STAMPS.so python tools/stamps_regs.py [lanes] [num_envs] [gap_um] [microseconds]"""
import ctypes as C
import sys
from collections import Counter, defaultdict

sys.path.insert(0, ".")
import numpy as np
import torch

from sparc_amd import WireEDMEnv, WireModuleParameters

lanes = int(sys.argv[1]) if len(sys.argv) > 1 else 2
n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
us = int(sys.argv[4]) if len(sys.argv) > 4 else 1000
env = WireEDMEnv(num_envs=n, device="cuda:0", wire_params=WireModuleParameters(segment_len=0.625))
env.set_kernel(7, lanes)
env.reset(seed=1234)
if len(sys.argv) > 3 and float(sys.argv[3]) > 0:
    env.state.wire_position = 10.0
    env.state.workpiece_position = 10.0 + float(sys.argv[3])
    env.state.target_position = 5000.0
act = env.make_action(0.1, 80.0, 5, 3.0, 80.0)
buf = torch.zeros(n * 64, dtype=torch.int64, device="cuda")
L = env._backend._L
L.wedm_debug_set_stamp_buffer.argtypes = [C.c_void_p, C.c_void_p]
L.wedm_debug_set_stamp_buffer(env._backend._ctx, C.c_void_p(buf.data_ptr()))
env.step_many(act, us)
buf.zero_()
env.step_many(act, us)
torch.cuda.synchronize()
raw = buf.cpu().numpy()
grid, block = (int(v) for v in env._backend.last_kernel().split("<<<")[1].split(">>>")[0].split(",")[:2])
wpb = block // 64
nw = grid * wpb                                              # waves of the launch
q = raw[: nw * 4].reshape(-1, 4).astype(float)               # quiet microseconds: prelude, walk, reduction, epilogue
g = raw[nw * 4: nw * 10].reshape(-1, 6).astype(float)        # general: prelude, walk, reduction + epilogue; their number; -; quiet ones
cen = raw[nw * 10: nw * 14].reshape(-1, 4)                   # census: HW_ID, XCC_ID, start, end (10 ns ticks)
keep = (g[:, 3] + g[:, 5]) > 0
q, g = q[keep], g[keep]
nq, ng = g[:, 5].sum(), g[:, 3].sum()
print(f"{env._backend.last_kernel()}: {len(q)} waves x {us} us; quiet {100 * nq / (nq + ng):.1f} % of wave-us, general {100 * ng / (nq + ng):.1f} %")
m = q.sum(axis=0) / max(nq, 1)
print(f"  quiet   wave-us: prelude {m[0]:.0f}  walk {m[1]:.0f}  reduction {m[2]:.0f}  epilogue {m[3]:.0f}  total {m.sum():.0f} cycles")
m = g[:, :3].sum(axis=0) / max(ng, 1)
print(f"  general wave-us: prelude {m[0]:.0f}  walk {m[1]:.0f}  reduction + epilogue {m[2]:.0f}  total {m.sum():.0f} cycles")
print(f"  all: {(q.sum() + g[:, :3].sum()) / (nq + ng):.0f} cycles per wave-us")

# ---- the census
if not cen[:, 3].any():
    sys.exit("  (no census rows: the library's wedm_step_regs writes none)")
hw, xcc = cen[:, 0], cen[:, 1] & 0xF
cu = (xcc << 16) | (((hw >> 13) & 7) << 8) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 0xF)
simd = (hw >> 4) & 3
t0, t1 = cen[:, 2].astype(np.float64) / 100.0, cen[:, 3].astype(np.float64) / 100.0   # us
start, span = t0.min(), t1.max() - t0.min()
blk = np.arange(nw) // wpb
on = defaultdict(list)
for i in range(nw):
    on[(int(cu[i]), int(simd[i]))].append(i)
print(f"  census: {nw} waves in blocks of {wpb} on {len(set(cu.tolist()))} CUs, {len(on)} SIMDs; launch span {span:.0f} us")
sizes = Counter(len(v) for v in on.values())
print("  waves per SIMD over the launch: " + ", ".join(f"{k}: {sizes[k]} SIMDs" for k in sorted(sizes)))
same = sum(1 for v in on.values() if len(v) == 2 and blk[v[0]] == blk[v[1]])
print(f"  SIMDs with exactly two waves: {sizes.get(2, 0)}, both of one block on {same}")
per_block = Counter()
for b in range(grid):
    per_block[tuple(sorted(Counter(simd[b * wpb:(b + 1) * wpb].tolist()).values()))] += 1
print("  waves per SIMD inside a block: " + ", ".join(f"{k}: {v} blocks" for k, v in sorted(per_block.items())))


def dist(x):
    x = np.asarray(x)
    return f"min {x.min():.0f}  p10 {np.percentile(x, 10):.0f}  median {np.median(x):.0f}  p90 {np.percentile(x, 90):.0f}  max {x.max():.0f} us"


first, second, lone, empty, both = [], [], 0.0, 0.0, 0.0
for v in on.values():
    v = sorted(v, key=lambda i: t0[i])
    first.append(t1[v[0]] - start)
    if len(v) > 1:
        second.append(t1[v[1]] - start)
    ev = sorted([(t0[i], 1) for i in v] + [(t1[i], -1) for i in v])
    cur, prev = 0, start
    for t, d in ev:
        if cur == 0:
            empty += t - prev
        elif cur == 1:
            lone += t - prev
        else:
            both += t - prev
        cur, prev = cur + d, t
    empty += start + span - prev
tot = span * len(on)
print(f"  end of wave - start of kernel, first-arrived wave of a SIMD:  {dist(first)}")
if second:
    print(f"  end of wave - start of kernel, second-arrived wave of a SIMD: {dist(second)}")
print(f"  wave lifetime: {dist(t1 - t0)}")
print(f"  share of the launch (SIMD-time over {len(on)} SIMDs): two or more waves resident {100 * both / tot:.1f} %, "
      f"one wave only {100 * lone / tot:.1f} %, none {100 * empty / tot:.1f} %")

# ---- candidates for the pair bit p of the two-lane register kernel's priority tie-break: a bit a wave can form by itself
# that differs between the two waves of a SIMD.  Per candidate: in how many of the SIMDs with exactly two waves p differs, and in how many of those
# p = 1 is the later-arrived wave.
pairs = [sorted(v, key=lambda i: t0[i]) for v in on.values() if len(v) == 2]
cands = {"grid half (blockIdx.x >= gridDim.x / 2)": (blk >= grid // 2).astype(int)}
for b in range(4):
    cands[f"HW_ID wave slot bit {b}"] = ((hw >> b) & 1).astype(int)
print(f"  pair bit candidates over {len(pairs)} SIMDs with exactly two waves:")
for name, p in cands.items():
    differ = [(a, z) for a, z in pairs if p[a] != p[z]]
    late = sum(1 for a, z in differ if p[z] == 1)
    print(f"    {name}: differs on {len(differ)}, equal on {len(pairs) - len(differ)}; p = 1 is the later-arrived wave on {late} of {len(differ)}")
slots = Counter((int(hw[a] & 0xF), int(hw[z] & 0xF)) for a, z in pairs)
print("  wave slots (first-arrived, second-arrived): " + ", ".join(f"{k}: {v}" for k, v in sorted(slots.items())))
lag = np.array([t0[z] - t0[a] for a, z in pairs]) if pairs else np.zeros(1)
print(f"  start of the second-arrived wave behind the first: {dist(lag)}")
