#!/usr/bin/env python
"""Phase stamps of the register kernel wedm_step_regs from a -DWEDM_STAMPS build (diagnostic, never the shipped library):
cycles per wave and microsecond in prelude / walk / reduction / epilogue, for the microseconds the quiet prelude handled
and, separately, for those that took the general path.
usage: WEDM_HIP_LIB=build/ablate/libwedm_STAMPS.so python tools/stamps_regs.py [lanes] [num_envs] [gap_um] [microseconds]"""
import ctypes as C
import sys

sys.path.insert(0, ".")
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
nblk = int(env._backend.last_kernel().split("<<<")[1].split(",")[0])
q = raw[: nblk * 16].reshape(-1, 4).astype(float)              # quiet microseconds: prelude, walk, reduction, epilogue
g = raw[nblk * 16: nblk * 16 + nblk * 24].reshape(-1, 6).astype(float)   # general: prelude, walk, reduction + epilogue; their number; -; quiet ones
keep = (g[:, 3] + g[:, 5]) > 0
q, g = q[keep], g[keep]
nq, ng = g[:, 5].sum(), g[:, 3].sum()
print(f"{env._backend.last_kernel()}: {len(q)} waves x {us} us; quiet {100 * nq / (nq + ng):.1f} % of wave-us, general {100 * ng / (nq + ng):.1f} %")
m = q.sum(axis=0) / max(nq, 1)
print(f"  quiet   wave-us: prelude {m[0]:.0f}  walk {m[1]:.0f}  reduction {m[2]:.0f}  epilogue {m[3]:.0f}  total {m.sum():.0f} cycles")
m = g[:, :3].sum(axis=0) / max(ng, 1)
print(f"  general wave-us: prelude {m[0]:.0f}  walk {m[1]:.0f}  reduction + epilogue {m[2]:.0f}  total {m.sum():.0f} cycles")
print(f"  all: {(q.sum() + g[:, :3].sum()) / (nq + ng):.0f} cycles per wave-us")
