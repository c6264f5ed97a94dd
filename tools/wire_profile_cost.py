#!/usr/bin/env python
"""Cost of the wire profile (`WireEDMEnv.wire_profile`: wedm_wire_profile) at three shapes:
65 536 x 128 (BASELINE configs[2]), 32 768 x 400 (the per-GPU shard of configs[3]) and a 16 384-environment shard with
per-environment geometry as in configs[4] (bench.config5_draws), each at 8 bins, in alternating rounds:

  launch   the launch alone, descriptor prebuilt (back to back the host keeps ahead of it: the kernel's own time);
  method   `env.wire_profile(8)`, the Python method included;
  torch    the same outputs as a stock-torch expression written in this tool (uniform shapes only: it reshapes the
           quad-interleaved block to [env, cell] and reduces with float64 sums, temporaries and all);
  clone    `T.clone()` of the same block, the bandwidth yardstick: it moves twice the bytes the profile reads;
  step / step_profile   `WireEDMVectorEnv.step` (autoreset and reward in the kernel) without and with `wire_profile_bins=8`.

    python tools/wire_profile_cost.py [--rounds 5] [--repeats 20] [--shapes headline,long,per_env] [--out FILE]

Prints (and with --out appends) one JSON line per shape: medians of the rounds in microseconds per call by device events,
the bytes of T the launch reads over its time against the HBM line bench.py prices with, and `launch_within_clone`: the
acceptance of section 4.12 at the two uniform shapes (the launch takes no longer than the clone in the same run)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

BINS = 8


def build(shape, dev):
    import numpy as np

    import bench
    from sparc_amd import WireEDMEnv, WireModuleParameters

    kw = dict(autoreset=True, reward="progress", device=dev)
    if shape == "headline":
        return WireEDMEnv(num_envs=65536, wire_params=WireModuleParameters(segment_len=0.625), **kw)
    if shape == "long":
        return WireEDMEnv(num_envs=32768, **kw)
    h, d, _ = bench.config5_draws(16384, 0, 16384)
    return WireEDMEnv(num_envs=16384, workpiece_height=np.asarray(h), wire_diameter=np.asarray(d), **kw)


def torch_profile(T, n_envs, n_seg, lo, hi, bins):
    """The profile's rows with stock torch, uniform geometry: what a user would write against the block today."""
    import torch

    cells = T[:, :n_envs].permute(1, 0, 2).reshape(n_envs, -1)[:, :n_seg]
    c64 = cells.to(torch.float64)
    zone = c64[:, lo:hi] if 0 <= lo < hi <= n_seg else c64
    top, hot = cells.max(dim=1)
    rows = [(zone.sum(dim=1) / zone.shape[1]).to(torch.float32), (c64.sum(dim=1) / n_seg).to(torch.float32), top,
            hot.to(torch.float32)]
    edges = [(b * n_seg // bins, max(b * n_seg // bins + 1, (b + 1) * n_seg // bins)) for b in range(bins)]
    rows += [cells[:, a:b].amax(dim=1) for a, b in edges]
    rows += [(c64[:, a:b].sum(dim=1) / (b - a)).to(torch.float32) for a, b in edges]
    return torch.stack(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--shapes", default="headline,long,per_env")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import bench
    from sparc_amd import WireEDMVectorEnv, _abi, _lib

    dev = "cuda:0"
    for shape in args.shapes.split(","):
        env = build(shape, dev)
        n, st = env.num_envs, env.state
        vec, vec_p = WireEDMVectorEnv(env), WireEDMVectorEnv(env, wire_profile_bins=BINS)
        vec.reset(seed=1234)
        action = env.make_action(0.1, 80.0, 5, 3.0, 80.0)
        vec.step(action)
        g = env.geometry
        out = torch.zeros((_abi.profile_rows(BINS), st.stride), dtype=torch.float32, device=dev)
        desc = _abi.ProfileDesc(
            T=st.T.data_ptr(), stride=st.stride, num_envs=n, n_seg_max=env.n_segments, n_seg=g.n_seg if g else 0,
            az_start=g.az_start if g else 0, az_end=g.az_end if g else 0, geom_i32=None if g else env._geom_i32.data_ptr(),
            bins=BINS, out=out.data_ptr(), out_stride=st.stride, out_cols=n)
        status = env._profile_status.data_ptr()
        ops = {"launch": lambda: env._backend.wire_profile(desc, None, n, status),
               "method": lambda: env.wire_profile(BINS),
               "clone": lambda: st.T.clone(),
               "step": lambda: vec.step(action),
               "step_profile": lambda: vec_p.step(action)}
        if g is not None:
            ops["torch"] = lambda: torch_profile(st.T, n, g.n_seg, g.az_start, g.az_end, BINS)
            torch.cuda.synchronize()
            agree = bool(torch.equal(ops["torch"]().view(torch.int32), env.wire_profile(BINS)["rows"].view(torch.int32)))
        else:
            agree = None
        for op in ops.values():   # warm-up: code objects loaded, the allocator holds the temporaries
            op()
        torch.cuda.synchronize()
        times = {name: [] for name in ops}
        for _ in range(args.rounds):
            for name, op in ops.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.repeats):
                    op()
                t1.record()
                t1.synchronize()
                times[name].append(t0.elapsed_time(t1) * 1e3 / args.repeats)
        env.check_errors()
        med = {name: statistics.median(v) for name, v in times.items()}
        read = st.T.shape[0] * n * 16
        gbs = read / (med["launch"] * 1e-6) / 1e9
        line = json.dumps({
            "shape": shape, "num_envs": n, "n_segments": env.n_segments, "per_env_geometry": g is None, "bins": BINS,
            "build_id": _lib.build_id(), "rounds": args.rounds, "repeats": args.repeats,
            **{f"{name}_us": v for name, v in med.items()},
            "step_profile_minus_step_us": med["step_profile"] - med["step"],
            "method_host_share": 1.0 - med["launch"] / med["method"],
            "launch_within_clone": med["launch"] <= med["clone"], "torch_agrees_bit_for_bit": agree,
            "bytes_read": read, "launch_GBs": gbs, "frac_of_hbm_peak": gbs / bench.HBM_PEAK_GBS,
            "hbm_peak_GBs": bench.HBM_PEAK_GBS, "rounds_us": times})
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        env.close()
        del env, vec, vec_p, ops, out, st
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
