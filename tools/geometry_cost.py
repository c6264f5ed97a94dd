#!/usr/bin/env python
"""Cost of resampling geometry (wedm_derive_geometry, WireEDMEnv(dynamic_geometry=...)) on BASELINE configs[4] as rank 5 of 8
sees it: 16 384 environments, per-environment workpiece height / wire diameter / current mode, fused launches of 1000 us.

  set_geometry: a new height and diameter for EVERY environment --
      device:   `env.set_geometry(h, di, reset=False)` with device tensors (the merge, the refusals, one launch), wall clock
                from the call to the device having finished, and the launch alone by device events;
      host:     what the parent commit offers for the same change: `derive.geometry_rows` on the host plus the upload of the
                two blocks, wall clock to the same point.
  vector_step:  `WireEDMVectorEnv.step` with `uniform_geometry_sampler` against the same environment without a sampler
                (in-kernel autoreset, progress reward), device events around `--steps` steps.

Alternating rounds, medians.  One JSON line per figure, printed and written to --out.

    python tools/geometry_cost.py [--rounds 5] [--calls 20] [--steps 10] [--out profiles/r4/geometry_cost.jsonl]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r4" / "geometry_cost.jsonl"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    from sparc_amd import EnvironmentConfig, WireEDMEnv, WireEDMVectorEnv, uniform_geometry_sampler
    from sparc_amd.core import derive

    dev = "cuda:0"
    n, rank, world = 16384, 5, 8
    h, d, mode = bench.config5_draws(world * n, rank * n, (rank + 1) * n)
    dias = (0.10, 0.15, 0.20, 0.25, 0.30)
    dyn = {"max_workpiece_height": 30.0, "wire_diameters": dias}

    def make(**kw):
        env = WireEDMEnv(num_envs=n, device=dev, workpiece_height=h, wire_diameter=d, env_id_offset=rank * n,
                         dynamic_geometry=dyn, **kw)
        env.reset(seed=1234)
        return env

    lines = []
    # ---- one set_geometry of every environment
    env = make(config=EnvironmentConfig(target_cutting_distance=5000.0))
    rng = np.random.default_rng(7)
    h2, di2 = rng.uniform(10.0, 30.0, n), rng.integers(0, len(dias), n)
    d2 = np.asarray(dias)[di2]
    h_dev, di_dev = torch.from_numpy(h2).to(dev), torch.from_numpy(di2).to(dev)
    stride = env._geom_f64.shape[1]

    def device_way():
        env.set_geometry(h_dev, di_dev, reset=False)

    def launch_alone():
        dy = env._dyn
        env._backend.derive_geometry(dy.desc, dy.height.data_ptr(), dy.dia.data_ptr(), None, None, dy.status.data_ptr())

    def host_way():
        gf, gi, _ = derive.geometry_rows(h2, d2, env.wire_params, env.wire_material, env.material_params, stride)
        env._geom_f64.copy_(torch.from_numpy(gf))
        env._geom_i32.copy_(torch.from_numpy(gi))

    def wall(fn, calls):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / calls * 1e6

    def events(fn, calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / calls * 1e3

    device_way()  # warm-up, and the rows the device derived against the host's
    same = bool(torch.equal(env._geom_f64[:, :n].cpu(), torch.from_numpy(
        derive.geometry_rows(h2, d2, env.wire_params, env.wire_material, env.material_params, stride)[0][:, :n])))
    launch_alone(), host_way()
    us = {"device": [], "launch": [], "host": []}
    for _ in range(args.rounds):
        us["device"].append(wall(device_way, args.calls))
        us["launch"].append(events(launch_alone, args.calls))
        us["host"].append(wall(host_way, 1))
    env.check_errors()
    med = {k: statistics.median(v) for k, v in us.items()}
    lines.append({"figure": "set_geometry", "workload": "configs4_rank5of8", "num_envs": n, "n_seg_max": env.n_segments,
                  "set_geometry_device_us": med["device"], "launch_alone_us": med["launch"],
                  "host_geometry_rows_plus_upload_us": med["host"], "host_over_device": med["host"] / med["device"],
                  "rows_bit_equal_to_host": same, "build_id": env._backend.build_id(), "us": us})
    del env
    # ---- the vector adapter's step with and without a geometry sampler
    vecs = {}
    for key in ("plain", "sampler"):
        e = make(autoreset=True, reward="progress", config=EnvironmentConfig(target_cutting_distance=5000.0))
        gen = torch.Generator(device=dev).manual_seed(11)
        sampler = uniform_geometry_sampler(height=(10.0, 30.0), generator=gen) if key == "sampler" else None
        v = WireEDMVectorEnv(e, geometry_sampler=sampler)
        e.reset(seed=1234)  # (not v.reset: both sides keep the constructor's geometry, so they follow the same trajectories)
        vecs[key] = (v, e.make_action(0.1, 80.0, mode, 3.0, 80.0))
    for v, act in vecs.values():
        for _ in range(3):
            v.step(act)
    us = {k: [] for k in vecs}
    for _ in range(args.rounds):
        for k, (v, act) in vecs.items():
            us[k].append(events(lambda: v.step(act), args.steps))
    med = {k: statistics.median(x) for k, x in us.items()}
    lines.append({"figure": "vector_step", "workload": "configs4_rank5of8", "num_envs": n,
                  "step_plain_us": med["plain"], "step_with_geometry_sampler_us": med["sampler"],
                  "added_us": med["sampler"] - med["plain"], "ratio": med["sampler"] / med["plain"],
                  "kernels": {k: v.env._backend.last_kernel() for k, (v, _) in vecs.items()},
                  "build_id": vecs["plain"][0].env._backend.build_id(), "us": us})
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("w") as f:
        for line in lines:
            text = json.dumps(line)
            print(text)
            f.write(text + "\n")


if __name__ == "__main__":
    main()
