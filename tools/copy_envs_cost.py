#!/usr/bin/env python
"""Cost of moving environments on the device (`WireEDMEnv.fork`, `snapshot`, `restore`: wedm_copy_columns, DESIGN.md
section 4.11) at BASELINE configs[2]'s shape, 65 536 environments x 128 segments, against the same copies written in stock
torch inside this tool (an `index_select` and an `index_copy_` per block: a temporary the size of the copied columns for
every block), in alternating rounds.

  fork:             64 sources broadcast over the other 65 472 slots (shooting: K states into K x M candidates);
  snapshot_restore: a snapshot of every environment followed by its restore.

    python tools/copy_envs_cost.py [--rounds 5] [--repeats 20] [--num-envs 65536]

Prints one JSON line per operation: the medians of the rounds in microseconds per operation, end to end (calls back to
back, so the slower of host and device), for the fork also its launch alone with prebuilt planes (`launch_only_us`: the
kernel's own time), the bytes moved (read + written) and bytes over time -- the launch alone where it was measured -- as a
fraction of the HBM line bench.py prices with (`HBM_PEAK_GBS`)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--num-envs", type=int, default=65536)
    args = ap.parse_args()

    import torch

    import bench
    from sparc_amd import WireEDMEnv, WireModuleParameters, _lib
    from sparc_amd.snapshot import _plane, env_blocks

    n, dev = args.num_envs, "cuda:0"
    env = WireEDMEnv(num_envs=n, device=dev, wire_params=WireModuleParameters(segment_len=0.625))
    env.reset(seed=1234)
    env.step_many(env.make_action(0.1, 80.0, 5, 3.0, 80.0), 1000)
    blocks = env_blocks(env)
    per_env = sum(t.shape[0] * t.element_size() * (4 if t.dim() == 3 else 1) for t in blocks.values())   # bytes of one column

    k = 64
    src = (torch.arange(n - k, device=dev) % k).to(torch.int32)
    dst = torch.arange(k, n, device=dev, dtype=torch.int32)
    src64, dst64, every = src.long(), dst.long(), torch.arange(n, device=dev)

    def torch_fork():
        for t in blocks.values():
            t.index_copy_(1, dst64, t.index_select(1, src64))

    held = {}

    def torch_snapshot_restore():
        for name, t in blocks.items():
            held[name] = t.index_select(1, every)
        for name, t in blocks.items():
            t.index_copy_(1, every, held[name])

    def kernel_snapshot_restore():
        env.restore(env.snapshot(every))

    # the fork's launch alone, planes prebuilt: back to back the host keeps ahead of it, so this is the kernel's own time
    # (the method around it also converts and checks the device indices with a dozen small torch ops per list)
    planes = [_plane(t, t, n, n) for t in blocks.values()]

    def launch_only():
        env._backend.copy_columns(planes, src.data_ptr(), dst.data_ptr(), n - k, env._copy_status.data_ptr())

    ops = {"fork": {"kernel": lambda: env.fork(src, dst), "torch": torch_fork, "launch": launch_only,
                    "bytes": 2 * (n - k) * per_env},
           "snapshot_restore": {"kernel": kernel_snapshot_restore, "torch": torch_snapshot_restore, "bytes": 4 * n * per_env}}
    for name, op in ops.items():
        sides = [side for side in ("kernel", "torch", "launch") if side in op]
        for side in sides:   # warm-up: code objects loaded, the allocator holds the temporaries
            op[side]()
        torch.cuda.synchronize()
        times = {side: [] for side in sides}
        for _ in range(args.rounds):
            for side in sides:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.repeats):
                    op[side]()
                t1.record()
                t1.synchronize()
                times[side].append(t0.elapsed_time(t1) * 1e3 / args.repeats)
        med = {side: statistics.median(v) for side, v in times.items()}
        gbs = op["bytes"] / (med.get("launch", med["kernel"]) * 1e-6) / 1e9
        print(json.dumps({"operation": name, "shape": f"{n} x 128", "build_id": _lib.build_id(), "planes": len(blocks),
                          "bytes_per_env_one_way": per_env, "bytes_moved": op["bytes"], "kernel_us": med["kernel"],
                          "torch_us": med["torch"], "torch_over_kernel": med["torch"] / med["kernel"], "launch_only_us": med.get("launch"),
                          "kernel_GBs": gbs,
                          "frac_of_hbm_peak": gbs / bench.HBM_PEAK_GBS, "hbm_peak_GBs": bench.HBM_PEAK_GBS,
                          "rounds_us": times}), flush=True)
    env.check_errors()


if __name__ == "__main__":
    main()
