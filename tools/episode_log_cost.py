#!/usr/bin/env python
"""Cost of the episode log as one call (wedm_episode_log) against the sync-free torch composition it replaces, in the same
process and build, in alternating rounds, timed with event pairs, medians.  65 536 environments, a ring of 65 536, the planes
of a stack that has every optional block (per-environment parameters, materials, dynamic geometry, pulse and signal
statistics, an episode sampler, a normaliser, ``params=True``: taken from such a stack's `EpisodeLog`, built small):

  a  the call, with 0 %, 1 % and 100 % of the environments finishing;
  b  the torch composition on the same blocks: cumsum, ``where``, a scatter with a dump slot per column, the accumulator
     updates, ``head``;
  c  `WireEDMVectorEnv.step` at 65 536 x 128 segments (the headline batch, resets inside the kernel) with and without an
     `EpisodeLog`, alternating.

Before timing, a and b are asserted to write the same ring.

    python tools/episode_log_cost.py [--rounds 5] [--out profiles/r4/episode_log_cost.jsonl] [--only-call SHARE]

``--only-call SHARE`` runs nothing but 50 calls of a at that share (for a kernel trace taken as a run of its own).
Prints one JSON line per workload (every sample in it) and writes them to ``--out``."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def timed(fn, count):
    import torch

    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(count):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / count  # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r4" / "episode_log_cost.jsonl"))
    ap.add_argument("--only-call", type=float, default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from sparc_amd import EpisodeLog, WireEDMEnv, WireEDMVectorEnv, WireModuleParameters, _lib
    from sparc_amd.episode_log import LAST, SUM_I32, device_episode_log
    from tests._episode_log_common import Problem, full_stack

    dev, N, CAP = "cuda:0", 65536, 65536
    small, small_log, _ = full_stack(dev, 16, n=70)
    np_of = {torch.uint8: np.uint8, torch.int8: np.int8, torch.int32: np.int32, torch.int64: np.int64, torch.float32: np.float32,
             torch.float64: np.float64}
    spec = tuple((p.kind, np_of[p.dtype], len(p.names)) for p in small_log._planes)
    columns = small_log.columns
    small.close()
    rng = np.random.default_rng(1)
    p = Problem(rng, N, CAP, spec=spec, masked=True)
    buf = torch.from_numpy(p.buf).to(dev)
    base = buf.data_ptr()

    def view(name):
        off, dt, shape = p.layout[name]
        t = buf[off: off + int(np.prod(shape)) * dt.itemsize].view(getattr(torch, np.dtype(dt).name))
        return t.view(*shape)

    shares = {"0": 0.0, "1": 0.01, "100": 1.0}
    term = {k: torch.from_numpy((rng.random(N) < s).astype(np.uint8)).to(dev) for k, s in shares.items()}
    desc = p.desc(base, stamp=1)

    def call(share):
        desc.terminated = term[share].data_ptr()
        device_episode_log(desc, dev)

    if args.only_call is not None:
        key = {0.0: "0", 0.01: "1", 1.0: "100"}[args.only_call]
        for _ in range(50):
            call(key)
        torch.cuda.synchronize()
        return

    # ---- b: the composition in torch on blocks of its own (a dump slot behind every ring row)
    planes = []
    for i, (kind, dt, rows) in enumerate(spec):
        src = view(f"src{i}")
        dst = torch.zeros((rows, CAP + 1), dtype=src.dtype if kind == LAST else (torch.int64 if kind == SUM_I32 else torch.float64), device=dev)
        acc = None if kind == LAST else torch.zeros((rows, N), dtype=dst.dtype, device=dev)
        planes.append((kind, src, dst, acc))
    env_out, stamp_out = torch.zeros(CAP + 1, dtype=torch.int64, device=dev), torch.zeros(CAP + 1, dtype=torch.int64, device=dev)
    head = torch.zeros(2, dtype=torch.int64, device=dev)
    ids = torch.arange(N, dtype=torch.int64, device=dev)
    mask, trunc = view("mask") != 0, view("truncated")
    stamp = torch.ones(N, dtype=torch.int64, device=dev)

    def composition(share):
        fin = ((term[share] | trunc) != 0) & mask
        f = fin.to(torch.int64)
        k = torch.cumsum(f, 0) - f
        n = f.sum()
        write = fin & (k >= n - CAP)
        slot = torch.where(write, (head[0] + k) % CAP, CAP)
        for kind, src, dst, acc in planes:
            rows = src.shape[0]
            at = slot.unsqueeze(0).expand(rows, N)
            if kind == LAST:
                dst.scatter_(1, at, src[:, :N])
            else:
                acc.add_(torch.where(mask, src[:, :N].to(acc.dtype), 0))
                dst.scatter_(1, at, acc)
                acc.masked_fill_(fin, 0)
        env_out.scatter_(0, slot, ids)
        stamp_out.scatter_(0, slot, stamp)
        head[0] += n
        head[1] = n

    # the two write the same ring: from empty accumulators and head 0, one call each at 1 %
    for i, (kind, _, _) in enumerate(spec):
        if kind != LAST:
            view(f"acc{i}").zero_()
    view("head").zero_()
    call("1")
    composition("1")
    torch.cuda.synchronize()
    n = int(head[1])
    assert n == int(view("head")[1]) > 0
    for i, (kind, src, dst, acc) in enumerate(planes):
        assert torch.equal(dst[:, :n].contiguous().view(torch.uint8), view(f"dst{i}")[:, :n].contiguous().view(torch.uint8)), i
    assert torch.equal(env_out[:n], view("env_out")[:n])

    work = {f"a_{k}": (lambda k=k: call(k)) for k in shares}
    work.update({f"b_{k}": (lambda k=k: composition(k)) for k in shares})
    for fn in work.values():
        for _ in range(3):
            fn()
    ms = {k: [] for k in work}
    for _ in range(args.rounds):
        for k, fn in work.items():
            ms[k].append(timed(fn, 50))
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines = [{"workload": "call", "num_envs": N, "capacity": CAP, "planes": len(spec), "rows": sum(s[2] for s in spec),
              "columns": len(columns), **{f"{k}_ms": v for k, v in med.items()},
              **{f"b_over_a_{k}": med[f"b_{k}"] / med[f"a_{k}"] for k in shares}, "build_id": _lib.build_id(), "ms": ms}]
    print(json.dumps(lines[-1]), flush=True)
    del planes, buf

    # ---- c: the adapter's step with and without the log
    wire = WireModuleParameters(segment_len=0.625)
    vecs = {}
    for name in ("without", "with"):
        env = WireEDMEnv(num_envs=N, device=dev, wire_params=wire, autoreset=True, reward="progress")
        vec = WireEDMVectorEnv(env, max_episode_steps=3000, episode_log=EpisodeLog() if name == "with" else None)
        vec.reset(seed=1)
        act = env.make_action(0.1, 80.0, 5, 3.0, 80.0)
        for _ in range(3):
            vec.step(act)
        vecs[name] = (vec, act)
    torch.cuda.synchronize()
    step = {k: [] for k in vecs}
    for _ in range(args.rounds):
        for k, (vec, act) in vecs.items():
            step[k].append(timed(lambda: vec.step(act), 6))
    med = {k: statistics.median(v) for k, v in step.items()}
    records = vecs["with"][0].episode_log.read()
    lines.append({"workload": "step", "num_envs": N, "segments": 128, "without_ms": med["without"], "with_ms": med["with"],
                  "added_ms": med["with"] - med["without"], "spread_without_ms": max(step["without"]) - min(step["without"]),
                  "episodes_logged": int(len(records["env"])) + int(records["lost"]), "build_id": _lib.build_id(), "ms": step})
    print(json.dumps(lines[-1]), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("".join(json.dumps(line) + "\n" for line in lines))


if __name__ == "__main__":
    main()
