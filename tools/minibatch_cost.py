#!/usr/bin/env python
"""Cost of dealing a rollout's rows into minibatches as `wedm_minibatch_index` against what torch offers for it, in the same
process and build, in alternating rounds, timed with event pairs, medians.

  call          one call over R rows (98 % of them live) into n = 8 parts, at R = 280, 65 536, 2^20 and 2^23 (the
                128 x 65 536 rollout): all three phases in one call;
  count, offsets, scatter   each phase in a call of its own, over the workspace the phases before it left: which of them the
                call's time is made of (their sum exceeds the call's by what back-to-back launches overlap);
  all_live      the call with a NULL ``valid`` (every row live: no row's position is known without a walk);
  randperm      ``torch.tensor_split(torch.randperm(R, device=...), n)``: what `RolloutBuffer.minibatches` does without a
                sampler;
  host_randperm ``torch.randperm(R, generator=<a CPU generator>).to(device)`` and the split: what the parity and resume
                stacks of the tests do to have a permutation with defined bits.  Host work: the second event waits for it.

    python tools/minibatch_cost.py [--rounds 7] [--out profiles/r19/minibatch_cost.jsonl]

Prints one JSON line per size (every sample in it) and writes them to ``--out``."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SIZES = (280, 65536, 1 << 20, 1 << 23)
PARTS = 8


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r19" / "minibatch_cost.jsonl"))
    args = ap.parse_args()

    import torch

    from sparc_amd import _abi, _lib

    assert torch.cuda.is_available(), "the cost is a measurement on the MI355X"
    dev = torch.device("cuda:0")
    L = _lib.load()
    gen = torch.Generator(device=dev).manual_seed(99)
    host_gen = torch.Generator().manual_seed(99)
    lines = []
    for R in SIZES:
        tiles = -(-R // _abi.MB_TILE)
        valid = (torch.rand(R, generator=gen, device=dev) >= 0.02).to(torch.uint8)
        index = torch.zeros(R, dtype=torch.int64, device=dev)
        count = torch.zeros(2, dtype=torch.int64, device=dev)
        tile_counts = torch.zeros(tiles, dtype=torch.int32, device=dev)
        tile_base = torch.zeros(tiles, dtype=torch.int32, device=dev)
        draws = [0]

        def ours(flags, with_valid=True):
            def fn():
                draws[0] += 1
                d = _abi.MbDesc(valid=valid.data_ptr() if with_valid else None, index=index.data_ptr(), count=count.data_ptr(),
                                tile_counts=tile_counts.data_ptr(), tile_base=tile_base.data_ptr(), seed=7, draw=draws[0], rows=R,
                                n_parts=PARTS, flags=flags)
                _lib.call_stateless(L.wedm_minibatch_index, dev, C.byref(d))
            return fn

        work = {"call": ours(0), "count": ours(_abi.MB_COUNT), "offsets": ours(_abi.MB_OFFSETS), "scatter": ours(_abi.MB_SCATTER),
                "all_live": ours(0, with_valid=False),
                "randperm": lambda: torch.tensor_split(torch.randperm(R, device=dev, generator=gen), PARTS),
                "host_randperm": lambda: torch.tensor_split(torch.randperm(R, generator=host_gen).to(dev), PARTS)}
        reps = {k: 300 if R <= 1 << 20 else 50 for k in work}
        reps["host_randperm"] = 30 if R <= 1 << 20 else 3
        for fn in work.values():   # warm-up: code loaded, the allocator's blocks made
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in work}
        for _ in range(args.rounds):
            for k, fn in work.items():   # (the phases alone follow "call": the workspace they run over is this valid block's)
                ms[k].append(timed(fn, reps[k]))
        line = {"workload": "minibatch_index", "rows": R, "n_parts": PARTS, "live": int(valid.sum()), "build_id": _lib.build_id(),
                **{f"{k}_us": 1e3 * statistics.median(v) for k, v in ms.items()}, "ms": ms}
        lines.append(line)
        print(json.dumps(line), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("".join(json.dumps(line) + "\n" for line in lines))


if __name__ == "__main__":
    main()
