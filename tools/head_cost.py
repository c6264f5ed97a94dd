#!/usr/bin/env python
"""Cost of the policy action head (wedm_policy_head through `PolicyHead`) against the same distribution composed from
``torch.distributions`` in float32 (Normal -> TanhTransform -> AffineTransform, and Categorical) -- what a user writes without
the call -- in alternating rounds, timed with event pairs, medians:

  sample:  65 536 rows (the headline batch): the action, its log-probability and the entropy; the torch side also casts
           the leaves to float64 and picks the mode numbers, as a `DeviceAction` needs them;
  update:  128 x 65 536 rows in 8 minibatches of 1 048 576: `evaluate` at the stored actions, a PPO-shaped loss and
           ``backward()`` into the parameter rows -- one epoch over the rollout.

Also times EVALUATE and BACKWARD by themselves on one minibatch at M = 1, 9 and 19 modes.  The bytes per second are the
algorithmic bytes -- 4 P + 20 read and 8 written per row by EVALUATE, 4 P + 28 read and 4 P written by BACKWARD -- over
the median time; how far they stay below what a copy reaches says whether the memory or the float64 arithmetic bounds it.

    python tools/head_cost.py [--rounds 5] [--out profiles/r4/head_cost.jsonl]

Prints one JSON line per workload and writes them to ``--out``."""
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


class TorchHead:
    """The head as a float32 ``torch.distributions`` composition on stored pre-squash values."""

    def __init__(self, head):
        import torch

        dev = head.device
        lo, hi = torch.tensor(head._lo, device=dev), torch.tensor(head._hi, device=dev)
        self.loc, self.scale = ((lo + hi) / 2).float(), ((hi - lo) / 2).float()
        self.modes = torch.tensor(head.modes, dtype=torch.int32, device=dev)

    def dists(self, params):
        from torch.distributions import Categorical, Normal, TransformedDistribution
        from torch.distributions.transforms import AffineTransform, TanhTransform

        base = Normal(params[:, 0:4], params[:, 4:8].exp())
        tanh, affine = TanhTransform(cache_size=1), AffineTransform(self.loc, self.scale, cache_size=1)
        return base, tanh, affine, TransformedDistribution(base, [tanh, affine]), Categorical(logits=params[:, 8:])

    def sample(self, params):
        import torch

        base, tanh, affine, squashed, cat = self.dists(params)
        u = base.sample()
        y = affine(tanh(u))
        k = cat.sample()
        log_prob = squashed.log_prob(y).sum(1) + cat.log_prob(k)
        entropy = base.entropy().sum(1) + cat.entropy()
        leaves = [y[:, i].double().contiguous() for i in range(4)]
        return leaves, self.modes[k], u, k.to(torch.int32), log_prob, entropy

    def evaluate(self, params, u, k):
        base, tanh, affine, squashed, cat = self.dists(params)
        y = affine(tanh(u))
        return squashed.log_prob(y).sum(1) + cat.log_prob(k), base.entropy().sum(1) + cat.entropy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r4" / "head_cost.jsonl"))
    args = ap.parse_args()

    import torch

    from sparc_amd import PolicyHead, WireEDMEnv, _lib
    from sparc_amd.policy_head import BACKWARD, EVALUATE

    dev, N, T, parts = "cuda:0", 65536, 128, 8
    env = WireEDMEnv(num_envs=N, device=dev)
    head = PolicyHead(env, seed=1)
    ref = TorchHead(head)
    P, M = head.param_dim, len(head.modes)
    gen = torch.Generator(device=dev).manual_seed(1234)

    def rows(n, P=P):
        p = torch.randn(n, P, generator=gen, device=dev)
        p[:, 4:8] = p[:, 4:8].clamp(-2.0, 1.0) - 1.0
        return p

    lines = []
    # ---- sample
    params = rows(N)
    head.sample(params)
    ref.sample(params)
    torch.cuda.synchronize()
    ms = {"device": [], "torch": []}
    for _ in range(args.rounds):
        ms["device"].append(timed(lambda: head.sample(params), 2000))
        ms["torch"].append(timed(lambda: ref.sample(params), 100))
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines.append({"workload": "sample", "rows": N, "modes": M, "device_ms": med["device"], "torch_f32_ms": med["torch"],
                  "torch_over_device": med["torch"] / med["device"], "build_id": _lib.build_id(), "ms": ms})
    print(json.dumps(lines[-1]), flush=True)

    # ---- one epoch of the update over a rollout, in minibatches
    B = T * N // parts
    batches = []
    for _ in range(parts):
        p = rows(B)
        u = (p[:, 0:4] + p[:, 4:8].exp() * torch.randn(B, 4, generator=gen, device=dev)).contiguous()
        k = torch.randint(0, M, (B,), generator=gen, device=dev)
        batches.append((p.requires_grad_(True), u, k.to(torch.int32), k, torch.randn(B, generator=gen, device=dev)))

    def epoch(evaluate, index):
        for p, u, k32, k64, adv in batches:
            p.grad = None
            lp, ent = evaluate(p, u, (k32, k64)[index])
            (-(lp * adv).mean() - 0.01 * ent.mean()).backward()

    device_epoch = lambda: epoch(head.evaluate, 0)   # noqa: E731
    torch_epoch = lambda: epoch(ref.evaluate, 1)     # noqa: E731
    device_epoch()
    got = batches[0][0].grad.clone()
    torch_epoch()
    torch.cuda.synchronize()
    want = batches[0][0].grad
    worst = float(((got - want).abs() / (1e-6 + want.abs().max())).max())   # agreement of what the two sides compute
    assert worst < 1e-3, worst
    ms = {"device": [], "torch": []}
    for _ in range(args.rounds):
        ms["device"].append(timed(device_epoch, 50))
        ms["torch"].append(timed(torch_epoch, 10))
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines.append({"workload": "update", "rows": T * N, "minibatches": parts, "modes": M, "device_ms": med["device"],
                  "torch_f32_ms": med["torch"], "torch_over_device": med["torch"] / med["device"],
                  "largest_gradient_difference_relative_to_the_largest_gradient": worst, "build_id": _lib.build_id(), "ms": ms})
    print(json.dumps(lines[-1]), flush=True)
    del batches, got, want

    # ---- the two launches of the update by themselves, by the number of modes
    for m in (1, 9, 19):
        p_dim = 8 + m
        p = rows(B, p_dim)
        u = (p[:, 0:4] + p[:, 4:8].exp() * torch.randn(B, 4, generator=gen, device=dev)).contiguous()
        k = torch.randint(0, m, (B,), generator=gen, device=dev, dtype=torch.int32)
        g = torch.randn(2, B, generator=gen, device=dev)
        lp, ent, grad = torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, p_dim, device=dev)
        d = head._desc(EVALUATE, B)   # (the descriptor takes any mode numbers and count; `PolicyHead` only crater modes)
        d.n_modes, d.param_stride, d.grad_stride = m, p_dim, p_dim
        d.modes[:m] = list(range(1, m + 1))
        d.params, d.u, d.mode_index, d.log_prob, d.entropy = p.data_ptr(), u.data_ptr(), k.data_ptr(), lp.data_ptr(), ent.data_ptr()
        d.g_log_prob, d.g_entropy, d.grad_params = g[0].data_ptr(), g[1].data_ptr(), grad.data_ptr()
        phases = {}
        for name, op in (("evaluate", EVALUATE), ("backward", BACKWARD)):
            d.op = op
            env._backend.policy_head(d)
            phases[name] = [timed(lambda: env._backend.policy_head(d), 500) for _ in range(args.rounds)]
        ev, bw = (statistics.median(phases[name]) for name in ("evaluate", "backward"))
        ev_bytes, bw_bytes = B * (4 * p_dim + 20 + 8), B * (4 * p_dim + 28 + 4 * p_dim)
        lines.append({"workload": "launches", "rows": B, "modes": m, "evaluate_ms": ev, "backward_ms": bw,
                      "evaluate_GB_per_s": ev_bytes / (ev * 1e-3) / 1e9, "backward_GB_per_s": bw_bytes / (bw * 1e-3) / 1e9,
                      "evaluate_ns_per_row": ev * 1e6 / B, "backward_ns_per_row": bw * 1e6 / B, "build_id": _lib.build_id(), "phase_ms": phases})
        print(json.dumps(lines[-1]), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("".join(json.dumps(line) + "\n" for line in lines))


if __name__ == "__main__":
    main()
