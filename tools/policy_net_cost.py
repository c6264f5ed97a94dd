#!/usr/bin/env python
"""Cost of the actor-critic network as `wedm_policy_net` (through `PolicyNet`) against a float32 torch MLP of the same
shape, in the same process and build, in alternating rounds, timed with event pairs, medians.  D = 16 observation
columns, hidden = (64, 64), M = 9 modes:

  forward   `PolicyNet.forward` at 65 536 rows (one launch) next to the torch MLP's forward under ``no_grad``;
  a         one epoch of 128 x 65 536 rows in 8 minibatches: ``net(rollout=, index=)``, `PPOLoss.backward(rollout=, index=)`,
            the network's backward into ``theta.grad`` -- nothing is gathered;
  b         the same epoch with the torch MLP on `RolloutBuffer.minibatches` (a ``randperm`` and an index-select of every
            block), `PPOLoss.backward` on the gathered tensors, autograd through the library GEMMs.

Also prints the float32-MFMA work of a (the FLOPs of every product of the definition) as a fraction of 155 TFLOP/s.

    python tools/policy_net_cost.py [--rounds 5] [--out profiles/r17/policy_net_cost.jsonl] [--only a|b]

``--only`` runs one epoch path alone, three times after a warm-up, for a kernel trace of it.
Prints one JSON line per workload (every sample in it) and writes them to ``--out``."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

MFMA_F32_TFLOPS = 155.0


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r17" / "policy_net_cost.jsonl"))
    ap.add_argument("--only", choices=("a", "b"), default=None)
    args = ap.parse_args()

    import torch

    from sparc_amd import PolicyHead, PolicyNet, PPOLoss, RolloutBuffer, WireEDMEnv, WireEDMVectorEnv, _lib

    dev, N, T, parts, hidden = "cuda:0", 65536, 128, 8, (64, 64)
    TN = T * N
    B = TN // parts
    vec = WireEDMVectorEnv(WireEDMEnv(num_envs=N, device=dev, pulse_stats=True, signal_stats=True))
    head = PolicyHead(vec, modes=(1, 3, 5, 7, 9, 11, 13, 15, 17), seed=1)
    ppo = PPOLoss(head, clip=0.2, vf_coef=0.5, ent_coef=0.01)
    net = PolicyNet(vec, head, hidden=hidden, activation="tanh", seed=1)
    D, P, M, (H1, H2) = net.obs_dim, head.param_dim, len(head.modes), hidden
    O = P + 1
    assert (D, M) == (16, 9), (D, M)
    gen = torch.Generator(device=dev).manual_seed(1234)

    # ---- a rollout's blocks: one real step allocates them, seeded values fill them (the time does not depend on the physics)
    buf = RolloutBuffer(vec, T, extras={"log_prob": torch.float32})
    obs, _ = vec.reset(seed=1)
    obs = torch.randn(N, D, generator=gen, device=dev)
    with torch.no_grad():
        out = head.sample(net.forward(obs)[0])
    zero = torch.zeros(N, device=dev)
    buf.add(obs, head.stored(out), zero, zero, zero.bool(), zero.bool(), log_prob=out.log_prob)
    flat = {**{k: v.view((TN,) + tuple(v.shape[2:])) for k, v in buf.stored.items()}, **{k: v.view(TN) for k, v in buf.computed.items()}}
    with torch.no_grad():
        for j in range(parts):
            s = slice(j * B, (j + 1) * B)
            flat["obs"][s] = torch.randn(B, D, generator=gen, device=dev)
            p, _ = net.forward(flat["obs"][s])
            flat["action.u"][s] = p[:, 0:4] + p[:, 4:8].exp() * torch.randn(B, 4, generator=gen, device=dev)
            flat["action.mode_index"][s] = torch.randint(0, M, (B,), generator=gen, device=dev, dtype=torch.int32)
            flat["log_prob"][s] = head.evaluate(p, flat["action.u"][s], flat["action.mode_index"][s])[0]
        flat["value"].copy_(torch.randn(TN, generator=gen, device=dev))
        flat["advantage_norm"].copy_(torch.randn(TN, generator=gen, device=dev))
        flat["returns"].copy_(flat["value"] + torch.randn(TN, generator=gen, device=dev))
        flat["valid"].copy_(torch.rand(TN, generator=gen, device=dev) >= 0.02)
    stored_names = dict(u="action.u", mode_index="action.mode_index", old_log_prob="log_prob", advantage="advantage_norm",
                        returns="returns", valid="valid")
    perm_gen = torch.Generator(device=dev)

    # ---- the torch MLP: the same parameters as separate leaves
    leaves = {k: getattr(net, k).clone().requires_grad_(True) for k in ("W1", "b1", "W2", "b2", "W3", "b3")}

    def mlp(x):
        x = torch.nan_to_num(x)
        h = torch.tanh(torch.addmm(leaves["b1"], x, leaves["W1"]))
        h = torch.tanh(torch.addmm(leaves["b2"], h, leaves["W2"]))
        o = torch.addmm(leaves["b3"], h, leaves["W3"])
        return o[:, :P], o[:, P]

    def epoch_a():
        perm_gen.manual_seed(77)
        net.theta.grad = None
        for idx in torch.tensor_split(torch.randperm(TN, device=dev, generator=perm_gen), parts):
            params, value = net(rollout=buf, index=idx)
            ppo.backward(params, value, rollout=buf, index=idx)

    def epoch_b():
        perm_gen.manual_seed(77)
        for leaf in leaves.values():
            leaf.grad = None
        for mb in buf.minibatches(parts, generator=perm_gen):
            params, value = mlp(mb["obs"])
            ppo.backward(params, value, **{k: mb[name] for k, name in stored_names.items()})

    fwd_obs = flat["obs"][:N]

    def forward_net():
        net.forward(fwd_obs)

    def forward_torch():
        with torch.no_grad():
            mlp(fwd_obs)

    if args.only:
        fn = epoch_a if args.only == "a" else epoch_b
        for _ in range(4):
            fn()
        torch.cuda.synchronize()
        return
    work = {"a": (epoch_a, 3), "b": (epoch_b, 3), "forward": (forward_net, 200), "forward_torch": (forward_torch, 200)}
    for fn, _ in work.values():   # warm-up: buffers grown, code loaded
        fn()
    epoch_a()
    got = net.theta.grad.clone()
    epoch_b()
    torch.cuda.synchronize()
    want = torch.cat([leaves[k].grad.reshape(-1) for k in ("W1", "b1", "W2", "b2", "W3", "b3")])
    worst = float(((got - want).abs() / (1e-12 + want.abs().max())).max())
    assert worst < 1e-3, worst
    ms = {k: [] for k in work}
    for _ in range(args.rounds):
        for k, (fn, count) in work.items():
            ms[k].append(timed(fn, count))
    med = {k: statistics.median(v) for k, v in ms.items()}
    layers = D * H1 + H1 * H2 + H2 * O
    # net(): three layers; the backward: two layers again, two back-propagated products, three weight gradients
    flops = 2.0 * TN * (layers + (D * H1 + H1 * H2) + (H2 * O + H1 * H2) + layers)
    lines = [{"workload": "epoch", "rows": TN, "minibatches": parts, "obs_dim": D, "hidden": list(hidden), "modes": M,
              "a_policy_net_rollout_index_ms": med["a"], "b_torch_mlp_minibatches_ms": med["b"], "b_over_a": med["b"] / med["a"],
              "a_mfma_flop": flops, "a_fraction_of_155_tflops_over_the_whole_epoch": flops / (med["a"] * 1e-3) / (MFMA_F32_TFLOPS * 1e12),
              "largest_gradient_difference_relative_to_the_largest_gradient": worst, "build_id": _lib.build_id(),
              "ms": {k: ms[k] for k in ("a", "b")}},
             {"workload": "forward", "rows": N, "policy_net_ms": med["forward"], "torch_mlp_ms": med["forward_torch"],
              "policy_net_fraction_of_155_tflops": 2.0 * N * layers / (med["forward"] * 1e-3) / (MFMA_F32_TFLOPS * 1e12),
              "build_id": _lib.build_id(), "ms": {k: ms[k] for k in ("forward", "forward_torch")}}]
    for line in lines:
        print(json.dumps(line), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("".join(json.dumps(line) + "\n" for line in lines))


if __name__ == "__main__":
    main()
