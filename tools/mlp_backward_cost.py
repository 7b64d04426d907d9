"""python tools/mlp_backward_cost.py [--reps 15] [--warmup 3] [--out profiles/mlp_backward_cost.txt]

What the training forward and backward of the reference's networks cost on the device: float32, measured in one process, the routes
taking turns from one repetition to the next on the same tensors:

  TrainMLP  rl_ptg_amd.TrainMLP under autograd: y = net(x); y.backward(g) -- mlp_forward with keep_hidden (one launch per layer), then
            mlp_backward (k_mlp_dw and k_mlp_dx per layer, no first-layer dx: the observations need no gradient), then autograd's copy of
            every returned gradient into .grad (the parameters' .grad is None before every repetition, as after SB3's zero_grad())
  raw       the same two library calls without autograd, the gradients written straight into preallocated .grad tensors: what a captured
            gradient step runs (no copy, no graph bookkeeping)
  torch     the eager route a caller writes today: y = seq(x); y.backward(g) on the same nn.Sequential, .grad None before every repetition

Two sections per shape: the backward alone (the forward runs untimed before every timed backward) and forward + backward.
Shapes: the nets of tools/mlp_cost.py (the reference's config/config_agent.yaml) at B = 6 and at each agent's own batch size.
Every timed section is queued behind a ~100 us device-side delay (cost_timing.timed), so the events bracket device work only -- for a
launch-bound route the device then waits for the host inside the interval, which is that route's cost.  Medians with min and max over
--reps repetitions after --warmup unrecorded ones."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cost_timing  # noqa: E402
from cost_timing import stats  # noqa: E402
from mlp_cost import NETS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mlp_backward_cost.txt"))
    args = ap.parse_args()
    import torch
    from rl_ptg_amd import TrainMLP, dist as ptg_dist
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    spec, _ = synthetic_spec(scenario=1, operation="OP1", eps_len_d=32)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    eng = HipEngine(spec.consts, spec.tables, spec.markets, 6, device=0, out_dtype="float32", obs_layout="sb3_flat")      # B is not tied to the engine's envs
    first_ptr, stride = ptg_dist.episode_plan(6, 1, 0)
    eng.set_episode_plan(spec.eps_ind, first_ptr, stride)
    say(f"# tools/mlp_backward_cost.py: float32 nets; {args.reps} repetitions after {args.warmup} warm-up, routes taking turns; device time from HIP events "
        f"[us]: median [min - max]")
    say(f"# torch {torch.__version__}; {torch.cuda.get_device_name(0)}; library {os.environ.get('PTG_LIB_PATH', 'in-tree default')}")
    say(f"{'net':>12s} {'B':>6s} {'what':>8s} {'launches':>8s}  {'TrainMLP':>30s}  {'raw':>30s}  {'torch':>30s} {'torch/TrainMLP':>14s} {'torch/raw':>9s}")
    torch.manual_seed(0)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    lost = []
    for name, fan_in, widths, act, own in NETS:
        mods, k = [], fan_in
        for l, w in enumerate(widths):
            mods.append(torch.nn.Linear(k, w))
            if l < len(widths) - 1:
                mods.append(torch.nn.ReLU() if act == "relu" else torch.nn.Tanh())
            k = w
        seq = torch.nn.Sequential(*mods).to(dev)
        lin = [m for m in seq if isinstance(m, torch.nn.Linear)]
        ws, bs = [m.weight.detach() for m in lin], [m.bias.detach() for m in lin]
        n = len(widths)
        for B in [6] + ([own] if own else []):
            x = torch.rand((B, fan_in), device=dev, generator=g) * 2 - 1
            gout = torch.rand((B, widths[-1]), device=dev, generator=g) * 2 - 1
            net = TrainMLP(eng, seq, batch=B)
            gw, gb = [torch.empty_like(w) for w in ws], [torch.empty_like(b) for b in bs]
            out = torch.empty((B, widths[-1]), device=dev)
            work, bwork = torch.empty_like(net.workspace), torch.empty_like(net.backward_workspace)

            def clear():
                for p in seq.parameters():
                    p.grad = None

            raw_fwd = lambda: eng.mlp_forward(x, ws, bs, hidden_activation=act, out=out, workspace=work, keep_hidden=True)
            raw_bwd = lambda: eng.mlp_backward(gout, x, ws, bs, out, work, hidden_activation=act, grad_weights=gw, grad_biases=gb, backward_workspace=bwork)
            routes = {"TrainMLP": (lambda: net(x), lambda y: y.backward(gout)), "raw": (raw_fwd, lambda y: raw_bwd()), "torch": (lambda: seq(x), lambda y: y.backward(gout))}
            t = {(r, s): [] for r in routes for s in ("backward", "both")}
            for rep in range(args.warmup + args.reps):
                for r, (fwd, bwd) in routes.items():
                    clear()
                    y = fwd()
                    tb = cost_timing.timed(lambda: bwd(y))[0]
                    clear()
                    tfb = cost_timing.timed(lambda: bwd(fwd()))[0]
                    if rep >= args.warmup:
                        t[(r, "backward")].append(tb)
                        t[(r, "both")].append(tfb)
            eng.sync()
            clear()
            net(x).backward(gout)
            mine = [p.grad.clone() for p in seq.parameters()]
            clear()
            seq(x).backward(gout)
            diff = max(float((a - p.grad).abs().max() / p.grad.abs().max()) for a, p in zip(mine, seq.parameters()))
            for s, launches in (("backward", 2 * n - 1), ("both", 3 * n - 1)):
                med = {r: statistics.median(t[(r, s)]) for r in routes}
                say(f"{name:>12s} {B:6d} {s:>8s} {launches:8d}  {stats(t[('TrainMLP', s)]):>30s}  {stats(t[('raw', s)]):>30s}  {stats(t[('torch', s)]):>30s} "
                    f"{med['torch'] / med['TrainMLP']:14.2f} {med['torch'] / med['raw']:9.2f}" + (f"   # max rel |TrainMLP .grad - torch .grad| {diff:.1e}" if s == "both" else ""))
                if s == "both" and own is not None and B == own and med["TrainMLP"] > med["torch"]:
                    lost.append((name, B, med["TrainMLP"], med["raw"], med["torch"]))
                    say(f"#   TrainMLP'S MEDIAN FORWARD + BACKWARD IS ABOVE TORCH'S: {med['TrainMLP']:.1f} (raw {med['raw']:.1f}) against {med['torch']:.1f} us")
            del net, x, gout
            clear()
            torch.cuda.empty_cache()
    say("# condition (each agent's own batch size, forward + backward): TrainMLP's median is not above torch's -- " +
        ("held at every such shape" if not lost else "MISSED at " + ", ".join(f"{n} B={b} ({m:.1f}, raw {r:.1f}, vs {t_:.1f} us)" for n, b, m, r, t_ in lost)))
    say("# launches: the project kernels of the raw route -- the forward's n, the backward's 2 n - 1 (no first-layer dx: x needs no gradient; out_act NONE: no last-layer pass); "
        "TrainMLP adds autograd's 2 n copies into .grad.")
    say("# not measured: an input that needs its gradient, the two-piece input, tanh outputs, accumulation, the kernels under a profiler, the host time of a call.")
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
