"""python tools/mlp_cost.py [--reps 15] [--warmup 3] [--out profiles/mlp_cost.txt]

What the inference forward of the reference's networks costs on the device: float32, measured in one process, the routes taking turns
from one repetition to the next on the same tensors:

  kernel  rl_ptg_amd.DeviceMLP into its preallocated output and workspace: one fused launch per layer (the host's choice of tile route);
          beside it HipEngine.mlp_forward with every layer forced onto the narrow and onto the wide route -- the host's switch is taken
          from these two columns
  torch   the eager route a caller writes today: the nn.Sequential under torch.no_grad(), float32 -- per Linear a BLAS launch and an
          activation launch

Shapes: the six nets of the reference's config/config_agent.yaml (DQN 7 x 366 ReLU, A2C 4 x 808 Tanh, PPO 2 x 358 ReLU -- fan-in 40, 5
outputs; the critics of TD3 3 x 743 ReLU and SAC 6 x 233 Tanh -- fan-in 41, 1 output; TQC's 3 x 708 ReLU, 41 in, 30 quantiles) at B = 6
(the reference's envs), at each agent's own batch size (A2C has none: its n_steps, 658), at 4 096, at 16 384 (to place the host's switch) and at 65 536 rows; and the
40 -> 64 -> 64 -> 5 tanh net of tools/policy_loop.py.
Every timed section is queued behind a ~100 us device-side delay, so the host has enqueued its work before the first event is reached:
the events bracket device work only -- for a launch-bound route the device then waits for the host inside the interval, which is that
route's cost.  Medians with min and max over --reps repetitions after --warmup unrecorded ones.
TF/s: 2 B sum(in * out) over the kernel route's median, against the 157 TF peak of the exact-float32 MFMA."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cost_timing  # noqa: E402
from cost_timing import stats  # noqa: E402

NETS = [("DQN q_net", 40, [366] * 7 + [5], "relu", 544), ("A2C policy", 40, [808] * 4 + [5], "tanh", 658), ("PPO policy", 40, [358] * 2 + [5], "relu", 203),
        ("TD3 critic", 41, [743] * 3 + [1], "relu", 257), ("SAC critic", 41, [233] * 6 + [1], "tanh", 470), ("TQC critic", 41, [708] * 3 + [30], "relu", 290),
        ("policy_loop", 40, [64, 64, 5], "tanh", None)]
PEAK_TF = 157.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mlp_cost.txt"))
    args = ap.parse_args()
    import torch
    from rl_ptg_amd import DeviceMLP, dist as ptg_dist
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
    say(f"# tools/mlp_cost.py: float32 nets under no_grad; {args.reps} repetitions after {args.warmup} warm-up, routes taking turns; device time from HIP events "
        f"[us]: median [min - max]")
    say(f"# torch {torch.__version__}; {torch.cuda.get_device_name(0)}; library {os.environ.get('PTG_LIB_PATH', 'in-tree default')}")
    say(f"{'net':>12s} {'B':>6s} {'launches':>8s}  {'kernel route':>30s} {'TF/s':>6s} {'of peak':>7s}  {'torch route':>30s} {'torch/kernel':>12s}  {'narrow':>9s} {'wide':>9s}")
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
        ws, bs = [m.weight.detach() for m in seq if isinstance(m, torch.nn.Linear)], [m.bias.detach() for m in seq if isinstance(m, torch.nn.Linear)]
        flop = 2.0 * sum(w.numel() for w in ws)
        for B in [6] + ([own] if own else []) + [4096, 16384, 65536]:
            x = torch.rand((B, fan_in), device=dev, generator=g) * 2 - 1
            net = DeviceMLP(eng, seq, batch=B)
            out2 = torch.empty_like(net.out)

            def eager():
                with torch.no_grad():
                    return seq(x)

            forced = lambda route: (lambda: eng.mlp_forward(x, ws, bs, hidden_activation=act, out=out2, workspace=net.workspace, _route=route))
            tk, tt, tn, tw = [], [], [], []
            for rep in range(args.warmup + args.reps):
                t = [cost_timing.timed(f)[0] for f in (lambda: net(x), eager, forced("narrow"), forced("wide"))]
                if rep >= args.warmup:
                    tk.append(t[0]); tt.append(t[1]); tn.append(t[2]); tw.append(t[3])
            eng.sync()
            diff = float((net(x) - eager()).abs().max())
            mk, mt = statistics.median(tk), statistics.median(tt)
            tf = flop * B / mk * 1e-6
            say(f"{name:>12s} {B:6d} {len(widths):8d}  {stats(tk):>30s} {tf:6.2f} {100 * tf / PEAK_TF:6.1f}%  {stats(tt):>30s} {mt / mk:12.2f}  {statistics.median(tn):9.1f} {statistics.median(tw):9.1f}"
                f"   # max |kernel - torch| {diff:.1e}")
            if own is not None and B in (6, own) and mk > mt:
                lost.append((name, B, mk, mt))
                say(f"#   THE KERNEL ROUTE'S MEDIAN IS ABOVE THE TORCH ROUTE'S: {mk:.1f} against {mt:.1f} us")
            del net, out2, x
            torch.cuda.empty_cache()
    say("# condition (B = 6 and the agents' own batch sizes only): the kernel route's median is not above the torch route's -- " +
        ("held at every such shape" if not lost else "MISSED at " + ", ".join(f"{n} B={b} ({mk:.1f} vs {mt:.1f} us)" for n, b, mk, mt in lost)))
    say("# launches: the kernel route's, one per layer; torch issues one BLAS launch per Linear and one per activation (about 2 n - 1, addmm folding the bias).")
    say("# narrow / wide: medians with every layer forced onto that route (a fresh output tensor, the same workspace); the kernel route column is the host's choice.")
    say("# not measured: keep_hidden, strided inputs, the two-piece input, other tile shapes, the kernels under a profiler, the host time of a call.")
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
