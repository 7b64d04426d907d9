"""python tools/mlp_group_cost.py [--reps 15] [--warmup 3] [--out profiles/mlp_group_cost.txt]

What the grouped MLP calls cost on the device against the route they replace: float32, measured in one process, the routes taking turns
from one repetition to the next on the same tensors:

  group     mlp_group_forward / mlp_group_backward: G networks in the launches of one, into preallocated buffers
  singles   the G single calls mlp_forward / mlp_backward one after the other, into the same kind of buffers: the route before the
            grouped calls existed
  torch     the same G nn.Sequentials: under no_grad for the forward alone; y_i = seq_i(x), torch.autograd.backward(ys, gs) for forward +
            backward, .grad None before every repetition
  class     DeviceMLPGroup (the forward alone) and TrainMLPGroup under autograd (forward + backward, .grad None before every repetition)

Two sections per shape: the forward alone (inference: no kept activations) and forward (keep_hidden) + backward (no first-layer dx: the
inputs need no gradient; every parameter gradient).  Shapes: the twin critics of TD3, SAC and TQC and the policy + value nets of PPO and
A2C with the reference's widths (tools/mlp_cost.py), at B = 6 and at each agent's own batch size; SAC's two critics and two targets as a
group of four, forward only.  All networks of a group read one input tensor.
Every timed section is queued behind a ~100 us device-side delay (cost_timing.timed), so the events bracket device work only -- for a
launch-bound route the device then waits for the host inside the interval, which is that route's cost.  Medians with min and max over
--reps repetitions after --warmup unrecorded ones; the route that goes first changes with the repetition.  The last column is the host's own
time inside the timed call(s), median: a grouped call does the argument checks of all its networks BEFORE its first launch, the single calls
check network i + 1 while network i's kernels run, so where the checks outlast the delay the device waits for the grouped call's host.
The one condition: at each shape and section the median of `group` is not above the median of `singles`."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cost_timing  # noqa: E402
from cost_timing import stats  # noqa: E402

# (name, fan-in, [the widths of each network], hidden activation, the agent's own batch size, sections)
GROUPS = [("TD3 critics", 41, [[743] * 3 + [1]] * 2, "relu", 257, ("forward", "both")),
          ("SAC critics", 41, [[233] * 6 + [1]] * 2, "tanh", 470, ("forward", "both")),
          ("TQC critics", 41, [[708] * 3 + [30]] * 2, "relu", 290, ("forward", "both")),
          ("PPO pi + vf", 40, [[358] * 2 + [5], [358] * 2 + [1]], "relu", 203, ("forward", "both")),
          ("A2C pi + vf", 40, [[808] * 4 + [5], [808] * 4 + [1]], "tanh", 658, ("forward", "both")),
          ("SAC 2 + 2", 41, [[233] * 6 + [1]] * 4, "tanh", 470, ("forward",))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mlp_group_cost.txt"))
    args = ap.parse_args()
    import torch
    from rl_ptg_amd import DeviceMLPGroup, TrainMLPGroup, dist as ptg_dist
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
    say(f"# tools/mlp_group_cost.py: float32 nets; {args.reps} repetitions after {args.warmup} warm-up, routes taking turns; device time from HIP events "
        f"[us]: median [min - max]")
    say(f"# torch {torch.__version__}; {torch.cuda.get_device_name(0)}; library {os.environ.get('PTG_LIB_PATH', 'in-tree default')}")
    say(f"{'group':>12s} {'G':>2s} {'B':>5s} {'what':>8s} {'launches group / singles':>24s}  {'group':>28s}  {'singles':>28s}  {'torch':>28s}  {'class':>28s} "
        f"{'singles/group':>13s} {'torch/group':>11s} {'torch/class':>11s}")
    torch.manual_seed(0)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    lost = []
    for name, fan_in, all_widths, act, own, sections in GROUPS:
        G = len(all_widths)
        seqs = []
        for widths in all_widths:
            mods, k = [], fan_in
            for l, w in enumerate(widths):
                mods.append(torch.nn.Linear(k, w))
                if l < len(widths) - 1:
                    mods.append(torch.nn.ReLU() if act == "relu" else torch.nn.Tanh())
                k = w
            seqs.append(torch.nn.Sequential(*mods).to(dev))
        lins = [[m for m in seq if isinstance(m, torch.nn.Linear)] for seq in seqs]
        ws, bs = [[m.weight.detach() for m in lin] for lin in lins], [[m.bias.detach() for m in lin] for lin in lins]
        n = len(all_widths[0])
        params = [p for seq in seqs for p in seq.parameters()]
        for B in (6, own):
            x = torch.rand((B, fan_in), device=dev, generator=g) * 2 - 1
            gouts = [torch.rand((B, w[-1]), device=dev, generator=g) * 2 - 1 for w in all_widths]
            infer, train = DeviceMLPGroup(eng, seqs, batch=B), (TrainMLPGroup(eng, seqs, batch=B) if "both" in sections else None)
            u8 = lambda nbytes: torch.empty(nbytes, dtype=torch.uint8, device=dev)
            # two sets of buffers, one per raw route: neither leg warms the other's outputs
            buf = {r: dict(out=[torch.empty((B, w[-1]), device=dev) for w in all_widths], work=[u8(eng.mlp_workspace(B, w, True)) for w in all_widths],
                           bwork=[u8(eng.mlp_backward_workspace(B, w)) for w in all_widths], gw=[[torch.empty_like(w) for w in net] for net in ws],
                           gb=[[torch.empty_like(b) for b in net] for net in bs]) for r in ("group", "singles")}

            def clear():
                for p in params:
                    p.grad = None

            def group_fwd(keep):
                b = buf["group"]
                eng.mlp_group_forward(x, ws, bs, hidden_activation=act, outs=b["out"], workspaces=b["work"], keep_hidden=keep)

            def group_bwd():
                b = buf["group"]
                eng.mlp_group_backward(gouts, x, ws, bs, b["out"], b["work"], hidden_activation=act, grad_weights=b["gw"], grad_biases=b["gb"], backward_workspaces=b["bwork"])

            def singles_fwd(keep):
                b = buf["singles"]
                for i in range(G):
                    eng.mlp_forward(x, ws[i], bs[i], hidden_activation=act, out=b["out"][i], workspace=b["work"][i], keep_hidden=keep)

            def singles_bwd():
                b = buf["singles"]
                for i in range(G):
                    eng.mlp_backward(gouts[i], x, ws[i], bs[i], b["out"][i], b["work"][i], hidden_activation=act, grad_weights=b["gw"][i], grad_biases=b["gb"][i],
                                     backward_workspace=b["bwork"][i])

            def torch_fwd():
                with torch.no_grad():
                    return [seq(x) for seq in seqs]

            routes = {"forward": {"group": lambda: group_fwd(False), "singles": lambda: singles_fwd(False), "torch": torch_fwd, "class": lambda: infer(x)},
                      "both": {"group": lambda: (group_fwd(True), group_bwd()), "singles": lambda: (singles_fwd(True), singles_bwd()),
                               "torch": lambda: torch.autograd.backward([seq(x) for seq in seqs], gouts),
                               "class": lambda: torch.autograd.backward(list(train(x)), gouts)}}
            t = {(s, r): [] for s in sections for r in routes[s]}
            host = {(s, r): [] for s in sections for r in routes[s]}

            def hosted(fn, sink):                            # the host's time inside fn(): argument checks, ctypes, the launches; no wait for the device
                def run():
                    t0 = time.perf_counter()
                    fn()
                    sink.append((time.perf_counter() - t0) * 1e6)
                return run

            for rep in range(args.warmup + args.reps):
                for s in sections:
                    names = list(routes[s])
                    for r in names[rep % len(names):] + names[:rep % len(names)]:      # the route that goes first changes with the repetition
                        clear()
                        sink = []
                        dt = cost_timing.timed(hosted(routes[s][r], sink))[0]
                        if rep >= args.warmup:
                            t[(s, r)].append(dt)
                            host[(s, r)] += sink
            eng.sync()
            # the two raw routes wrote the same bits
            same = all(torch.equal(a, b) for k in ("out", "gw", "gb") for a, b in zip(_flat(buf["group"][k]), _flat(buf["singles"][k]))) if "both" in sections else \
                all(torch.equal(a, b) for a, b in zip(buf["group"]["out"], buf["singles"]["out"]))
            for s in sections:
                per_net = n if s == "forward" else 3 * n - 1
                med = {r: statistics.median(t[(s, r)]) for r in routes[s]}
                say(f"{name:>12s} {G:2d} {B:5d} {s:>8s} {per_net:11d} / {G * per_net:<10d}  {stats(t[(s, 'group')]):>28s}  {stats(t[(s, 'singles')]):>28s}  "
                    f"{stats(t[(s, 'torch')]):>28s}  {stats(t[(s, 'class')]):>28s} {med['singles'] / med['group']:13.2f} {med['torch'] / med['group']:11.2f} "
                    f"{med['torch'] / med['class']:11.2f}   # host us in the call(s): group {statistics.median(host[(s, 'group')]):.0f}, singles {statistics.median(host[(s, 'singles')]):.0f}, "
                    f"class {statistics.median(host[(s, 'class')]):.0f}" + ("" if same else "   # THE TWO RAW ROUTES DISAGREE IN BITS"))
                if med["group"] > med["singles"]:
                    lost.append((name, B, s, med["group"], med["singles"]))
                    say(f"#   THE GROUPED ROUTE'S MEDIAN IS ABOVE THE SINGLE CALLS': {med['group']:.1f} against {med['singles']:.1f} us")
            del infer, train, x, gouts, buf
            clear()
            torch.cuda.empty_cache()
    say("# condition (every shape and section): the grouped route's median is not above the median of the G single calls taken in turn -- " +
        ("held at every shape" if not lost else "MISSED at " + ", ".join(f"{n} B={b} {s} ({m:.1f} vs {o:.1f} us)" for n, b, s, m, o in lost)))
    say("# launches: the project kernels of the raw routes -- forward n, forward + backward 3 n - 1 per call (no first-layer dx, out_act NONE); the grouped route issues "
        "one call's launches for the whole group.  class: DeviceMLPGroup (forward) and TrainMLPGroup (both), which adds autograd's copies into .grad.")
    say("# not measured: the kernels under a profiler, groups above 4, an input that needs its gradient, the two-piece input, tanh outputs, the captured step against a "
        "captured torch twin.")
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def _flat(xs):
    return [t for x in xs for t in (x if isinstance(x, (list, tuple)) else [x])]


if __name__ == "__main__":
    main()
