"""python tools/optim_cost.py [--reps 15] [--warmup 3] [--out profiles/optim_cost.txt]

What the optimiser step behind loss.backward() costs on the device: float32 parameters at the reference's network shapes
(config/config_agent.yaml) over the 40-column observation, measured in one process, the routes taking turns on tensors of the same shapes:

  DeviceOptimizer   rl_ptg_amd.DeviceOptimizer.step(): norm pass (when clipping), head kernel, update -- three launches, two without
                    clipping, whatever the number of tensors; zero_grad is part of the update
  torch foreach     clip_grad_norm_ + torch.optim.Adam / RMSprop .step() (the default multi-tensor route) + zero_grad(set_to_none=False)
  torch fused       the same with fused=True, where this torch build offers it for the optimizer
  polyak            HipEngine.polyak_update (one launch) against SB3's polyak_update loop (two launches per tensor)

Shapes: PPO 2 x 358 (actor and critic, Adam, clip 0.5), A2C 4 x 808 (actor and critic, RMSprop, clip 0.5), DQN 7 x 366 (one Q-network,
Adam, clip 10), TD3 3 x 743 (the two critics of one optimizer over observation + action, Adam, no clip, targets with tau 0.005).
Every timed section is queued behind a ~100 us device-side delay (tools/cost_timing.py), so the events bracket device work only -- for
the launch-bound torch routes the device then waits for the host inside the interval, which is that route's cost.
Compulsory bytes per element at float32: Adam 16 read (p, g, m, v) + 12 written (p, m, v), + 4 with a norm pass (the gradient is read
twice), + 8 with a target; RMSprop 12 read + 8 written.  The 4 bytes of the zeroed gradient, which every route here also writes, are not counted.  The floor of these shapes is the chain's
launch count times the 6-7 us of one short launch between two events (profiles/minibatch_cost.txt)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cost_timing import stats, timed  # noqa: E402


def mlp_shapes(n_in, width, depth, n_out):
    dims = [n_in] + [width] * depth + [n_out]
    out = []
    for a, b in zip(dims[:-1], dims[1:]):
        out += [(b, a), (b,)]
    return out


CASES = [  # name, kind, parameter shapes, max_grad_norm, targets
    ("PPO 2x358", "adam", mlp_shapes(40, 358, 2, 5) + mlp_shapes(40, 358, 2, 1), 0.5, False),
    ("A2C 4x808", "rmsprop", mlp_shapes(40, 808, 4, 5) + mlp_shapes(40, 808, 4, 1), 0.5, False),
    ("DQN 7x366", "adam", mlp_shapes(40, 366, 7, 5), 10.0, False),
    ("TD3 3x743", "adam", mlp_shapes(41, 743, 3, 1) * 2, None, True),
]
LR, EPS, TAU = 3e-4, 1e-5, 0.005


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "optim_cost.txt"))
    args = ap.parse_args()
    import torch
    from rl_ptg_amd import DeviceOptimizer
    from rl_ptg_amd import dist as ptg_dist
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    spec, _ = synthetic_spec(scenario=1, operation="OP1", eps_len_d=32)
    eng = HipEngine(spec.consts, spec.tables, spec.markets, 6, device=0, out_dtype="float32", obs_layout="sb3_flat")
    first_ptr, stride = ptg_dist.episode_plan(6, 1, 0)
    eng.set_episode_plan(spec.eps_ind, first_ptr, stride)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def rounds(fns):
        """the times of every route, taken in turns"""
        ts = [[] for _ in fns]
        for rep in range(args.warmup + args.reps):
            for k, fn in enumerate(fns):
                t = timed(fn)[0]
                if rep >= args.warmup:
                    ts[k].append(t)
        return ts

    g = torch.Generator(device="cuda")
    g.manual_seed(1)

    def leaves(shapes):
        ps = [(torch.randn(s, device=dev, generator=g) * 0.1).requires_grad_(True) for s in shapes]
        for p in ps:
            p.grad = torch.randn(p.shape, device=dev, generator=g) * 0.01
        return ps

    def torch_route(ps, kind, clip, **kw):
        opt = torch.optim.Adam(ps, lr=LR, eps=EPS, **kw) if kind == "adam" else torch.optim.RMSprop(ps, lr=LR, alpha=0.99, eps=EPS, **kw)

        def run():
            if clip is not None:
                torch.nn.utils.clip_grad_norm_(ps, clip)
            opt.step()
            opt.zero_grad(set_to_none=False)
        return run

    def sb3_polyak(ps, qs):
        def run():
            with torch.no_grad():
                for p, q in zip(ps, qs):
                    q.data.mul_(1 - TAU)
                    torch.add(q.data, p.data, alpha=TAU, out=q.data)
        return run

    say(f"# tools/optim_cost.py: float32; {args.reps} repetitions after {args.warmup} warm-up, routes taking turns; device time from HIP events [us]: median [min - max]")
    say(f"# torch {torch.__version__}; {torch.cuda.get_device_name(0)}; library {os.environ.get('PTG_LIB_PATH', 'in-tree default')}; chunk {eng.optim_chunk()} elements")
    say(f"{'network':>10s} {'optimizer':>9s} {'tensors':>7s} {'elements':>9s} {'launches':>8s}  {'DeviceOptimizer':>30s}  {'torch foreach':>30s}  {'torch fused':>30s} "
        f"{'foreach/dev':>11s} {'fused/dev':>9s}  {'GB/s':>7s}")
    for name, kind, shapes, clip, with_targets in CASES:
        ps_dev, ps_fe, ps_fu = leaves(shapes), leaves(shapes), leaves(shapes)
        targets = [p.detach().clone() for p in ps_dev] if with_targets else None
        opt = DeviceOptimizer(eng, ps_dev, kind=kind, lr=LR, eps=EPS, max_grad_norm=clip, targets=targets, tau=TAU if with_targets else None, zero_grad=True)
        routes = [opt.step, torch_route(ps_fe, kind, clip)]
        fused = None
        try:
            fused = torch_route(ps_fu, kind, clip, fused=True)
            fused()
            torch.cuda.synchronize()
            routes.append(fused)
        except Exception as e:                                  # this build has no fused kernel for the optimizer
            fused = None
            why = type(e).__name__
        if with_targets:                                        # the torch routes move their targets with SB3's loop: part of their step
            for k in (1, 2)[:len(routes) - 1]:
                step, pol = routes[k], sb3_polyak((ps_fe, ps_fu)[k - 1], [p.detach().clone() for p in ps_dev])
                routes[k] = (lambda s, q: lambda: (s(), q()))(step, pol)
        ts = rounds(routes)
        eng.sync()
        n = sum(p.numel() for p in ps_dev)
        per = (16 + 12 if kind == "adam" else 12 + 8) + (4 if clip is not None else 0) + (8 if with_targets else 0)
        md = statistics.median(ts[0])
        fu = f"{stats(ts[2]):>30s}" if fused else f"{'not offered (' + why + ')':>30s}"
        fr = f"{statistics.median(ts[2]) / md:9.2f}" if fused else f"{'-':>9s}"
        say(f"{name:>10s} {kind:>9s} {len(shapes):7d} {n:9d} {3 if clip is not None else 2:8d}  {stats(ts[0]):>30s}  {stats(ts[1]):>30s}  {fu} "
            f"{statistics.median(ts[1]) / md:11.2f} {fr}  {n * per / md * 1e-3:7.1f}")
    say("# polyak_update alone (tau 0.005), one launch against SB3's loop of two launches per tensor")
    say(f"{'network':>10s} {'tensors':>7s} {'elements':>9s}  {'HipEngine.polyak_update':>30s}  {'SB3 loop':>30s} {'loop/dev':>9s}  {'GB/s':>7s}")
    for name, kind, shapes, clip, with_targets in (CASES[3], CASES[2]):
        ps = [p.detach() for p in leaves(shapes)]
        qs, qs2 = [p.clone() for p in ps], [p.clone() for p in ps]
        plan = eng.polyak_update(ps, qs, TAU)
        ta, tb = rounds([lambda: eng.polyak_update(ps, qs, TAU, plan=plan), sb3_polyak(ps, qs2)])
        eng.sync()
        n = sum(p.numel() for p in ps)
        say(f"{name:>10s} {len(shapes):7d} {n:9d}  {stats(ta):>30s}  {stats(tb):>30s} {statistics.median(tb) / statistics.median(ta):9.2f}  "
            f"{n * 12 / statistics.median(ta) * 1e-3:7.1f}")
    say("# GB/s: compulsory bytes per element (Adam 28, RMSprop 20, + 4 norm pass, + 8 target; the zeroed gradient not counted; polyak alone 12) over the device route's")
    say("# median.  The floor is the launch count times the 6-7 us of one short launch between two events.")
    say("# not measured: float64 parameters, views at odd offsets (the element-wise path), lr as a device tensor, the captured (hipGraph) call,")
    say("# the host time of a call, torch's single-tensor route (foreach=False), the kernels under a profiler, lists of more than 20 tensors.")
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
