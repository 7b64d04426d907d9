"""python tools/train_group_cost.py [--reps 15] [--warmup 3] [--out profiles/train_group_cost.txt]

What the grouped policy loss and the grouped optimiser step cost on the device against the route they replace:
float32, one process, the routes taking turns from one repetition to the next, the route that goes first rotating.

(a) policy_loss_group against the G single policy_loss calls taken in turn, raw calls into preallocated outputs:
    PPO B = 203, A = 5, G in {2, 4, 6, 8};  A2C B = 3 948 with normalize_advantage, G in {2, 6}.
(b) optim_step_group against the G single optim_step calls taken in turn:
    PPO's parameter set per member (40 -> 358 -> 358 -> 5 and 40 -> 358 -> 358 -> 1), Adam with clipping and zero_grad, G in {2, 4, 6, 8};
    A2C's two 4 x 808 nets per member, RMSprop with clipping, G in {2, 6}.
    (a) and (b): every timed section is queued behind a ~100 us device-side delay (cost_timing.timed), so the HIP events bracket device
    work only; median [min - max] over --reps repetitions after --warmup unrecorded ones.
(c) a whole captured gradient step of G = 4 PPO agents at the reference's shape (B = 203 of 2 639 rows): per-agent next_batch, ONE
    TrainMLPGroup of eight nets, ppo_loss_group, one backward, DeviceOptimizerGroup -- one graph -- against the parent's route: the four
    single-agent graphs (next_batch, TrainMLPGroup of two nets, ppo_loss, backward, DeviceOptimizer) replayed in turn on one stream.
    Wall time per step of all four agents over --replays replays with one synchronisation at the end.  Beside it, without a condition:
    the same four graphs on four streams, and a graph of the four gathers alone as a share of the grouped replay.
The one condition: at every shape of (a), (b) and (c) the grouped route's median is not above the parent route's median."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cost_timing  # noqa: E402
from cost_timing import stats  # noqa: E402

PPO_NETS = [[40, 358, 358, 5], [40, 358, 358, 1]]
A2C_NETS = [[40, 808, 808, 808, 808, 5], [40, 808, 808, 808, 808, 1]]


def _shapes(nets):
    return [s for net in nets for a, b in zip(net, net[1:]) for s in ((b, a), (b,))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "train_group_cost.txt"))
    args = ap.parse_args()
    import torch
    from torch import nn
    from rl_ptg_amd import DeviceOptimizer, DeviceOptimizerGroup, DeviceRolloutBuffer, TrainMLPGroup, dist as ptg_dist, ppo_loss, ppo_loss_group
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    spec, _ = synthetic_spec(scenario=1, operation="OP1", eps_len_d=32)
    lines, lost = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    N = 7                                                    # 7 envs x 377 steps = 2 639 rows = 13 batches of 203
    eng = HipEngine(spec.consts, spec.tables, spec.markets, N, device=0, out_dtype="float32", obs_layout="sb3_flat")
    first_ptr, stride = ptg_dist.episode_plan(N, 1, 0)
    eng.set_episode_plan(spec.eps_ind, first_ptr, stride)
    say(f"# tools/train_group_cost.py: float32; {args.reps} repetitions after {args.warmup} warm-up, routes taking turns, the first one rotating; "
        f"[us]: median [min - max]")
    say(f"# torch {torch.__version__}; {torch.cuda.get_device_name(0)}; library {os.environ.get('PTG_LIB_PATH', 'in-tree default')}; "
        f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', 'unset')}")
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)

    def take_turns(routes):
        """device time of every route, the first one rotating"""
        names = list(routes)
        t = {r: [] for r in names}
        for rep in range(args.warmup + args.reps):
            for r in names[rep % len(names):] + names[:rep % len(names)]:
                dt = cost_timing.timed(routes[r])[0]
                if rep >= args.warmup:
                    t[r].append(dt)
        return t

    def row(section, shape, G, launches, t, a="group", b="singles"):
        ma, mb = statistics.median(t[a]), statistics.median(t[b])
        held = ma <= mb
        say(f"{section:>3s} {shape:>34s} {G:2d} {launches:>16s}  {stats(t[a]):>28s}  {stats(t[b]):>28s} {mb / ma:8.2f}   {'held' if held else 'MISSED'}")
        if not held:
            lost.append(f"{section} {shape} G={G} ({ma:.1f} vs {mb:.1f} us)")

    say(f"{'':>3s} {'shape':>34s} {'G':>2s} {'launches grp/sgl':>16s}  {'grouped':>28s}  {'G single calls in turn':>28s} {'sgl/grp':>8s}   condition")
    # ------------------------------------------------------------------ (a) the loss
    for kind, B, A, norm, Gs in (("ppo", 203, 5, True, (2, 4, 6, 8)), ("a2c", 3948, 5, True, (2, 6))):
        for G in Gs:
            members, outs = [], {}
            for i in range(G):
                ac = rn(B, A + 1)
                m = dict(head_input=ac[:, :A], values=ac[:, A], actions=torch.randint(0, A, (B,), device=dev, generator=g), advantages=rn(B), returns=rn(B),
                         ent_coef=0.01 * i, vf_coef=0.5)
                if kind == "ppo":
                    m.update(old_log_prob=-1.6 + 0.1 * rn(B), clip_range=0.1 + 0.02 * i)
                members.append(m)
            for r in ("group", "singles"):                   # one set of outputs per route: neither leg warms the other's
                outs[r] = [((torch.empty(8, dtype=torch.float64, device=dev), torch.empty(B, A, device=dev), torch.empty(B, device=dev), None),
                            eng.policy_loss_workspace(B)) for _ in range(G)]
            grouped = [dict(m, out=o, workspace=w) for m, (o, w) in zip(members, outs["group"])]

            def singles():
                for m, (o, w) in zip(members, outs["singles"]):
                    eng.policy_loss(kind, m["head_input"], m["values"], m["actions"], m.get("old_log_prob"), m["advantages"], m["returns"], clip_range=m.get("clip_range"),
                                    ent_coef=m["ent_coef"], vf_coef=m["vf_coef"], normalize_advantage=norm, out=o, workspace=w)
            t = take_turns({"group": lambda: eng.policy_loss_group(kind, grouped, normalize_advantage=norm), "singles": singles})
            eng.sync()
            same = all(torch.equal(a[0][k], b[0][k]) for a, b in zip(outs["group"], outs["singles"]) for k in range(3))
            per = 1 if B <= 256 else (4 if norm else 2)
            row("(a)", f"{kind} loss B={B} A={A}" + ("" if same else " BITS DIFFER"), G, f"{per} / {G * per}", t)
    # ------------------------------------------------------------------ (b) the optimiser
    for label, nets, kind, Gs in (("PPO pi+vf 2x358 adam clip zero", PPO_NETS, "adam", (2, 4, 6, 8)), ("A2C pi+vf 4x808 rmsprop clip", A2C_NETS, "rmsprop", (2, 6))):
        for G in Gs:
            plans = {}
            for r in ("group", "singles"):
                plans[r] = []
                for i in range(G):
                    params, grads = [0.1 * rn(*s) for s in _shapes(nets)], [rn(*s) for s in _shapes(nets)]
                    plans[r].append(eng.optim_plan(params, grads, kind))
            kw = dict(eps=1e-5, max_grad_norm=0.5, zero_grad=kind == "adam")
            lrs = [3e-4 * (i + 1) for i in range(G)]

            def singles():
                for p, lr in zip(plans["singles"], lrs):
                    eng.optim_step(p, lr, **kw)
            t = take_turns({"group": lambda: eng.optim_step_group(plans["group"], lrs, **kw), "singles": singles})
            eng.sync()
            p0 = plans["group"][0]
            row("(b)", f"{label}", G, f"3 / {3 * G}", t)
            say(f"#       per member {sum(p.numel() for p in p0.params)} parameters in {len(p0.params)} tensors, {p0.n_chunks} chunks")
            del plans
            torch.cuda.empty_cache()
    # ------------------------------------------------------------------ (c) the captured gradient step of four PPO agents
    G, B, T, F, A = 4, 203, 377, eng.obs_dim, 5
    lr, clip = [3e-4, 1e-4, 5e-4, 2e-4], [0.2, 0.1, 0.3, 0.15]

    def agent_nets(seed):
        torch.manual_seed(seed)
        return [nn.Sequential(nn.Linear(F, 358), nn.ReLU(), nn.Linear(358, 358), nn.ReLU(), nn.Linear(358, o)).to(dev) for o in (A, 1)]

    def filled_buffer(seed):
        buf = DeviceRolloutBuffer(eng, T, seed=seed)
        buf.storage.obs_rows.copy_(torch.rand(buf.storage.obs_rows.shape, device=dev, generator=g))
        buf.actions.copy_(torch.randint(0, A, (T, N), device=dev, generator=g))
        buf.values.copy_(0.1 * rn(T, N)); buf.log_probs.copy_(-1.6 + 0.1 * rn(T, N)); buf.advantages.copy_(rn(T, N)); buf.returns.copy_(rn(T, N))
        return buf

    def optimizer(params, i):
        for p in params:
            p.grad = torch.zeros_like(p)
        return DeviceOptimizer(eng, params, kind="adam", lr=lr[i], eps=1e-5, max_grad_norm=0.5, zero_grad=True)

    def capture(fn):
        fn()                                                 # the eager step: plans are built, buffers exist
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        return graph

    # the grouped route
    bufs = [filled_buffer(10 + i) for i in range(G)]
    pairs = [agent_nets(50 + i) for i in range(G)]
    grp = TrainMLPGroup(eng, [m for pair in pairs for m in pair], batch=B)
    owned = [[p for m in pair for p in m.parameters()] for pair in pairs]
    ogrp = DeviceOptimizerGroup(eng, [optimizer(owned[i], i) for i in range(G)])
    wss = [eng.policy_loss_workspace(B) for _ in range(G)]
    samples = [None] * G

    def gathers():
        for i in range(G):
            samples[i] = bufs[i].next_batch(B, out=samples[i])

    def grouped_step():
        gathers()
        outs = grp([s.observations for s in samples for _ in range(2)])
        members = [dict(head_input=outs[2 * i], values=outs[2 * i + 1], actions=samples[i].actions, old_log_prob=samples[i].old_log_prob,
                        advantages=samples[i].advantages, returns=samples[i].returns, workspace=wss[i]) for i in range(G)]
        losses, _ = ppo_loss_group(eng, members, clip_range=clip, ent_coef=0.01)
        torch.autograd.backward(losses)
        ogrp.step()
    g_group = capture(grouped_step)
    g_gather = capture(gathers)

    # the parent's route: one graph per agent
    class Single:
        def __init__(self, i):
            self.i, self.buf = i, filled_buffer(20 + i)
            self.grp = TrainMLPGroup(eng, agent_nets(50 + i), batch=B)
            self.opt = optimizer(self.grp.parameters(), i)
            self.ws, self.samples = eng.policy_loss_workspace(B), None

        def __call__(self):
            s = self.samples = self.buf.next_batch(B, out=self.samples)
            logits, values = self.grp(s.observations)
            loss, _ = ppo_loss(eng, logits, values, s.actions, s.old_log_prob, s.advantages, s.returns, clip_range=clip[self.i], ent_coef=0.01, workspace=self.ws)
            loss.backward()
            self.opt.step()
    singles = [Single(i) for i in range(G)]
    g_single = [capture(s) for s in singles]
    streams = [torch.cuda.Stream() for _ in range(G)]

    def in_turn():
        for gr in g_single:
            gr.replay()

    def on_streams():
        for gr, s in zip(g_single, streams):
            with torch.cuda.stream(s):
                gr.replay()
    routes = {"group": g_group.replay, "singles": in_turn, "streams": on_streams, "gathers": g_gather.replay}
    names = list(routes)
    t = {r: [] for r in names}
    for rep in range(args.warmup + args.reps):
        for r in names[rep % len(names):] + names[:rep % len(names)]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.replays):
                routes[r]()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                t[r].append((time.perf_counter() - t0) * 1e6 / args.replays)
    eng.sync()
    say(f"# (c) wall time per gradient step of all {G} agents [us], {args.replays} replays and one synchronisation per repetition")
    row("(c)", f"PPO step 2x358 B={B} of {T * N} rows", G, "1 graph / 4", t)
    mg = statistics.median(t["group"])
    say(f"#       the same four graphs on four streams: {stats(t['streams'])}   (grouped / this: {mg / statistics.median(t['streams']):.2f}; no condition)")
    say(f"#       the four gathers alone, one graph:    {stats(t['gathers'])}   ({100 * statistics.median(t['gathers']) / mg:.0f} % of a grouped replay; no condition)")
    say("# condition (every shape of (a), (b), (c)): the grouped route's median is not above the parent route's median -- " +
        ("held at every shape" if not lost else "MISSED at " + "; ".join(lost)))
    say("# not measured: float64, the Gaussian head, G agents as G processes, the kernels under a profiler.")
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
