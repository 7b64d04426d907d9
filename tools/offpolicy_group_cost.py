"""python tools/offpolicy_group_cost.py [--reps 15] [--warmup 3] [--out profiles/offpolicy_group_cost.txt]

What the grouped off-policy ops cost on the device against the route they replace: float32, one process, the
routes taking turns from one repetition to the next, the route that goes first rotating.

(a) each grouped op against the G single calls taken in turn, raw library calls on descriptors built beforehand into preallocated
    outputs, G in {2, 4, 6, 8}, at the reference's shapes: the TD loss of SAC (B = 470, K = 2, log alpha), TD3 (B = 257, K = 2) and DQN
    (B = 544, A = 5); SAC's actor loss (B = 470, K = 2) and the entropy-coefficient loss alone (B = 470); TD3's actor loss (B = 257);
    rsample and rsample_backward (B = 470); TD3's smoothing (B = 257).  Every timed section is queued behind a ~100 us device-side delay
    (cost_timing.timed), so the HIP events bracket device work only -- unless the host needs longer than the delay to enqueue the
    section: such a row is marked "host-bound" (the host's median enqueue time stands beside it).
    median [min - max] over --reps repetitions after --warmup unrecorded ones.
(b) a whole captured SAC gradient step of G = 4 agents at the reference's networks (6 x 233, Tanh; B = 470) as ONE graph -- TrainMLPGroup
    of the four actors, of the eight critics, DeviceMLPGroup of the eight targets, the *_group losses, three DeviceOptimizerGroups --
    against the parent's route: the four single-agent graphs replayed in turn on one stream.  Wall time per step of all four agents over
    --replays replays with one synchronisation at the end.
The one condition: at every shape of (a) and (b) the grouped route's median is not above the parent route's median."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cost_timing  # noqa: E402
from cost_timing import stats  # noqa: E402

DELAY_US = 100.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--sections", default="ab", help="which of (a) and (b) to run")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "offpolicy_group_cost.txt"))
    args = ap.parse_args()
    import torch
    from torch import nn
    from rl_ptg_amd import (DeviceMLPGroup, DeviceOptimizer, DeviceOptimizerGroup, TrainMLP, TrainMLPGroup, _lib, ent_coef_loss, ent_coef_loss_group, sac_actor_loss,
                            sac_actor_loss_group, sac_critic_loss, sac_critic_loss_group, squashed_rsample, squashed_rsample_group)
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    spec, _ = synthetic_spec(scenario=1, operation="OP1", eps_len_d=32)
    lines, lost = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    N = 8
    eng = HipEngine(spec.consts, spec.tables, spec.markets, N, device=0, out_dtype="float32", obs_layout="sb3_flat")
    eng.set_episode_plan(spec.eps_ind, N, N)
    L, h = eng._L, eng._h
    say(f"# tools/offpolicy_group_cost.py: float32; {args.reps} repetitions after {args.warmup} warm-up, routes taking turns, the first one rotating; "
        f"[us]: median [min - max]")
    say(f"# torch {torch.__version__}; {torch.cuda.get_device_name(0)}; library {os.environ.get('PTG_LIB_PATH', 'in-tree default')}; "
        f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', 'unset')}")
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)
    f64 = lambda x: torch.tensor([x], dtype=torch.float64, device=dev)

    def take_turns(routes):
        """device time of every route and the host's time to enqueue it, the first route rotating"""
        names = list(routes)
        t, host = {r: [] for r in names}, {r: [] for r in names}

        def clocked(r):
            def f():
                t0 = time.perf_counter()
                routes[r]()
                host[r].append((time.perf_counter() - t0) * 1e6)
            return f
        for rep in range(args.warmup + args.reps):
            for r in names[rep % len(names):] + names[:rep % len(names)]:
                dt = cost_timing.timed(clocked(r))[0]
                if rep >= args.warmup:
                    t[r].append(dt)
        return t, {r: statistics.median(v[-args.reps:]) for r, v in host.items()}

    def row(section, shape, G, launches, t, host=None, a="group", b="singles"):
        ma, mb = statistics.median(t[a]), statistics.median(t[b])
        held = ma <= mb
        note = ""
        if host is not None and max(host.values()) > DELAY_US:
            note = f"   host-bound (host enqueues in {host[a]:.0f} / {host[b]:.0f} us)"
        say(f"{section:>3s} {shape:>34s} {G:2d} {launches:>16s}  {stats(t[a]):>28s}  {stats(t[b]):>28s} {mb / ma:8.2f}   {'held' if held else 'MISSED'}{note}")
        if not held:
            lost.append(f"{section} {shape} G={G} ({ma:.1f} vs {mb:.1f} us)")

    def finish():
        say("# condition (every shape of (a) and (b)): the grouped route's median is not above the parent route's median -- " +
            ("held at every shape" if not lost else "MISSED at " + "; ".join(lost)))
        say("# not measured: float64, TQC's actor loss, G agents as G processes, the kernels under a profiler.")
        eng.close()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    say(f"{'':>3s} {'shape':>34s} {'G':>2s} {'launches grp/sgl':>16s}  {'grouped':>28s}  {'G single calls in turn':>28s} {'sgl/grp':>8s}   condition")

    # ------------------------------------------------------------------ (a) op by op: descriptors built once, raw calls
    def cols(B, K):
        return [rn(B) for _ in range(K)]

    def td_desc(kind, B, i):
        if kind == "dqn":
            kw = dict(q=rn(B, 5), next_q=rn(B, 5), actions=torch.randint(0, 5, (B,), device=dev, generator=g))
            out = (torch.empty(8, dtype=torch.float64, device=dev), torch.empty(B, 5, device=dev), None)
        else:
            kw = dict(q=cols(B, 2), next_q=cols(B, 2))
            out = (torch.empty(8, dtype=torch.float64, device=dev), [torch.empty(B, device=dev) for _ in range(2)], None)
            if kind == "sac":
                kw.update(next_log_prob=rn(B), log_ent_coef=f64(-1.0 - 0.1 * i))
        kw.update(rewards=rn(B), dones=(torch.rand(B, device=dev, generator=g) < 0.1).float())
        d, _, ws = eng._td_loss_member("cost", kind, gamma=0.95 + 0.005 * i, out=out, workspace=eng.td_loss_workspace(B), **kw)[1]()
        return d, (kw, out, ws)                              # the descriptor holds addresses: its tensors travel with it

    def al_desc(kind, B, i):
        kw, gq = {}, None
        if kind == "sac":
            kw, gq = dict(q=cols(B, 2), log_prob=rn(B), ent_coef=0.1 + 0.02 * i), [torch.empty(B, device=dev) for _ in range(2)]
        elif kind == "td3":
            kw, gq = dict(q=rn(B)), torch.empty(B, device=dev)
        else:
            kw = dict(log_prob=rn(B), log_ent_coef=f64(-1.0 - 0.1 * i), target_entropy=-1.0)
        out = (torch.empty(8, dtype=torch.float64, device=dev), gq, torch.empty(B, device=dev) if kind == "sac" else None,
               torch.empty(1, dtype=torch.float64, device=dev) if kind == "ent_coef" else None)
        d, _, ws = eng._actor_loss_member("cost", kind, out=out, workspace=eng.actor_loss_workspace(B), **kw)[1]()
        return d, (kw, out, ws)

    def rs_desc(what, B, i):
        if what == "smooth":
            mean, counter, out = rn(B, 1).tanh(), eng.new_draw_counter(), torch.empty(B, 1, device=dev)
            return eng._smooth_member("cost", mean, counter, 0.2, 0.5, seed=i, out=out)[1]()[0], (mean, counter, out)
        ml = rn(B, 2)
        if what == "fwd":
            counter, out = eng.new_draw_counter(), (torch.empty(B, 1, device=dev), torch.empty(B, 1, device=dev), torch.empty(B, 1, dtype=torch.float64, device=dev))
            return eng._rsample_member("cost", ml[:, :1], ml[:, 1:], counter, seed=i, out=out)[1]()[0], (ml, counter, out)
        noise, ga, gl, out = torch.randn(B, 1, dtype=torch.float64, device=dev, generator=g), rn(B, 1), rn(B, 1), (torch.empty(B, 1, device=dev), torch.empty(B, 1, device=dev))
        return eng._rsample_backward_member("cost", ml[:, :1], ml[:, 1:], noise, ga, gl, out=out)[1]()[0], (ml, noise, ga, gl, out)

    ops = [("td", "sac", 470, "TD loss SAC B=470 K=2", 2), ("td", "td3", 257, "TD loss TD3 B=257 K=2", 2), ("td", "dqn", 544, "TD loss DQN B=544 A=5", 2),
           ("al", "sac", 470, "actor loss SAC B=470 K=2", 2), ("al", "ent_coef", 470, "ent-coef loss B=470", 2), ("al", "td3", 257, "actor loss TD3 B=257", 2),
           ("rs", "fwd", 470, "rsample B=470", 2), ("rs", "bwd", 470, "rsample_backward B=470", 1), ("rs", "smooth", 257, "smoothing B=257", 2)]
    entry = {"td": ("ptg_td_loss", _lib.PtgTd), "al": ("ptg_actor_loss", _lib.PtgAl), "rs": ("ptg_rsample", _lib.PtgRs)}
    for op, kind, B, label, launches in ops if "a" in args.sections else ():
        name, T = entry[op]
        if (op, kind) == ("rs", "bwd"):
            name = "ptg_rsample_backward"
        make = {"td": td_desc, "al": al_desc, "rs": rs_desc}[op]
        single, group = getattr(L, name), getattr(L, name + "_group")
        for G in (2, 4, 6, 8):
            made = {r: [make(kind, B, i) for i in range(G)] for r in ("group", "singles")}       # one set of tensors per route: neither leg warms the other's
            arr = (T * G)(*[d for d, _ in made["group"]])
            ds = [d for d, _ in made["singles"]]
            stream = eng._stream()

            def grouped():
                assert group(h, arr, G, stream) == 0

            def singles():
                for d in ds:
                    assert single(h, C.byref(d), stream) == 0
            with torch.cuda.device(dev):
                t, host = take_turns({"group": grouped, "singles": singles})
            eng.sync()
            row("(a)", label, G, f"{launches} / {G * launches}", t, host)
            del made, arr, ds

    # ------------------------------------------------------------------ (b) the captured SAC step of four agents
    G, B, F, W, D = 4, 470, eng.obs_dim, 233, 6
    lr, gamma, tau, H_t = [3e-4, 1e-4, 5e-4, 2e-4], [0.96, 0.97, 0.98, 0.95], 0.005, -1.0

    def mlp(seed, fan_in, out):
        torch.manual_seed(seed)
        layers, k = [], fan_in
        for _ in range(D):
            layers += [nn.Linear(k, W), nn.Tanh()]
            k = W
        return nn.Sequential(*layers, nn.Linear(W, out)).to(dev)

    def optimizer(params, **kw):
        for p in params:
            p.grad = torch.zeros_like(p)
        return DeviceOptimizer(eng, params, kind="adam", zero_grad=True, **kw)

    def set_grads(params, grads):
        for p, x in zip(params, grads):
            p.grad.copy_(x)

    class Agent:
        def __init__(self, i):
            self.i = i
            self.actor = mlp(50 + i, F, 2)
            with torch.no_grad():
                self.actor[-1].weight.mul_(0.1); self.actor[-1].bias[1] = -1.0
            self.critics, self.targets = [mlp(60 + 2 * i + k, F + 1, 1) for k in range(2)], [mlp(60 + 2 * i + k, F + 1, 1) for k in range(2)]
            self.log_alpha = torch.tensor([-1.0], dtype=torch.float64, device=dev, requires_grad=True)
            self.counter = eng.new_draw_counter()
            self.ap = list(self.actor.parameters())
            self.opt_a = optimizer(self.ap, lr=lr[i])
            self.opt_c = optimizer([p for m in self.critics for p in m.parameters()], lr=lr[i], targets=[p for m in self.targets for p in m.parameters()], tau=tau)
            self.opt_l = optimizer([self.log_alpha], lr=lr[i])
            self.batch = dict(obs=rn(B, F), next_obs=rn(B, F), actions=rn(B, 1).tanh(), rewards=rn(B), dones=(torch.rand(B, device=dev, generator=g) < 0.1).float())

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

    agents = [Agent(i) for i in range(G)]
    actors, actors_nograd = TrainMLPGroup(eng, [a.actor for a in agents], batch=B), DeviceMLPGroup(eng, [a.actor for a in agents], batch=B)
    critics = TrainMLPGroup(eng, [m for a in agents for m in a.critics], batch=B)
    targets = DeviceMLPGroup(eng, [m for a in agents for m in a.targets], batch=B)
    og_a, og_c, og_l = (DeviceOptimizerGroup(eng, [getattr(a, n) for a in agents]) for n in ("opt_a", "opt_c", "opt_l"))
    twice = lambda xs: [x for x in xs for _ in range(2)]

    def grouped_step():
        s = [a.batch for a in agents]
        ml = actors([b["obs"] for b in s])
        pi = squashed_rsample_group(eng, [dict(mean=o[:, :1], log_std=o[:, 1:], counter=a.counter) for o, a in zip(ml, agents)], seed=list(range(G)))
        els, el_stats = ent_coef_loss_group(eng, [dict(log_prob=lp, log_ent_coef=a.log_alpha) for (_, lp), a in zip(pi, agents)], target_entropy=H_t)
        alphas = [st[4:5] for st in el_stats]
        torch.autograd.backward(els)
        og_l.step()
        with torch.no_grad():
            nml = actors_nograd([b["next_obs"] for b in s])
            nxt = squashed_rsample_group(eng, [dict(mean=o[:, :1], log_std=o[:, 1:], counter=a.counter) for o, a in zip(nml, agents)], seed=list(range(G)))
            nq = targets(twice([b["next_obs"] for b in s]), x2=twice([na for na, _ in nxt]))
        q = critics(twice([b["obs"] for b in s]), x2=twice([b["actions"] for b in s]))
        closses, _ = sac_critic_loss_group(eng, [dict(q=list(q[2 * i:2 * i + 2]), next_q=list(nq[2 * i:2 * i + 2]), rewards=s[i]["rewards"], dones=s[i]["dones"],
                                                      next_log_prob=nxt[i][1], ent_coef=alphas[i]) for i in range(G)], gamma=gamma)
        torch.autograd.backward(closses)
        og_c.step()
        q_pi = critics(twice([b["obs"] for b in s]), x2=twice([a_pi for a_pi, _ in pi]))
        alosses, _ = sac_actor_loss_group(eng, [dict(q=list(q_pi[2 * i:2 * i + 2]), log_prob=pi[i][1], ent_coef=alphas[i]) for i in range(G)])
        all_ap = [p for a in agents for p in a.ap]
        set_grads(all_ap, torch.autograd.grad(alosses, all_ap))
        og_a.step()

    class Single:
        def __init__(self, i):
            a = self.a = Agent(i)
            self.actor, self.actor_nograd = TrainMLP(eng, a.actor, batch=B), DeviceMLPGroup(eng, [a.actor], batch=B)
            self.critics, self.targets = TrainMLPGroup(eng, a.critics, batch=B), DeviceMLPGroup(eng, a.targets, batch=B)

        def __call__(self):
            a, b, i = self.a, self.a.batch, self.a.i
            ml = self.actor(b["obs"])
            a_pi, lp = squashed_rsample(eng, ml[:, :1], ml[:, 1:], a.counter, seed=i)
            el, el_stats = ent_coef_loss(eng, lp, a.log_alpha, target_entropy=H_t)
            alpha = el_stats[4:5]
            el.backward()
            a.opt_l.step()
            with torch.no_grad():
                nml, = self.actor_nograd(b["next_obs"])
                na, nlp = squashed_rsample(eng, nml[:, :1], nml[:, 1:], a.counter, seed=i)
                nq = self.targets(b["next_obs"], x2=na)
            q = self.critics(b["obs"], x2=b["actions"])
            cl, _ = sac_critic_loss(eng, list(q), list(nq), b["rewards"], b["dones"], nlp, gamma=gamma[i], ent_coef=alpha)
            cl.backward()
            a.opt_c.step()
            q_pi = self.critics(b["obs"], x2=a_pi)
            al, _ = sac_actor_loss(eng, list(q_pi), lp, ent_coef=alpha)
            set_grads(a.ap, torch.autograd.grad(al, a.ap))
            a.opt_a.step()

    def finite(who, agent_list):
        """every parameter, target and log alpha of these agents finite?  (a timing of NaNs would be a timing of the early exits)"""
        bad = [a.i for a in agent_list if not all(bool(torch.isfinite(p).all()) for p in a.ap + a.opt_c.params + a.opt_c.targets + [a.log_alpha])]
        say(f"#       {who}: " + ("every parameter, target and log alpha finite" if not bad else f"NON-FINITE parameters in agents {bad}"))

    if "b" not in args.sections:
        return finish()
    from rl_ptg_amd.engine import PtgError
    raised = []

    def stage(what):
        """the handle's error words after `what`: a bad row anywhere is named with the stage that raised it, and the run goes on"""
        try:
            eng.sync()
        except PtgError as e:
            raised.append(what)
            say(f"#       ERROR WORD RAISED by {what}: code {e.code}")

    g_group = capture(grouped_step)
    stage("the grouped route's eager step")
    singles = [Single(i) for i in range(G)]                  # kept for as long as their graphs replay: a graph holds addresses, not tensors
    g_single = []
    for i, s in enumerate(singles):
        g_single.append(capture(s))
        stage(f"single agent {i}'s eager step")

    def in_turn():
        for gr in g_single:
            gr.replay()
    g_group.replay()
    stage("the grouped graph's first replay")
    in_turn()
    stage("the single graphs' first replay")
    routes = {"group": g_group.replay, "singles": in_turn}
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
    torch.cuda.synchronize()
    say(f"# (b) wall time per gradient step of all {G} agents [us], {args.replays} replays and one synchronisation per repetition")
    row("(b)", f"SAC step {D}x{W} Tanh B={B}", G, "1 graph / 4", t)
    stage("the timed replays (either route)")
    steps = 2 + (args.warmup + args.reps) * args.replays
    finite(f"after {steps} gradient steps on one batch, grouped", agents)
    finite(f"after {steps} gradient steps on one batch, singles", [s.a for s in singles])
    say("#       error words of the handle over (b): " + ("none raised" if not raised else "RAISED by " + "; ".join(raised)))
    finish()


if __name__ == "__main__":
    main()
