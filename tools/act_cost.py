"""python tools/act_cost.py [--reps 15] [--warmup 3]

What the action head costs on the device while collecting: float32, A = 5 (the reference's discrete action space), N in {6, 4 096,
65 536}, measured in one process, the two routes alternating from one repetition to the next on the same tensors:

  ptg_act  HipEngine.act_categorical / act_eps_greedy / act_gaussian into preallocated outputs: one kernel + the counter kernel
  torch    the eager route a caller writes today:
             categorical  d = torch.distributions.Categorical(logits=x); a = d.sample(); d.log_prob(a); d.entropy()
             eps-greedy   torch.where(torch.rand(N) < eps, torch.randint(0, A, (N,)), x.argmax(1))
             gaussian     d = Normal(mean, log_std.exp()); g = d.rsample(); g.clamp(-1, 1); d.log_prob(g)

and the captured collect step of tools/policy_loop.py's shape (sb3_flat rows -> 40 -> 64 -> 64 -> 5 tanh MLP -> SAMPLED action ->
ptg_step on a replay-proof engine, one hipGraph per step), once with the torch categorical head and once with act_categorical.

Every timed section is queued behind a ~100 us device-side delay, so the host has enqueued its work before the first event is
reached: the events bracket device work only -- for the launch-bound torch routes the device then waits for the host inside the
interval, which is that route's cost.  Medians with min and max over --reps repetitions after --warmup unrecorded ones.
Compulsory bytes of the categorical head at float32, A = 5, int32 actions and both float outputs: 20 read + 12 written per env --
2 MB at N = 65 536; the launch is bound by its own latency at every one of these batches, so no bandwidth fraction is stated: the
floor is one short launch between two events (6-7 us, profiles/minibatch_cost.txt) plus the counter kernel behind it."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cost_timing  # noqa: E402

NS = [6, 4096, 65536]
A = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from torch.distributions import Categorical, Normal
    from rl_ptg_amd import dist as ptg_dist
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    spec, _ = synthetic_spec(scenario=1, operation="OP1", eps_len_d=32)          # tools/policy_loop.py's engine

    stats = lambda v: cost_timing.stats(v, width=8)
    alternate = lambda fa, fb: cost_timing.alternate(fa, fb, args.warmup, args.reps)

    def engine(n):
        eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
        first_ptr, stride = ptg_dist.episode_plan(n, 1, 0)
        eng.set_episode_plan(spec.eps_ind, first_ptr, stride)
        eng.set_noise_rng(seed=20250614)
        return eng

    print(f"# tools/act_cost.py: float32, A = {A}, int32 actions; {args.reps} repetitions after {args.warmup} warm-up, routes alternating; "
          f"device time from HIP events [us]: median [min - max]")
    print(f"# torch {torch.__version__}; {torch.cuda.get_device_name(0)}; library {os.environ.get('PTG_LIB_PATH', 'in-tree default')}")
    print(f"{'head':>12s} {'N':>6s}  {'ptg_act':>26s}  {'torch route':>26s} {'torch/ptg_act':>13s}")
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    for n in NS:
        eng = engine(n)
        x = torch.randn((n, A), device=dev, generator=g) * 3
        mean, ls = torch.randn(n, device=dev, generator=g) * 0.5, torch.full((1,), -1.0, device=dev)
        eps = torch.full((1,), 0.1, dtype=torch.float64, device=dev)
        eps32 = 0.1
        cnt = eng.new_draw_counter()
        rc, re_, rg = eng.act_categorical(x, cnt), eng.act_eps_greedy(x, eps, cnt), eng.act_gaussian(mean, ls, cnt, want_entropy=False)

        def t_cat():
            d = Categorical(logits=x, validate_args=False)
            a = d.sample()
            return a, d.log_prob(a), d.entropy()

        def t_eps():
            return torch.where(torch.rand(n, device=dev) < eps32, torch.randint(0, A, (n,), device=dev), x.argmax(dim=1))

        def t_gau():
            d = Normal(mean, ls.exp(), validate_args=False)
            s = d.rsample()
            return s.clamp(-1.0, 1.0), d.log_prob(s)

        for name, fk, ft in (("categorical", lambda: eng.act_categorical(x, cnt, out=rc), t_cat),
                             ("eps-greedy", lambda: eng.act_eps_greedy(x, eps, cnt, out=re_), t_eps),
                             ("gaussian", lambda: eng.act_gaussian(mean, ls, cnt, out=rg, want_entropy=False), t_gau)):
            tk, tt = alternate(fk, ft)
            print(f"{name:>12s} {n:6d}  {stats(tk):>26s}  {stats(tt):>26s} {statistics.median(tt) / statistics.median(tk):13.2f}")
        eng.sync()
        # the kernel's draw is a distribution, not torch's bit stream: compare the action frequencies of one row's worth of envs
        if n == 65536:
            p = torch.softmax(x.double(), 1).mean(0).cpu()
            f = torch.bincount(rc.actions.long(), minlength=A).double().cpu() / n
            print(f"# N = {n}: mean action probabilities {[round(v, 4) for v in p.tolist()]}, ptg_act frequencies {[round(v, 4) for v in f.tolist()]}")
        eng.close()

    print(f"{'collect step':>12s} {'N':>6s}  {'graph with act_categorical':>26s}  {'graph with torch head':>26s} {'torch/ptg_act':>13s}")
    torch.manual_seed(0)
    l1, l2, l3 = torch.nn.Linear(40, 64).to(dev), torch.nn.Linear(64, 64).to(dev), torch.nn.Linear(64, 5).to(dev)
    for n in (6, 65536):
        graphs, engs = [], []
        for route in ("ptg_act", "torch"):
            eng = engine(n)
            eng.set_replay_proof(True)
            obs = eng.reset()
            a_static = torch.zeros(n, dtype=torch.int32, device=dev)
            lp_static, en_static = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
            cnt = eng.new_draw_counter()
            out = eng.act_categorical(torch.zeros((n, A), device=dev), None, deterministic=True)

            def body(eng=eng, obs=obs, route=route, out=out, cnt=cnt, a_static=a_static, lp_static=lp_static, en_static=en_static):
                logits = l3(torch.tanh(l2(torch.tanh(l1(obs)))))
                if route == "ptg_act":
                    eng.act_categorical(logits, cnt, out=out)
                    eng.step(out.actions, want_final=False)
                else:
                    d = Categorical(logits=logits, validate_args=False)
                    a = d.sample()
                    lp_static.copy_(d.log_prob(a)); en_static.copy_(d.entropy()); a_static.copy_(a)
                    eng.step(a_static, want_final=False)

            with torch.no_grad():
                for _ in range(3):
                    body()                                    # (torch wants the ops warm before a capture)
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.stream(side):
                    with torch.cuda.graph(gr, stream=side):
                        body()
                torch.cuda.current_stream().wait_stream(side)
            graphs.append(gr); engs.append(eng)
        tk, tt = alternate(graphs[0].replay, graphs[1].replay)
        for eng in engs:
            eng.note_replays(args.warmup + args.reps - 1)
            eng.sync()
            eng.close()
        print(f"{'collect step':>12s} {n:6d}  {stats(tk):>26s}  {stats(tt):>26s} {statistics.median(tt) / statistics.median(tk):13.2f}")
    print("# not measured: float64 inputs, A other than 5, int64 actions, strided (sliced) inputs, the squashed Gaussian, the kernels under a profiler,")
    print("# the eager (uncaptured) collect step, N between 6 and 4 096.")


if __name__ == "__main__":
    main()
