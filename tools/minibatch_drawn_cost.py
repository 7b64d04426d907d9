"""python tools/minibatch_drawn_cost.py [--reps 15] [--warmup 3]

What it costs to draw a PPO / A2C minibatch's indices inside the gather (HipEngine.minibatch_drawn = ptg_minibatch_drawn: the gather and
the one-thread cursor kernel behind it) instead of reading them from a permutation in memory (HipEngine.minibatch = ptg_minibatch), in
one process, the routes alternating from one repetition to the next, medians with min and max over --reps repetitions after --warmup
unrecorded ones.  Buffers as in tools/minibatch_cost.py: float32 SB3_FLAT rows (F = 40, 160 bytes), five float32 columns and int32
actions, every output preallocated.

(a) per batch, device time from HIP events behind a ~100 us device-side delay, at the four shapes of profiles/minibatch_cost.txt --
    T = 609 = 3 * 203 in place of 658 at the two shapes with B = 203, because the drawn route takes only a batch that divides T * N:
      idx     minibatch() on a ready int64 idx slice of a torch.randperm(T * N): the parent's route, ONE launch
      drawn   minibatch_drawn(): TWO launches, the gather and the cursor kernel
(b) per epoch, device time from HIP events behind the same delay (a launch-bound route makes the device wait for the host inside the
    interval, which is that route's cost):
      idx     torch.randperm(T * N) and the T * N / B gathers on its slices
      drawn   the T * N / B drawn gathers alone
(c) one epoch of PPO gradient steps at the reference's shape -- policy 40 -> 358 -> 358 -> 5 and value 40 -> 358 -> 358 -> 1 in one
    TrainMLPGroup, B = 203, 21 batches of a 4263 x 1 window, Adam with grad-norm clipping -- wall time with ONE synchronisation at the end:
      eager   for mb in rollout.get(203): forward -> ppo_loss -> backward() -> DeviceOptimizer.step()       (the parent's route)
      replay  21 replays of ONE captured graph of next_batch -> the same step
    Both routes take the same number of steps from the same start; their parameters are not compared here (tests/test_minibatch_drawn.py
    does that bit for bit under one order)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cost_timing import stats, timed  # noqa: E402

SHAPES = [(609, 6, 203), (609, 4096, 203), (20, 65536, 65536), (658, 65536, 65536)]
EPOCH_SHAPES = [(4263, 6, 203), (20, 65536, 65536), (658, 65536, 65536)]


def _engine(n):
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=32)          # 4 608-step episodes: no boundary inside a window
    eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
    eng.set_episode_plan(spec.eps_ind, n, n)
    eng.set_noise_rng(11)
    eng.reset()
    return eng


def _window(eng, T, g):
    import torch
    n = eng.n
    acts = torch.randint(0, 5, (T, n), dtype=torch.int32, device="cuda", generator=g)
    obs = eng.alloc_obs(T)
    rew, done = torch.empty((T, n), device="cuda"), torch.empty((T, n), dtype=torch.uint8, device="cuda")
    for a in range(0, T, 512):                               # 4 608-step episodes: a window of 4 263 steps stays inside one
        b = min(a + 512, T)
        eng.rollout(acts[a:b], obs[a:b], rew[a:b], done[a:b])
    cols = [torch.randn((T, n), dtype=torch.float32, device="cuda", generator=g) for _ in range(4)] + [rew, acts]
    return obs, cols


def per_batch(args):
    import torch
    print("# (a) per batch; device time from HIP events [us]: median [min - max]")
    print(f"{'T':>4s} {'N':>6s} {'B':>6s}  {'idx (1 launch)':>26s}  {'drawn (2 launches)':>26s}  {'drawn/idx':>9s}  within idx's [min - max]")
    for T, n, B in SHAPES:
        eng = _engine(n)
        F = eng.obs_dim
        g = torch.Generator(device="cuda"); g.manual_seed(T + n)
        obs, cols = _window(eng, T, g)
        idx = torch.randperm(T * n, device="cuda", generator=g)[:B].contiguous()
        cur = eng.new_epoch_cursor()
        out = torch.empty((B, F), dtype=torch.float32, device="cuda")
        outs = [torch.empty((B,), dtype=c.dtype, device="cuda") for c in cols]
        ti, td = [], []
        for rep in range(args.warmup + args.reps):
            a, _ = timed(lambda: eng.minibatch(idx, obs, cols, obs_out=out, columns_out=outs))
            b, _ = timed(lambda: eng.minibatch_drawn(cur, B, obs, cols, seed=7, obs_out=out, columns_out=outs))
            if rep >= args.warmup:
                ti.append(a); td.append(b)
        eng.sync()
        mi, md_ = statistics.median(ti), statistics.median(td)
        verdict = "yes" if min(ti) <= md_ <= max(ti) else ("below it" if md_ < min(ti) else "NO: %+.1f us past it" % (md_ - max(ti)))
        print(f"{T:4d} {n:6d} {B:6d}  {stats(ti):>26s}  {stats(td):>26s}  {md_ / mi:9.2f}  {verdict}")
        eng.close()
        del obs, cols, out, outs
        torch.cuda.empty_cache()


def per_epoch(args):
    import torch
    print("# (b) per epoch; device time from HIP events [us]: median [min - max]")
    print(f"{'T':>4s} {'N':>6s} {'B':>6s} {'batches':>7s}  {'randperm + idx gathers':>30s}  {'drawn gathers':>30s}  {'idx/drawn':>9s}")
    for T, n, B in EPOCH_SHAPES:
        eng = _engine(n)
        F = eng.obs_dim
        g = torch.Generator(device="cuda"); g.manual_seed(T + n)
        obs, cols = _window(eng, T, g)
        TN = T * n
        cur = eng.new_epoch_cursor()
        out = torch.empty((B, F), dtype=torch.float32, device="cuda")
        outs = [torch.empty((B,), dtype=c.dtype, device="cuda") for c in cols]

        def by_idx():
            perm = torch.randperm(TN, device="cuda")
            for s in range(0, TN, B):
                eng.minibatch(perm[s:s + B], obs, cols, obs_out=out, columns_out=outs)

        def drawn():
            for _ in range(TN // B):
                eng.minibatch_drawn(cur, B, obs, cols, seed=7, obs_out=out, columns_out=outs)

        ti, td = [], []
        for rep in range(args.warmup + args.reps):
            a, _ = timed(by_idx)
            b, _ = timed(drawn)
            if rep >= args.warmup:
                ti.append(a); td.append(b)
        eng.sync()
        print(f"{T:4d} {n:6d} {B:6d} {TN // B:7d}  {stats(ti, 11):>30s}  {stats(td, 11):>30s}  {statistics.median(ti) / statistics.median(td):9.2f}")
        eng.close()
        del obs, cols, out, outs
        torch.cuda.empty_cache()


def ppo_epoch(args):
    import torch
    from torch import nn
    from rl_ptg_amd import DeviceOptimizer, DeviceRolloutBuffer, TrainMLPGroup, ppo_loss
    T, N, B, F, A, W = 4263, 1, 203, 40, 5, 358
    eng = _engine(N)
    buf = DeviceRolloutBuffer(eng, T, seed=7)
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    buf.begin()
    for t in range(T):
        act = torch.randint(0, A, (N,), dtype=torch.int64, device="cuda", generator=g)
        obs, rew, done = eng.step(act)
        buf.add(obs, rew, done, actions=act, values=0.1 * torch.randn(N, device="cuda", generator=g), log_probs=-1.6 + 0.1 * torch.randn(N, device="cuda", generator=g))
    buf.compute_returns_and_advantage(torch.zeros(N, device="cuda"), 0.99, 0.95)
    eng.sync()

    class Step:
        def __init__(self):
            torch.manual_seed(3)
            pi = nn.Sequential(nn.Linear(F, W), nn.Tanh(), nn.Linear(W, W), nn.Tanh(), nn.Linear(W, A)).cuda()
            vf = nn.Sequential(nn.Linear(F, W), nn.Tanh(), nn.Linear(W, W), nn.Tanh(), nn.Linear(W, 1)).cuda()
            self.grp = TrainMLPGroup(eng, [pi, vf], batch=B)
            for p in self.grp.parameters():
                p.grad = torch.zeros_like(p)
            self.opt = DeviceOptimizer(eng, self.grp.parameters(), kind="adam", lr=1e-5, eps=1e-5, max_grad_norm=0.5, zero_grad=True)
            self.ws = eng.policy_loss_workspace(B)
            self.samples = None

        def __call__(self, mb):
            logits, values = self.grp(mb.observations)
            loss, _ = ppo_loss(eng, logits, values, mb.actions, mb.old_log_prob, mb.advantages, mb.returns, clip_range=0.2, ent_coef=0.01, workspace=self.ws)
            loss.backward()
            self.opt.step()

        def drawn(self):
            self.samples = buf.next_batch(B, out=self.samples)
            self(self.samples)

    eager, cap = Step(), Step()
    cap.drawn()                                              # eager once: code objects loaded, the optimiser's tables built
    buf.end_epoch()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            cap.drawn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    per = T * N // B

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    def eager_epoch():
        for mb in buf.get(B):
            eager(mb)

    def replay_epoch():
        for _ in range(per):
            graph.replay()

    te, tr = [], []
    for rep in range(args.warmup + args.reps):
        a, b = wall(eager_epoch), wall(replay_epoch)
        if rep >= args.warmup:
            te.append(a); tr.append(b)
    eng.sync()
    assert buf.epoch_cursor()[1] == 0
    print(f"# (c) one epoch of PPO gradient steps: two 2 x {W} nets, B = {B}, {per} batches; wall time with one synchronisation at the end [us]: median [min - max]")
    print(f"eager loop over get()       {stats(te, 11)}   per step {statistics.median(te) / per:8.1f}")
    print(f"replayed graph of the step  {stats(tr, 11)}   per step {statistics.median(tr) / per:8.1f}")
    print(f"eager / replay              {statistics.median(te) / statistics.median(tr):.2f}")
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parts", default="abc")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    print(f"# tools/minibatch_drawn_cost.py: float32 SB3_FLAT rows (160 B), 5 float32 columns + int32 actions; {args.reps} repetitions after "
          f"{args.warmup} warm-up, routes alternating")
    print(f"# torch {torch.__version__}; {torch.cuda.get_device_name(0)}")
    if "a" in args.parts:
        per_batch(args)
    if "b" in args.parts:
        per_epoch(args)
    if "c" in args.parts:
        ppo_epoch(args)


if __name__ == "__main__":
    main()
