"""python tools/rollout_buffer_cost.py [--mode add|collect] [--reps 15] [--warmup 3] [--label TEXT]

What the on-policy store costs on the device, measured in one process, the variants alternating from one repetition to the next.

How add advances the cursor is fixed when csrc/ptg_train.hip is compiled (-DPTG_RO_FORM): 0, the library that ships, is the copy
kernel and a one-thread cursor kernel behind it (DeviceReplayBuffer's form); 1 and 2 are measurement builds in which add is ONE
kernel and the workgroup that draws the last ticket advances the cursor, with (1) or without (2) a __threadfence before every
ticket.  The tool times the library it loads; to compare the forms, build ptg_train.hip with the other values, link each beside the
tree's other objects and run the same command once per library through PTG_LIB_PATH, with --label naming the build in the output.

--mode add (default): one DeviceRolloutBuffer.add = ptg_rollout_buffer_add of a step()'s outputs with five columns
(int64 actions, float32 values read at stride 6 from a joint network output, float32 log-probs, float32 rewards, uint8 dones: 21
bytes per env) at N = 6, 4 096 and 65 536 envs, float32 SB3_FLAT rows (F = 40) and SPLIT rows (F = 16), against
  torch   the route it replaces: obs_rows[t + 1].copy_(obs) plus one copy_ per column with a HOST t -- six launches, and not
          replayable, since a captured copy_ keeps its row
  copy    one copy_ of the same number of bytes between two flat buffers: the floor of a single launch
Compulsory bytes per add: 2 * (N * F * 4 + 21 * N), every byte read once and written once.  GB/s = those bytes / the median time.

--mode collect: the captured collect step -- DeviceMLP F -> 64 -> 64 -> 6 (tanh), act_categorical, replay-proof step() -- at 4 096 and
65 536 envs (SB3_FLAT), one graph without storage and one with add() behind the step, replayed in turns; the difference of the
medians is what storing costs inside the step.

Every timed section is queued behind a ~100 us device-side delay (tools/cost_timing.py), so the host has enqueued its work before
the first event is reached.  Medians with min and max over --reps repetitions after --warmup unrecorded ones."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cost_timing import alternate, stats, timed  # noqa: E402

ADD_SHAPES = [(6, "sb3_flat"), (6, "split"), (4096, "sb3_flat"), (4096, "split"), (65536, "sb3_flat"), (65536, "split")]
COLLECT_SHAPES = [4096, 65536]
COL_BYTES = 8 + 4 + 4 + 4 + 1


def _engine(spec, n, layout):
    from rl_ptg_amd.engine import HipEngine
    eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout=layout)
    eng.set_episode_plan(spec.eps_ind, n, n)
    eng.set_noise_rng(11)
    eng.set_replay_proof(True)
    eng.reset()
    return eng


def mode_add(args, spec):
    import torch
    from rl_ptg_amd import DeviceRolloutBuffer
    dev = torch.device("cuda", 0)
    T = args.warmup + args.reps
    print(f"{'N':>6s} {'layout':>8s} {'F':>3s}  {'add':>29s}  {'torch route (6 launches)':>29s}  {'one copy_':>29s}  {'bytes':>10s} {'GB/s':>7s} {'torch/add':>9s}")
    for n, layout in ADD_SHAPES:
        eng = _engine(spec, n, layout)
        F = eng.obs_dim
        buf, twin = DeviceRolloutBuffer(eng, T), DeviceRolloutBuffer(eng, T)
        g = torch.Generator(device="cuda")
        g.manual_seed(n)
        acts = torch.randint(0, 5, (n,), dtype=torch.int64, device=dev, generator=g)
        out = torch.randn((n, 6), device=dev, generator=g)
        logp = torch.randn((n,), device=dev, generator=g)
        obs, rew, done = eng.step(acts.int())
        nbytes = n * F * 4 + COL_BYTES * n
        flat_a, flat_b = torch.zeros(nbytes, dtype=torch.uint8, device=dev), torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        st = twin.storage
        srcs = [acts, out[:, 5], logp, rew, done]
        host_t = [0]

        def torch_route():
            t = host_t[0]
            st.obs_rows[t + 1].copy_(obs)
            for ring, x in zip(st.col_rows, srcs):
                ring[t].copy_(x)
            host_t[0] = t + 1

        buf.begin(); twin.begin()
        ta, tt, tc = [], [], []
        for rep in range(T):
            a = timed(lambda: buf.add(obs, rew, done, actions=acts, values=out[:, 5], log_probs=logp))[0]
            b = timed(torch_route)[0]
            c = timed(lambda: flat_b.copy_(flat_a))[0]
            if rep >= args.warmup:
                ta.append(a); tt.append(b); tc.append(c)
        eng.sync()
        same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip([buf.storage.obs_rows] + buf.storage.col_rows, [st.obs_rows] + st.col_rows))
        assert same and buf.cursor() == (T, 0), "the torch route and ptg_rollout_buffer_add disagree"
        med = statistics.median(ta)
        print(f"{n:6d} {layout:>8s} {F:3d}  {stats(ta):>29s}  {stats(tt):>29s}  {stats(tc):>29s}  {2 * nbytes:10d} {2 * nbytes / (med * 1e-6) / 1e9:7.1f} "
              f"{statistics.median(tt) / med:9.2f}   # storage byte-equal: {same}; add <= torch route: {med <= statistics.median(tt)}")
        eng.close()
        del buf, twin, st, flat_a, flat_b
        torch.cuda.empty_cache()


def mode_collect(args, spec):
    import torch
    from torch import nn
    from rl_ptg_amd import DeviceMLP, DeviceRolloutBuffer
    T = args.warmup + args.reps + 2
    print(f"{'N':>6s}  {'step without storage':>29s}  {'step with add':>29s}  {'difference of medians':>21s}")
    for n in COLLECT_SHAPES:
        eng = _engine(spec, n, "sb3_flat")
        torch.manual_seed(1)
        pi = nn.Sequential(nn.Linear(eng.obs_dim, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 6)).cuda()
        policy = DeviceMLP(eng, pi, batch=n)
        counter = eng.new_draw_counter()
        buf = DeviceRolloutBuffer(eng, T)
        head = eng.act_categorical(policy(eng.obs)[:, :5], counter, seed=2, act_dtype=torch.int64)

        def step(store):
            out = policy(eng.obs)
            eng.act_categorical(out[:, :5], counter, seed=2, out=head)
            eng.step(head.actions)
            if store:
                buf.add(eng.obs, eng.rew, eng.done, actions=head.actions, values=out[:, 5], log_probs=head.log_prob)

        buf.begin()
        graphs = []
        side = torch.cuda.Stream()
        for store in (False, True):
            step(store)                                     # eager once: code objects are loaded before the capture
            eng.sync()
            side.wait_stream(torch.cuda.current_stream())
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(gr, stream=side):
                    step(store)
            torch.cuda.current_stream().wait_stream(side)
            graphs.append(gr)
        t0, t1 = alternate(graphs[0].replay, graphs[1].replay, args.warmup, args.reps)
        eng.note_replays(2 * (args.warmup + args.reps) - 2)
        eng.sync()
        assert buf.cursor() == (1 + args.warmup + args.reps, 0), buf.cursor()
        print(f"{n:6d}  {stats(t0):>29s}  {stats(t1):>29s}  {statistics.median(t1) - statistics.median(t0):21.1f}")
        eng.close()
        del buf, graphs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("add", "collect"), default="add")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="the tree's library: copy kernel + cursor kernel (PTG_RO_FORM 0)")
    args = ap.parse_args()
    import torch
    from rl_ptg_amd.prep import synthetic_spec
    torch.cuda.set_device(0)
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=32)          # 4 608-step episodes: no boundary inside the measurement
    print(f"# tools/rollout_buffer_cost.py --mode {args.mode}: {args.reps} repetitions after {args.warmup} warm-up, variants alternating; "
          f"device time from HIP events [us]: median [min - max]")
    print(f"# torch {torch.__version__}; {torch.cuda.get_device_name(0)}; build: {args.label}")
    (mode_add if args.mode == "add" else mode_collect)(args, spec)


if __name__ == "__main__":
    main()
