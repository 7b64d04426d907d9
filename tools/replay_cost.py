"""python tools/replay_cost.py [--reps 15] [--warmup 3]

What the off-policy store and draw cost on the device: float32 SB3_FLAT rows (F = 40, 160 bytes), int32 actions, float32 rewards
and float32 dones, in a DeviceReplayBuffer of 1 000 000 transitions (N = 6: 166 666 rows) or 64 rows (N = 65 536: 4.2 M
transitions, 1.3 GB of rings), measured in one process, the variants alternating from one repetition to the next:

  add     DeviceReplayBuffer.add of a T-step window (T = 1: a step()'s outputs, T = 20: a rollout()'s) with final_obs
          = ptg_replay_add, one kernel + the cursor kernel                                  HIP events around the call
  torch   the same store with eager torch on the same tensors: slots = (cursor + arange(T)) % S, index_copy_ into both
          observation rings (torch.where on the done rows for the next observation) and the three columns, cursor += T
  sample  DeviceReplayBuffer.sample(B), indices drawn on the device = ptg_replay_sample, one kernel + the cursor kernel, at the
          batch sizes of the reference's config_agent.yaml (DQN 544, SAC 257, TD3 470, TQC 290) and at 65 536 rows
  torch   torch.randint(0, size * N, (B,)) and advanced indexing of the flattened rings and columns (six launches), eager

Every timed section is queued behind a ~100 us device-side delay, so the host has enqueued its work before the first event is
reached: the events bracket device work only -- for the launch-bound torch routes the device then waits for the host inside the
interval, which is that route's cost.  Medians with min and max over --reps repetitions after --warmup unrecorded ones.
Compulsory bytes of an add: every window row read once and written to two rings (3 * F * 4 per transition), the first step's
previous observation (N * F * 4), 9 bytes of columns read and 12 written per transition; of a sample: 2 * F * 4 read and written
plus 12 + 12 of columns per row.  Fraction of the HBM peak = those bytes / the median time / 8 TB/s."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cost_timing import stats, timed  # noqa: E402

ADD_SHAPES = [(6, 1), (6, 20), (65536, 1), (65536, 20)]      # (N, T)
SAMPLE_SHAPES = [(6, 544), (6, 257), (6, 470), (6, 290), (6, 65536), (65536, 544), (65536, 65536)]      # (N, B)
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from rl_ptg_amd import DeviceReplayBuffer
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=32)          # 4 608-step episodes: no boundary inside a window

    print(f"# tools/replay_cost.py: float32 SB3_FLAT rows (160 B), int32 actions, float32 rewards and dones; {args.reps} repetitions after "
          f"{args.warmup} warm-up, variants alternating; device time from HIP events [us]: median [min - max]")
    print(f"# torch {torch.__version__}; {torch.cuda.get_device_name(0)}")
    made = {}

    def setup(n):
        if n in made:
            return made[n]
        made.clear()
        torch.cuda.empty_cache()
        eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
        eng.set_episode_plan(spec.eps_ind, n, n)
        eng.set_noise_rng(11)
        prev = eng.reset().clone()
        buf = DeviceReplayBuffer(eng, 1000000 if n == 6 else 64 * n, columns={"actions": torch.int32}, seed=3)
        twin = DeviceReplayBuffer(eng, 1000000 if n == 6 else 64 * n, columns={"actions": torch.int32}, seed=3)     # the torch route's rings
        g = torch.Generator(device="cuda")
        g.manual_seed(n)
        acts = torch.randint(0, 5, (20, n), dtype=torch.int32, device=dev, generator=g)
        obs, rew, done = eng.rollout(acts)                    # real rows
        done[7, ::5] = 1                                      # some finished rows, so that final_obs is read
        fin = obs.flip(0).contiguous()
        S = buf.buffer_size
        for w in range(-(-S // 20) if n != 6 else 4):         # N = 65 536: fill all 64 rows; N = 6: 80 of 166 666 rows live
            k = min(20, S)
            buf.add(prev, obs[:k], rew[:k], done[:k], final_obs=fin[:k], actions=acts[:k])
            twin.add(prev, obs[:k], rew[:k], done[:k], final_obs=fin[:k], actions=acts[:k])
        eng.sync()
        made[n] = (eng, buf, twin, prev, obs, rew, done, fin, acts)
        return made[n]

    print(f"{'N':>6s} {'T':>3s}  {'add':>29s}  {'torch route':>29s}  {'bytes':>10s} {'GB/s':>7s} {'of 8 TB/s':>9s} {'torch/add':>9s}")
    for n, T in ADD_SHAPES:
        eng, buf, twin, prev, obs, rew, done, fin, acts = setup(n)
        F, S = eng.obs_dim, buf.buffer_size
        st = twin.storage
        ar = torch.arange(T, device=dev)

        def torch_route():
            slots = (st.cursor[0] + ar) % S
            st.obs_ring.index_copy_(0, slots, torch.cat([prev[None], obs[:T - 1]]))
            st.next_ring.index_copy_(0, slots, torch.where(done[:T, :, None] != 0, fin[:T], obs[:T]))
            st.col_rings[0].index_copy_(0, slots, acts[:T])
            st.col_rings[1].index_copy_(0, slots, rew[:T])
            st.col_rings[2].index_copy_(0, slots, done[:T].float())
            st.cursor[0] += T

        ta, tt = [], []
        for rep in range(args.warmup + args.reps):
            a, _ = timed(lambda: buf.add(prev, obs[:T], rew[:T], done[:T], final_obs=fin[:T], actions=acts[:T]))
            b, _ = timed(torch_route)
            if rep >= args.warmup:
                ta.append(a); tt.append(b)
        eng.sync()
        same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in
                   zip([buf.storage.obs_ring, buf.storage.next_ring] + buf.storage.col_rings, [st.obs_ring, st.next_ring] + st.col_rings))
        assert same and buf.cursor()[0] == twin.cursor()[0], "the torch route and ptg_replay_add disagree"
        nbytes = T * n * (3 * F * 4 + 9 + 12) + n * F * 4
        med = statistics.median(ta)
        gbs = nbytes / (med * 1e-6) / 1e9
        print(f"{n:6d} {T:3d}  {stats(ta):>29s}  {stats(tt):>29s}  {nbytes:10d} {gbs:7.1f} {gbs * 1e9 / HBM_PEAK:9.4f} {statistics.median(tt) / med:9.2f}"
              f"   # rings byte-equal: {same}")
    print(f"{'N':>6s} {'B':>6s}  {'sample':>29s}  {'torch route':>29s}  {'bytes':>10s} {'GB/s':>7s} {'of 8 TB/s':>9s} {'torch/smp':>9s}")
    for n, B in SAMPLE_SHAPES:
        eng, buf, twin, prev, obs, rew, done, fin, acts = setup(n)
        F = eng.obs_dim
        st = buf.storage
        live = buf.size() * n
        out = eng.replay_sample(st, batch_size=B, seed=3, want_idx=True)
        flat = [st.obs_ring.view(-1, F), st.next_ring.view(-1, F)] + [c.view(-1) for c in st.col_rings]

        def torch_route():
            i = torch.randint(0, live, (B,), device=dev)
            return [x[i] for x in flat]

        ts, tt = [], []
        for rep in range(args.warmup + args.reps):
            a, _ = timed(lambda: eng.replay_sample(st, batch_size=B, seed=3, out=out))
            b, _ = timed(torch_route)
            if rep >= args.warmup:
                ts.append(a); tt.append(b)
        eng.sync()
        i = out[3]
        same = all(torch.equal(o.view(torch.uint8), x[i].view(torch.uint8)) for o, x in zip([out[0], out[1]] + out[2], flat))
        assert same and int(i.min()) >= 0 and int(i.max()) < live, "ptg_replay_sample's rows are not a gather at its indices"
        nbytes = B * (4 * F * 4 + 24)
        med = statistics.median(ts)
        gbs = nbytes / (med * 1e-6) / 1e9
        print(f"{n:6d} {B:6d}  {stats(ts):>29s}  {stats(tt):>29s}  {nbytes:10d} {gbs:7.1f} {gbs * 1e9 / HBM_PEAK:9.4f} {statistics.median(tt) / med:9.2f}"
              f"   # rows equal a gather at idx_out: {same}")
    made.clear()


if __name__ == "__main__":
    main()
