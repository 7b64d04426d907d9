"""python tools/mlp_split_cost.py [--reps 15] [--warmup 3] [--out profiles/mlp_split_cost.txt]

What split observation rows as the first layer's input cost on the device (PTG_MLP_SPLIT_INPUT): the same net on
the same observations two ways, taking turns from one repetition to the next,

  flat    HipEngine.mlp_forward on the [B, 40] SB3_FLAT rows
  split   HipEngine.mlp_forward(..., split=True) on the [B, 16] split rows those flat rows were rebuilt from

for layer 0 alone (a one-layer call of the first Linear with the hidden activation as its output activation) and for the whole net:
40 -> 64 -> 64 -> 5 (tanh, tools/policy_loop.py's policy) and PPO's 40 -> 358 -> 358 -> 5 (ReLU) at B = 6, 203, 4 096 and 65 536 rows,
the host's own choice of tile route.  And one weight-gradient call: mlp_backward of the FIRST LAYER ALONE (one k_mlp_dw launch, no input
gradient) at B = 203 and 4 096, flat against split.
The rows are synthetic: random env columns, hour indices drawn over the whole series.  Every timed section is queued behind a ~100 us
device-side delay (tools/cost_timing.py), so the events bracket device work only.  Medians with min and max over --reps repetitions after
--warmup unrecorded ones.  The two routes' outputs are compared bit for bit after the timing of every shape."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cost_timing  # noqa: E402
from cost_timing import stats  # noqa: E402

NETS = [("policy_loop", [64, 64, 5], "tanh"), ("PPO policy", [358, 358, 5], "relu")]
BATCHES = [6, 203, 4096, 65536]
DW_BATCHES = [203, 4096]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mlp_split_cost.txt"))
    args = ap.parse_args()
    import torch
    from rl_ptg_amd import dist as ptg_dist
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.policy_split import flat_rows_from_split
    from rl_ptg_amd.prep import synthetic_spec
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    spec, _ = synthetic_spec(scenario=1, operation="OP1", eps_len_d=32)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    eng = HipEngine(spec.consts, spec.tables, spec.markets, 6, device=0, out_dtype="float32", obs_layout="split")      # B is not tied to the engine's envs
    first_ptr, stride = ptg_dist.episode_plan(6, 1, 0)
    eng.set_episode_plan(spec.eps_ind, first_ptr, stride)
    series = eng.market_feature_series()
    last_hour = series["featA"].size - 13
    say(f"# tools/mlp_split_cost.py: float32, 'mod', price_ahead 13 (flat width 40); {args.reps} repetitions after {args.warmup} warm-up, flat and split taking "
        f"turns; device time from HIP events [us]: median [min - max]")
    say(f"# torch {torch.__version__}; {torch.cuda.get_device_name(0)}; library {os.environ.get('PTG_LIB_PATH', 'in-tree default')}")
    say(f"{'net':>12s} {'what':>8s} {'B':>6s}  {'flat':>30s}  {'split':>30s} {'split/flat':>10s}")
    torch.manual_seed(0)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    for name, widths, act in NETS:
        ws, bs, k = [], [], 40
        for w in widths:
            lin = torch.nn.Linear(k, w).to(dev)
            ws.append(lin.weight.detach()); bs.append(lin.bias.detach())
            k = w
        for B in BATCHES:
            rows = torch.rand((B, 16), device=dev, generator=g) * 2 - 1
            rows[:, 14] = torch.randint(0, last_hour + 1, (B,), device=dev, generator=g).float()
            rows[:, 15] = 0.0
            flat = flat_rows_from_split(rows, series, "mod", 13).contiguous()
            for what, w_, b_, out_act in (("layer 0", ws[:1], bs[:1], act), ("net", ws, bs, None)):
                wl = [w.shape[0] for w in w_]
                work = torch.empty(eng.mlp_workspace(B, wl), dtype=torch.uint8, device=dev)
                of, os_ = torch.empty((B, wl[-1]), device=dev), torch.empty((B, wl[-1]), device=dev)
                f_flat = lambda: eng.mlp_forward(flat, w_, b_, hidden_activation=act, out_activation=out_act, out=of, workspace=work)
                f_split = lambda: eng.mlp_forward(rows, w_, b_, hidden_activation=act, out_activation=out_act, out=os_, workspace=work, split=True)
                tf, ts = cost_timing.alternate(f_flat, f_split, args.warmup, args.reps)
                eng.sync()
                same = bool(torch.equal(of.view(torch.int32), os_.view(torch.int32)) or torch.equal(of, os_))
                say(f"{name:>12s} {what:>8s} {B:6d}  {stats(tf):>30s}  {stats(ts):>30s} {statistics.median(ts) / statistics.median(tf):10.2f}"
                    + ("" if same else "   # THE TWO ROUTES' OUTPUTS DIFFER"))
            if B in DW_BATCHES:
                w0, b0 = ws[:1], bs[:1]
                work = torch.empty(eng.mlp_workspace(B, [widths[0]], True), dtype=torch.uint8, device=dev)
                out = eng.mlp_forward(flat, w0, b0, hidden_activation=act, workspace=work, keep_hidden=True).out
                gout = torch.rand((B, widths[0]), device=dev, generator=g) - 0.5
                bwork = torch.empty(eng.mlp_backward_workspace(B, [widths[0]]), dtype=torch.uint8, device=dev)
                gf, gs = ([torch.empty_like(w0[0])], [torch.empty_like(b0[0])]), ([torch.empty_like(w0[0])], [torch.empty_like(b0[0])])
                d_flat = lambda: eng.mlp_backward(gout, flat, w0, b0, out, work, hidden_activation=act, grad_weights=gf[0], grad_biases=gf[1], backward_workspace=bwork)
                d_split = lambda: eng.mlp_backward(gout, rows, w0, b0, out, work, hidden_activation=act, grad_weights=gs[0], grad_biases=gs[1], backward_workspace=bwork,
                                                   split=True)
                tf, ts = cost_timing.alternate(d_flat, d_split, args.warmup, args.reps)
                eng.sync()
                same = torch.equal(gf[0][0], gs[0][0]) and torch.equal(gf[1][0], gs[1][0])
                say(f"{name:>12s} {'dW 0':>8s} {B:6d}  {stats(tf):>30s}  {stats(ts):>30s} {statistics.median(ts) / statistics.median(tf):10.2f}"
                    + ("" if same else "   # THE TWO ROUTES' GRADIENTS DIFFER"))
            torch.cuda.empty_cache()
    say("# layer 0: a one-layer call of the first Linear (k_mlp_layer against k_mlp_layer_split); net: all three layers, of which only the first differs.")
    say("# dW 0: mlp_backward of the first layer alone, out_activation None: one k_mlp_dw (k_mlp_dw_split) launch, no k_mlp_dz_out, no k_mlp_dx.")
    say("# not measured: 'raw', other price_ahead, a second input piece, the grouped calls, forced routes, the kernels under a profiler, the host time of a call.")
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
