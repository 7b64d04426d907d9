"""ptg_policy_loss, HipEngine.policy_loss and rl_ptg_amd.loss (include/ptg_env.h) -- the PPO / A2C loss of a minibatch, SB3's logged
statistics and the gradients with respect to the network's outputs in one pass -- against the NumPy restatement
(tests/policy_loss_restatement.py, pinned against torch autograd by tests/test_policy_loss_host.py).

Tolerances, derived and not measured.  The kernel computes in float64 and rounds a gradient once on the store, so against the
float64 restatement only the last-place differences between the device's and libm's exp / log and the order of the batch sums show:
  float64 gradients  within 1e-12 * max(1, |B * ref|) / B (tests/test_act.py's bound, on the gradient before its division by B)
  float32 gradients  within one float32 spacing of the restatement rounded to float32
  every mean         within (B * 2^-53 + 1e-12) * max(1, mean |term|): summation of B terms in any order, plus the per-term bound;
                     the advantage mean and std alike, on the scale of max(1, mean |adv|) resp. max(1, std)
  loss               the same bound applied to its three means, weighted by 1, ent_coef and vf_coef, plus 4 * 2^-53 * max(1, |loss|):
                     loss is not a mean but (policy_loss + c_e * entropy_loss) + c_v * value_loss, two products and two sums on top
                     of the means, each rounded once -- a term added here, beyond the bound on the means, for those four roundings
  clip_fraction      exact (tests/test_policy_loss_host.py shows that no ratio of these inputs is within 1e-9 of a clip edge)
Each test prints its measured maxima in units of its tolerance."""
import ctypes as C

import numpy as np
import pytest

import policy_loss_restatement as pr

pytestmark = pytest.mark.gpu

SENTINEL = 7.5
_engines = {}
_spec = []
CONFIGS = [("ppo", True, pr.CLIP_VF), ("ppo", False, None), ("a2c", False, None), ("a2c", True, pr.CLIP_VF)]      # kind, normalise, clip_range_vf


def _engine(n=64, fresh=False):
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    if not fresh and n in _engines:
        return _engines[n]
    if not _spec:
        _spec.append(synthetic_spec(scenario=2, operation="OP2", eps_len_d=1, train_steps=200000)[0])      # 139-step episodes
    s = _spec[0]
    eng = HipEngine(s.consts, s.tables, s.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
    eng.set_episode_plan(s.eps_ind, n, n)
    eng.set_noise_rng(seed=4)
    if not fresh:
        _engines[n] = eng
    return eng


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_case(c, wide, act_dtype=None):
    """host case -> device tensors; wide: logits and values are columns of one [B, A + 1] tensor, and so are the gradients (rows of
    SENTINEL above and below it); else everything is contiguous and separate"""
    import torch
    d = {k: _t(v) for k, v in c.items()}
    if act_dtype is not None:
        d["actions"] = d["actions"].to(act_dtype)
    B, A = c["logits"].shape
    dt = d["logits"].dtype
    stats = torch.full((8,), SENTINEL, dtype=torch.float64, device="cuda")
    if wide:
        w = torch.cat([d["logits"], d["values"][:, None]], dim=1)
        d["logits"], d["values"] = w[:, :A], w[:, A]
        guard = torch.full((B + 2, A + 1), SENTINEL, dtype=dt, device="cuda")
        G = guard[1:B + 1]
        d["out"], d["guard"] = (stats, G[:, :A], G[:, A], None), guard
    else:
        d["out"] = (stats, torch.full((B, A), SENTINEL, dtype=dt, device="cuda"), torch.full((B,), SENTINEL, dtype=dt, device="cuda"), None)
    return d


def _grad_err(got, ref64, B, skip=None):
    """max error of a gradient in units of its tolerance; rows in skip (untouched by the kernel) are left out; NaN must meet NaN"""
    got = got.cpu().numpy()
    ref64 = np.asarray(ref64, np.float64).reshape(got.shape)
    keep = np.ones(got.shape[0], bool)
    if skip is not None:
        keep &= ~skip
    got, ref64 = got[keep], ref64[keep]
    nan = np.isnan(ref64)
    assert np.array_equal(np.isnan(got), nan)
    if nan.all():
        return 0.0
    if got.dtype == np.float32:
        ref = ref64.astype(np.float32)
        tol = np.spacing(np.abs(ref)).astype(np.float64)
        d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    else:
        tol = 1e-12 * np.maximum(1.0, np.abs(B * ref64)) / B
        d = np.abs(got - ref64)
    return float((d[~nan] / tol[~nan]).max())


def _stats_err(stats, ref, B, ent_coef, vf_coef, adv):
    """max error of the statistics in units of their tolerance; clip_fraction must be exact"""
    got, want = stats.cpu().numpy(), ref["stats"]
    u = B * 2.0 ** -53 + 1e-12
    am = ref["abs_mean"]
    tol = {k: u * max(1.0, am[k]) for k in ("policy_loss", "value_loss", "entropy_loss", "approx_kl")}
    e = {k: abs(got[i] - want[i]) / tol[k] for i, k in ((1, "policy_loss"), (2, "value_loss"), (3, "entropy_loss"), (4, "approx_kl"))}
    e["loss"] = abs(got[0] - want[0]) / (tol["policy_loss"] + abs(ent_coef) * tol["entropy_loss"] + abs(vf_coef) * tol["value_loss"] + 4 * 2.0 ** -53 * max(1.0, abs(want[0])))
    assert got[5] == want[5], (got[5], want[5])
    a64 = np.asarray(adv, np.float64)
    e["adv_mean"] = abs(got[6] - want[6]) / (u * max(1.0, float(np.abs(a64).mean())))
    e["adv_std"] = abs(got[7] - want[7]) / (u * max(1.0, want[7]))
    return max(e.values())


def _run(eng, kind, norm, cvf, d, ws=None, **kw):
    return eng.policy_loss(kind, d["logits"], d["values"], d["actions"], d["old_log_prob"] if kind == "ppo" else None, d["advantages"], d["returns"],
                           clip_range=pr.CLIP if kind == "ppo" else None, clip_range_vf=cvf, ent_coef=pr.ENT_COEF, vf_coef=pr.VF_COEF,
                           normalize_advantage=norm, old_values=d["old_values"] if cvf is not None else None, out=d.get("out"), workspace=ws, **kw)


def _ref(kind, norm, cvf, c, **kw):
    return pr.policy_loss(kind, c["mean"] if "mean" in c else c["logits"], c["values"], c["actions"], c["old_log_prob"], c["advantages"], c["returns"],
                          clip_range=pr.CLIP, clip_range_vf=cvf, ent_coef=pr.ENT_COEF, vf_coef=pr.VF_COEF, normalize_advantage=norm,
                          old_values=c["old_values"], log_std=c.get("log_std"), **kw)


def _check_case(eng, c, wide, act_dtype, configs=CONFIGS):
    import torch
    B = c["logits"].shape[0]
    worst = dict(grad=0.0, stats=0.0)
    for kind, norm, cvf in configs:
        d = _device_case(c, wide, act_dtype)
        res = _run(eng, kind, norm, cvf, d)
        eng.sync()
        ref = _ref(kind, norm, cvf, c)
        assert res.grad_log_std is None and res.stats.data_ptr() == d["out"][0].data_ptr()
        worst["grad"] = max(worst["grad"], _grad_err(res.grad_input, ref["grad_input"], B), _grad_err(res.grad_values, ref["grad_values"], B))
        worst["stats"] = max(worst["stats"], _stats_err(res.stats, ref, B, pr.ENT_COEF, pr.VF_COEF, c["advantages"]))
        if wide:                                             # one [B, A + 1] tensor was filled, and nothing around it
            g = d["guard"]
            assert bool((g[0] == SENTINEL).all()) and bool((g[-1] == SENTINEL).all())
            assert torch.equal(g[1:-1, :-1], res.grad_input) and torch.equal(g[1:-1, -1], res.grad_values)
    return worst


@pytest.mark.parametrize("B", pr.BS)
def test_both_losses_over_every_shape(B):
    """B at 1, 2, around the wave, PPO's 203, past one block (257: the single-launch route ends at 256 rows) and 4 097; A in {2, 5,
    32}; float32 and float64; int32 and int64 actions, each with contiguous inputs and separate gradient tensors (row stride A) and
    with an [B, A + 1] actor-critic tensor read and written in place (row stride A + 1); PPO and A2C, each with and without advantage normalisation and value clipping; the planted rows of
    tests/policy_loss_restatement.py case()"""
    import torch
    eng = _engine()
    worst = dict(grad32=0.0, stats32=0.0, grad64=0.0, stats64=0.0)
    for A in pr.AS:
        for dt in pr.DTYPES:
            c = pr.case(B, A, dt)
            tag = "32" if dt == np.float32 else "64"
            for wide in (False, True):                       # row stride A (everything contiguous and separate) / A + 1 (in place)
                for adt in (torch.int32, torch.int64):
                    w = _check_case(eng, c, wide, adt)
                    worst["grad" + tag] = max(worst["grad" + tag], w["grad"])
                    worst["stats" + tag] = max(worst["stats" + tag], w["stats"])
    print(f"B={B}: max error / tolerance", {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


def test_a_batch_that_crosses_the_partial_boundaries():
    """70 001 rows = 274 blocks of 256: the final merge's 256 threads walk the block partials in laps of 256, so 18 threads take a
    second partial (one lap boundary crossed), and the moment merge's 64 lanes walk them in laps of 64 (boundaries at 64, 128, 192
    and 256 blocks crossed); the last block is ragged (113 rows, its last wave 49)"""
    import torch
    eng = _engine()
    worst = {}
    for dt in pr.DTYPES:
        c = pr.case(pr.B_BIG, 5, dt)
        worst[np.dtype(dt).name] = _check_case(eng, c, True, torch.int32, configs=CONFIGS[:1] + CONFIGS[2:3])
    print("B=70001: max error / tolerance", worst)
    assert max(max(w.values()) for w in worst.values()) <= 1.0, worst


@pytest.mark.parametrize("B", [1, 65, 203, 4097])
def test_the_gaussian_head(B):
    """means [B] (contiguous, and as column 0 of a [B, 2] tensor beside the values), the stored raw samples as actions, one log_std:
    gradients with respect to the means, the values and log_std"""
    import torch
    eng = _engine()
    worst = 0.0
    for dt in pr.DTYPES:
        c = pr.gaussian_case(B, dt)
        for kind, norm, cvf in CONFIGS:
            for wide in (False, True):
                d = {k: _t(v) for k, v in c.items()}
                if wide:
                    w = torch.stack([d["mean"], d["values"]], dim=1)
                    d["mean"], d["values"] = w[:, 0], w[:, 1]
                res = eng.policy_loss(kind, d["mean"], d["values"], d["actions"], d["old_log_prob"] if kind == "ppo" else None, d["advantages"], d["returns"],
                                      clip_range=pr.CLIP if kind == "ppo" else None, clip_range_vf=cvf, ent_coef=pr.ENT_COEF, vf_coef=pr.VF_COEF,
                                      normalize_advantage=norm, old_values=d["old_values"] if cvf is not None else None, log_std=d["log_std"])
                eng.sync()
                ref = _ref(kind, norm, cvf, c)
                gls = ref["grad_log_std"]
                e = [_grad_err(res.grad_input, ref["grad_input"], B), _grad_err(res.grad_values, ref["grad_values"], B),
                     _stats_err(res.stats, ref, B, pr.ENT_COEF, pr.VF_COEF, c["advantages"])]
                got = float(res.grad_log_std[0])
                if dt == np.float32:                         # a sum over the batch rounded once: one float32 spacing, plus the summation bound
                    e.append(abs(got - float(np.float32(gls))) / (float(np.spacing(np.float32(abs(gls)))) + (B * 2.0 ** -53 + 1e-12) * max(1.0, abs(gls))))
                else:
                    e.append(abs(got - gls) / ((B * 2.0 ** -53 + 1e-12) * max(1.0, abs(gls))))
                worst = max(worst, *e)
                assert res.grad_input.shape == (B,) and res.grad_log_std.shape == (1,)
    print(f"B={B}: max error / tolerance {worst:.4f}")
    assert worst <= 1.0


def test_two_runs_give_identical_bits():
    import torch
    eng = _engine()
    for B, dt in ((203, np.float32), (pr.B_BIG, np.float32), (pr.B_BIG, np.float64)):
        c = pr.case(B, 5, dt)
        runs = []
        for _ in range(2):
            d = _device_case(c, True, torch.int32)
            res = _run(eng, "ppo", True, pr.CLIP_VF, d)
            eng.sync()
            runs.append((res.stats.clone(), d["guard"].clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), (B, dt)
        assert bool(torch.isfinite(runs[0][0]).all())


def _torch_lines(kind, out, A, d, norm, cvf):
    """SB3's lines on the device in the tensors' dtype, on the [B, A + 1] output of a network"""
    import torch
    import torch.nn.functional as F
    dist = torch.distributions.Categorical(logits=out[:, :A])
    values = out[:, A]
    log_prob, entropy = dist.log_prob(d["actions"]), dist.entropy()
    advantages = d["advantages"]
    if norm and len(advantages) > 1:
        advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
    if kind == "ppo":
        ratio = torch.exp(log_prob - d["old_log_prob"])
        policy_loss = -torch.min(advantages * ratio, advantages * torch.clamp(ratio, 1 - pr.CLIP, 1 + pr.CLIP)).mean()
    else:
        policy_loss = -(advantages * log_prob).mean()
    values_pred = values if cvf is None else d["old_values"] + torch.clamp(values - d["old_values"], -cvf, cvf)
    return policy_loss + pr.ENT_COEF * -torch.mean(entropy) + pr.VF_COEF * F.mse_loss(d["returns"], values_pred)


def test_loss_backward_drives_a_network_as_torch_autograd_does():
    """float64 Linear(40, A + 1): after loss.backward() through rl_ptg_amd.loss the parameter gradients equal those of SB3's lines
    under torch autograd on the device within 1e-12 * max(1, max |ref|); the loss itself too"""
    import torch
    from rl_ptg_amd import a2c_loss, ppo_loss
    eng = _engine()
    B, A = 203, 5
    torch.manual_seed(3)
    net = torch.nn.Linear(40, A + 1).double().cuda()
    obs = torch.randn(B, 40, dtype=torch.float64, device="cuda")
    c = pr.case(B, A, np.float64)
    d = {k: _t(v) for k, v in c.items()}
    with torch.no_grad():
        out0 = net(obs)
        lp0 = torch.distributions.Categorical(logits=out0[:, :A]).log_prob(d["actions"])
        d["old_log_prob"] = (lp0 - _t(np.random.default_rng(5).uniform(-0.5, 0.5, B))).contiguous()
        d["old_values"] = (out0[:, A] + _t(np.random.default_rng(6).uniform(-0.6, 0.6, B))).contiguous()
    ratio = torch.exp(lp0 - d["old_log_prob"])
    assert float(torch.minimum((ratio - (1 - pr.CLIP)).abs(), (ratio - (1 + pr.CLIP)).abs()).min()) > 1e-9
    worst = 0.0
    for kind, norm, cvf in CONFIGS:
        if kind == "a2c":
            cvf = None                                       # a2c_loss has no value clipping: SB3's A2C has none
        net.zero_grad()
        _torch_lines(kind, net(obs), A, d, norm, cvf).backward()
        ref = [p.grad.clone() for p in net.parameters()]
        ref_loss = float(_torch_lines(kind, net(obs), A, d, norm, cvf).detach())
        net.zero_grad()
        out = net(obs)
        if kind == "ppo":
            loss, stats = ppo_loss(eng, out[:, :A], out[:, A], d["actions"], d["old_log_prob"], d["advantages"], d["returns"], clip_range=pr.CLIP,
                                   clip_range_vf=cvf, ent_coef=pr.ENT_COEF, vf_coef=pr.VF_COEF, normalize_advantage=norm, old_values=d["old_values"] if cvf else None)
        else:
            loss, stats = a2c_loss(eng, out[:, :A], out[:, A], d["actions"], d["advantages"], d["returns"], ent_coef=pr.ENT_COEF, vf_coef=pr.VF_COEF,
                                   normalize_advantage=norm)
        assert loss.dim() == 0 and loss.dtype == torch.float64 and loss.requires_grad and not stats.requires_grad
        loss.backward()
        eng.sync()
        assert abs(float(loss) - ref_loss) <= 1e-12 * max(1.0, abs(ref_loss)) and float(stats[0]) == float(loss)
        for p, r in zip(net.parameters(), ref):
            worst = max(worst, float((p.grad - r).abs().max()) / (1e-12 * max(1.0, float(r.abs().max()))))
    print(f"parameter gradients: max error / tolerance {worst:.4f}")
    assert worst <= 1.0
    # a float32 network: the loss comes back in float32 and twice the loss gives twice the gradients
    net32 = torch.nn.Linear(40, A + 1).cuda()
    d32 = {k: (v.float() if v.is_floating_point() else v) for k, v in d.items()}
    grads = []
    for scale in (1.0, 2.0):
        net32.zero_grad()
        out = net32(obs.float())
        loss, _ = ppo_loss(eng, out[:, :A], out[:, A], d32["actions"], d32["old_log_prob"], d32["advantages"], d32["returns"], clip_range=pr.CLIP)
        assert loss.dtype == torch.float32
        (loss * scale).backward()
        grads.append(net32.weight.grad.clone())
    eng.sync()
    assert torch.equal(grads[0] * 2.0, grads[1]) and float(grads[0].abs().max()) > 0


def test_behind_a_real_rollout_chain():
    """rollout -> vn_normalize -> gae -> minibatches -> policy_loss on 64 envs x 29 steps in PPO's batches of 203 (the last one 29
    rows), every batch against the restatement on what the gather delivered"""
    import torch
    N, T, A = 64, 29, 5
    eng = _engine(N, fresh=True)
    eng.vn_init()
    eng.reset()
    g = torch.Generator(device="cuda"); g.manual_seed(2)
    net = torch.nn.Linear(eng.obs_dim, A + 1).cuda()
    acts = torch.randint(0, A, (T, N), dtype=torch.int32, device="cuda", generator=g)
    obs, rew, done = eng.rollout(acts)
    with torch.no_grad():
        out = net(eng.rows(obs).reshape(T * N, -1)).reshape(T, N, A + 1)
        old_lp = torch.distributions.Categorical(logits=out[..., :A]).log_prob(acts.long()).contiguous()
        values = out[..., A].contiguous()
        last_values = values[-1].clone()
    rn = eng.vn_normalize(rew, done)
    adv, ret = eng.gae(rn, values, done, last_values, 0.99, 0.95)
    perm = torch.randperm(T * N, device="cuda", generator=g)
    worst, batches = 0.0, 0
    with torch.no_grad():
        net.weight.mul_(1.05)                                # an optimiser step later: the ratios are no longer 1
    for ob, (a_b, v_b, lp_b, adv_b, ret_b) in eng.minibatches(perm, 203, obs, [acts, values, old_lp, adv, ret]):
        with torch.no_grad():
            o = net(ob)
        res = eng.policy_loss("ppo", o[:, :A], o[:, A], a_b, lp_b, adv_b, ret_b, clip_range=pr.CLIP, clip_range_vf=pr.CLIP_VF, ent_coef=pr.ENT_COEF,
                              vf_coef=pr.VF_COEF, old_values=v_b)
        eng.sync()
        B = a_b.shape[0]
        h = lambda t: t.cpu().numpy()
        ref = pr.policy_loss("ppo", h(o[:, :A]), h(o[:, A]), h(a_b), h(lp_b), h(adv_b), h(ret_b), clip_range=pr.CLIP, clip_range_vf=pr.CLIP_VF,
                             ent_coef=pr.ENT_COEF, vf_coef=pr.VF_COEF, old_values=h(v_b))
        assert ref["margin"] >= 1e-9 and not ref["bad"].any()
        worst = max(worst, _grad_err(res.grad_input, ref["grad_input"], B), _grad_err(res.grad_values, ref["grad_values"], B),
                    _stats_err(res.stats, ref, B, pr.ENT_COEF, pr.VF_COEF, h(adv_b)))
        batches += 1
    assert batches == 10 and B == 29 and worst <= 1.0, (batches, B, worst)
    eng.close()


def test_on_a_side_stream():
    import torch
    eng = _engine()
    c = pr.case(257, 5, np.float64)
    side = torch.cuda.Stream()
    d = _device_case(c, True, torch.int64)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = _run(eng, "ppo", True, None, d)
        eng.sync()
    torch.cuda.current_stream().wait_stream(side)
    ref = _ref("ppo", True, None, c)
    assert _grad_err(res.grad_input, ref["grad_input"], 257) <= 1.0 and _stats_err(res.stats, ref, 257, pr.ENT_COEF, pr.VF_COEF, c["advantages"]) <= 1.0


@pytest.mark.parametrize("B", [203, 1000])
def test_captured_and_replayed_three_times_with_rewritten_logits(B):
    """one launch (203) and the four-kernel chain (1 000) captured on a side stream with out= and workspace=, replayed three times
    with other logits, values and log-probs written into the graph's inputs; the host doubles (clip ranges, coefficients) are kept"""
    import torch
    eng = _engine()
    A = 5
    cases = [pr.case(B, A, np.float32, seed=k) for k in range(4)]
    d = _device_case(cases[0], True, torch.int32)
    ws = eng.policy_loss_workspace(B)

    def load(k):
        src = _device_case(cases[k], True, torch.int32)
        for name in ("logits", "values", "actions", "old_log_prob", "advantages", "returns", "old_values"):
            d[name].copy_(src[name])

    def check(k):
        ref = _ref("ppo", True, pr.CLIP_VF, cases[k])
        assert _grad_err(d["out"][1], ref["grad_input"], B) <= 1.0 and _grad_err(d["out"][2], ref["grad_values"], B) <= 1.0, k
        assert _stats_err(d["out"][0], ref, B, pr.ENT_COEF, pr.VF_COEF, cases[k]["advantages"]) <= 1.0, k

    _run(eng, "ppo", True, pr.CLIP_VF, d, ws)                # eager once: code objects are loaded before the capture
    eng.sync()
    check(0)
    d["guard"].fill_(SENTINEL)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            _run(eng, "ppo", True, pr.CLIP_VF, d, ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert bool((d["guard"] == SENTINEL).all())              # capturing enqueued nothing
    for k in (1, 2, 3):
        load(k)
        graph.replay()
        torch.cuda.synchronize()
        check(k)
    eng.sync()


def _equal_state(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_equal_state(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def test_no_host_synchronisation_and_nothing_else_touched():
    """A condition, not a timing: the stream is busy with milliseconds of fused steps before the calls and still busy when they
    have returned.  Afterwards env state, finished ring, vn statistics and a replay cursor equal a twin's that made no call."""
    import torch
    from rl_ptg_amd import DeviceReplayBuffer
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    n, T, calls, A = 65536, 250, 8, 5
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=32)          # 4 608-step episodes: no boundary inside
    engs = []
    for _ in range(2):
        e = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
        e.set_episode_plan(spec.eps_ind, n, n)
        e.set_noise_rng(5)
        e.vn_init()
        e.reset()
        engs.append(e)
    eng, twin = engs
    buf = DeviceReplayBuffer(eng, 2 * n)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    acts = torch.randint(0, 5, (T, n), dtype=torch.int32, device="cuda", generator=g)
    c = pr.case(n, A, np.float32)
    d = _device_case(c, True, torch.int32)
    ws = eng.policy_loss_workspace(n)
    obs, rew, done = eng.alloc_obs(T), torch.empty((T, n), device="cuda"), torch.empty((T, n), dtype=torch.uint8, device="cuda")
    eng.rollout(acts, obs, rew, done)                                            # warm: first-launch work is not part of the condition
    twin.rollout(acts)
    _run(eng, "ppo", True, pr.CLIP_VF, d, ws)
    _run(eng, "a2c", False, None, d, ws)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    assert stream.query() is True
    for _ in range(calls):
        eng.rollout(acts, obs, rew, done)
    busy_before = stream.query()
    _run(eng, "a2c", False, None, d, ws)
    _run(eng, "ppo", True, pr.CLIP_VF, d, ws)
    busy_after = stream.query()
    assert busy_before is False, "the rollouts were over before the calls: the check would prove nothing"
    assert busy_after is False, "the stream was idle when the calls had returned: a call waited for the device"
    eng.sync()
    ref = _ref("ppo", True, pr.CLIP_VF, c)
    assert _grad_err(d["out"][1], ref["grad_input"], n) <= 1.0 and _stats_err(d["out"][0], ref, n, pr.ENT_COEF, pr.VF_COEF, c["advantages"]) <= 1.0
    for _ in range(calls):
        twin.rollout(acts)
    twin.sync()
    a, b = eng.state_dict(), twin.state_dict()
    assert _equal_state(a["fields"], b["fields"]) and _equal_state(a["vn"], b["vn"])
    assert buf.cursor() == (0, 0)
    assert len(eng.finished_episodes()[0]) == len(twin.finished_episodes()[0])
    eng.close(); twin.close()


def test_bad_rows():
    """every kind of row the call has no finite loss for: NaN gradients on that row, the others computed, NaN statistics and
    PTG_E_NONFINITE once; an action outside [0, A): the row's gradients untouched and PTG_E_INDEX once; a clean call syncs clean"""
    import torch
    from rl_ptg_amd import _lib
    from rl_ptg_amd.engine import PtgError
    eng = _engine()
    B, A = 300, 5                                            # two blocks: the multi-launch route, no normalisation (a non-finite advantage
    #                                                          would make every row NaN through the moments, as the arithmetic says)

    def expect(code, then_clean=True):
        with pytest.raises(PtgError) as ei:
            eng.sync()
        assert ei.value.code == code and "ptg_policy_loss" in str(ei.value)
        if then_clean:
            eng.sync()

    def spoil(c, k, row):
        act = c["actions"][row]
        if k == "nan_logit": c["logits"][row, 2] = np.nan
        elif k == "inf_logit": c["logits"][row, 0] = np.inf
        elif k == "all_minus_inf": c["logits"][row] = -np.inf
        elif k == "prob_zero": c["logits"][row, act] = -np.inf
        elif k == "ratio_overflow":                          # finite inputs, r = exp(lp + 1e30) = +Inf; on one of the rows Ah * r is 0 * Inf
            c["old_log_prob"][row] = -1e30
            if row % 2: c["advantages"][row] = 0.0
        else: c[k][row] = {0: np.nan, 1: np.inf, 2: -np.inf}[row % 3]

    kinds = ["nan_logit", "inf_logit", "all_minus_inf", "prob_zero", "ratio_overflow", "values", "advantages", "returns", "old_log_prob", "old_values"]
    for dt in pr.DTYPES:
        for k in kinds:                                      # one kind at a time, on a row of either block
            c = pr.case(B, A, dt)
            rows = [20, 277]
            for r in rows:
                spoil(c, k, r)
            d = _device_case(c, True, torch.int64)
            res = _run(eng, "ppo", False, pr.CLIP_VF, d)
            expect(_lib.E_NONFINITE)
            ref = _ref("ppo", False, pr.CLIP_VF, c)
            assert np.nonzero(ref["bad"])[0].tolist() == rows, k
            assert _grad_err(res.grad_input, ref["grad_input"], B) <= 1.0 and _grad_err(res.grad_values, ref["grad_values"], B) <= 1.0, k
            assert bool(torch.isnan(res.grad_input[rows]).all()) and bool(torch.isnan(res.grad_values[rows]).all())
            assert int(torch.isnan(res.grad_input).any(dim=1).sum()) == 2 and bool(torch.isnan(res.stats[:6]).all()), k
        c = pr.case(B, A, dt)                                # all kinds at once, with two actions out of range beside them: one error each
        for j, k in enumerate(kinds):
            spoil(c, k, 30 + j)
        c["actions"][5] = A; c["actions"][299] = -1
        d = _device_case(c, True, torch.int64)
        res = _run(eng, "ppo", False, pr.CLIP_VF, d)
        expect(_lib.E_INDEX, then_clean=False)               # one error per sync: the index word first, then the other, then none
        expect(_lib.E_NONFINITE)
        ref = _ref("ppo", False, pr.CLIP_VF, c)
        assert np.nonzero(ref["oob"])[0].tolist() == [5, 299] and ref["bad"].sum() == len(kinds)
        assert bool((d["guard"][1:-1][[5, 299]] == SENTINEL).all())                   # logit and value gradients alike
        assert _grad_err(res.grad_input, ref["grad_input"], B, skip=ref["oob"]) <= 1.0 and _grad_err(res.grad_values, ref["grad_values"], B, skip=ref["oob"]) <= 1.0
        small = {k: v[:100].copy() for k, v in pr.case(B, A, dt).items()}
        small["actions"][7] = 2 ** 31 - 1                     # an int32 action out of range alone, in the single-launch route
        d = _device_case(small, False, torch.int32)
        res = _run(eng, "a2c", False, None, d)
        expect(_lib.E_INDEX)
        assert bool((res.grad_input[7] == SENTINEL).all()) and float(res.grad_values[7]) == SENTINEL and bool(torch.isnan(res.stats[:4]).all())
        ref = _ref("a2c", False, None, small)
        assert _grad_err(res.grad_input, ref["grad_input"], 100, skip=ref["oob"]) <= 1.0
    # the Gaussian head: a non-finite mean, a non-finite sample; then a NaN and a +Inf log_std (every row)
    c = pr.gaussian_case(B, np.float64)
    c["mean"][3] = np.nan; c["mean"][270] = -np.inf; c["actions"][9] = np.inf
    d = {k: _t(v) for k, v in c.items()}
    gau = lambda d: eng.policy_loss("ppo", d["mean"], d["values"], d["actions"], d["old_log_prob"], d["advantages"], d["returns"], clip_range=pr.CLIP,
                                    normalize_advantage=False, log_std=d["log_std"])
    res = gau(d)
    expect(_lib.E_NONFINITE)
    ref = _ref("ppo", False, None, c)
    assert np.nonzero(ref["bad"])[0].tolist() == [3, 9, 270] and _grad_err(res.grad_input, ref["grad_input"], B) <= 1.0
    assert bool(torch.isnan(res.grad_log_std).all()) and bool(torch.isnan(res.stats[:6]).all())
    for ls in (np.nan, np.inf):
        c = pr.gaussian_case(B, np.float64)
        c["log_std"][0] = ls
        res = gau({k: _t(v) for k, v in c.items()})
        expect(_lib.E_NONFINITE)
        assert bool(torch.isnan(res.grad_input).all()) and bool(torch.isnan(res.grad_values).all())
    c = pr.case(B, A, np.float32)                            # a clean call syncs clean
    res = _run(eng, "ppo", True, pr.CLIP_VF, _device_case(c, True, torch.int32))
    eng.sync()
    assert bool(torch.isfinite(res.stats).all())


def test_refused_arguments_enqueue_nothing():
    import torch
    from rl_ptg_amd import _lib
    eng = _engine()
    B, A = 300, 5
    L, h, stream = eng._L, eng._h, eng._stream()
    c = pr.case(B, A, np.float32)
    d = _device_case(c, True, torch.int32)
    ls = torch.zeros(1, device="cuda")
    g_ls = torch.full((1,), SENTINEL, device="cuda")
    ws = eng.policy_loss_workspace(B)
    ws.fill_(0x5A)
    torch.cuda.synchronize()
    stats, g_in, g_val, _ = d["out"]

    def desc(**kw):
        a = dict(kind=_lib.LOSS_PPO, head=_lib.HEAD_CATEGORICAL, flags=_lib.LOSS_NORM_ADV | _lib.LOSS_CLIP_VF, n_actions=A, in_dtype=_lib.OUT_F32,
                 act_kind=_lib.ACT_I32, batch=B, in_dev=d["logits"].data_ptr(), in_s_n=A + 1, val_dev=d["values"].data_ptr(), val_s_n=A + 1,
                 act_dev=d["actions"].data_ptr(), old_logp_dev=d["old_log_prob"].data_ptr(), adv_dev=d["advantages"].data_ptr(),
                 ret_dev=d["returns"].data_ptr(), old_val_dev=d["old_values"].data_ptr(), clip_range=0.2, clip_range_vf=0.3, ent_coef=0.01, vf_coef=0.5,
                 stats_dev=stats.data_ptr(), grad_in_dev=g_in.data_ptr(), g_s_n=A + 1, grad_val_dev=g_val.data_ptr(), gv_s_n=A + 1, ws_dev=ws.data_ptr())
        a.update(kw)
        return _lib.PtgLoss(**a)

    GAU = dict(head=_lib.HEAD_GAUSSIAN, in_dev=d["returns"].data_ptr(), in_s_n=1, g_s_n=1, log_std_dev=ls.data_ptr(), act_dev=d["advantages"].data_ptr(), grad_log_std_dev=g_ls.data_ptr())
    nan = float("nan")
    bad = [desc(in_dev=None), desc(val_dev=None), desc(act_dev=None), desc(old_logp_dev=None), desc(adv_dev=None), desc(ret_dev=None),
           desc(stats_dev=None), desc(grad_in_dev=None), desc(grad_val_dev=None), desc(ws_dev=None), desc(ws_dev=ws.data_ptr() + 4),
           desc(kind=2), desc(kind=-1), desc(head=_lib.HEAD_EPS_GREEDY), desc(head=3), desc(flags=4), desc(flags=8 | _lib.LOSS_NORM_ADV),
           desc(batch=0), desc(batch=-3), desc(batch=2 ** 40), desc(batch=2 ** 31 + 1), desc(n_actions=1), desc(n_actions=33, in_s_n=33, g_s_n=33), desc(in_s_n=A - 1), desc(g_s_n=A - 1),
           desc(val_s_n=0), desc(gv_s_n=0), desc(val_s_n=-1), desc(in_dtype=2), desc(in_dtype=-1), desc(act_kind=_lib.ACT_F32), desc(act_kind=3),
           desc(old_val_dev=None), desc(grad_log_std_dev=g_ls.data_ptr()), desc(clip_range=nan), desc(clip_range=-0.1), desc(clip_range_vf=nan),
           desc(clip_range_vf=-1.0), desc(**dict(GAU, log_std_dev=None)), desc(**dict(GAU, in_s_n=0)), desc(**dict(GAU, g_s_n=0))]
    for k, ds in enumerate(bad):
        assert L.ptg_policy_loss(h, C.byref(ds), stream) == _lib.E_INVALID, k
        assert b"ptg_policy_loss" in L.ptg_last_error(h)
        assert torch.cuda.current_stream().query() is True, k
    assert L.ptg_policy_loss(h, None, stream) == _lib.E_INVALID and L.ptg_policy_loss(None, C.byref(desc()), stream) == _lib.E_INVALID
    assert torch.cuda.current_stream().query() is True
    assert bool((d["guard"] == SENTINEL).all()) and bool((stats == SENTINEL).all()) and bool((g_ls == SENTINEL).all()) and bool((ws == 0x5A).all())
    good = [desc(), desc(kind=_lib.LOSS_A2C, old_logp_dev=None, clip_range=nan), desc(flags=0, old_val_dev=None, clip_range_vf=nan),
            desc(**GAU), desc(**dict(GAU, grad_log_std_dev=None, act_kind=77)), desc(batch=1), desc(clip_range=0.0, clip_range_vf=0.0)]
    for k, ds in enumerate(good):
        assert L.ptg_policy_loss(h, C.byref(ds), stream) == 0, (k, L.ptg_last_error(h))
    eng.sync()
    assert bool(torch.isfinite(stats).all()) and bool(torch.isfinite(g_ls).all())
