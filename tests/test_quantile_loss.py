"""ptg_quantile_loss, HipEngine.quantile_loss and rl_ptg_amd.tqc_critic_loss (include/ptg_env.h) -- the sort of the target critics'
quantiles, the TD targets, TQC's quantile-Huber loss, four statistics and the gradients with respect to the current quantiles in one
pass -- against the NumPy restatement (tests/quantile_loss_restatement.py, pinned against torch autograd by
tests/test_quantile_loss_host.py).

Bounds, derived and not measured.  The per-row outputs (the targets y and every gradient) hold no reduction across lanes and no
transcendental: float64 arithmetic in the header's operand order, the j loop in the header's order, every operation rounded once.  They
are compared BIT FOR BIT through integer views: float64 outputs equal the restatement, float32 outputs equal the restatement rounded
once.  With a log alpha on the device the restatement is fed the alpha the kernel reports in stats[5], which itself is held to np.exp
within 2 float64 spacings (1 ulp is the published error of the device library's double exp, NumPy's libm is within 1 ulp of the true
value too; a libm that is off by more would break this bound, not the kernel).
  every mean         within (N * 2^-53 + 1e-12) * max(1, mean |term|), N the number of summands of that mean (B * K * Q * M pairs for the
                     loss and mean |delta|, B * K * Q for the mean quantile, B * M for the mean target): summation of the terms in any
                     order plus the per-term bound
  stats[4]           exact: a count divided once
What was thinned: the issue's cross product (9 batch sizes x 7 shapes x 2 quantile dtypes x 3 layouts x 4 reward / done dtype pairs x
3 alpha forms = 4 536 calls) is walked diagonally.  Every batch size runs every shape at both quantile dtypes; layout, reward / done
pair and alpha form rotate with (shape, dtype, batch) so that each of them meets every shape and every batch size's launch route
somewhere, and the reference's shape (K, Q, d) = (2, 30, 2) runs the full 3 x 3 layout x alpha square at every batch size.  The kernel
has no branch that couples those axes to the batch size beyond the one- or two-launch route.
Each test prints its measured maxima in units of its tolerance."""
import ctypes as C

import numpy as np
import pytest

import quantile_loss_restatement as qr

pytestmark = pytest.mark.gpu

SENTINEL = 7.5
LOG_ALPHA = -1.3125
_engines = {}
_spec = []
RD_DTYPES = [(np.float32, np.float32), (np.float64, np.float32), (np.float32, np.float64), (np.float64, np.float64)]      # rewards, dones
FORMS = ["stacked", "list", "wide"]
MODES = ["host", "dev", "log"]
_worst = {"exp_spacings": 0.0}


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


def _full(shape, dt):
    import torch
    return torch.full(shape, SENTINEL, dtype=dt, device="cuda")


def _same_bits(got, ref64):
    """a per-row output against the restatement rounded once to the output's dtype, through integer views; a NaN must meet a NaN"""
    got = got.detach().cpu().numpy()
    ref = np.asarray(ref64, np.float64).reshape(got.shape).astype(got.dtype)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    iv = np.int32 if got.dtype == np.float32 else np.int64
    assert np.array_equal(got[~nan].view(iv), ref[~nan].view(iv)), float(np.abs(got[~nan].astype(np.float64) - ref[~nan]).max())


def _means_err(stats, ref):
    """max error of stats[0..3] in units of their tolerance; stats[4] and the tail must be exact"""
    got, want, am, cnt = stats.cpu().numpy(), ref["stats"], ref["abs_mean"], ref["count"]
    e = [abs(got[i] - want[i]) / ((cnt[k] * 2.0 ** -53 + 1e-12) * max(1.0, am[k])) for i, k in enumerate(("loss", "q", "y", "abs_delta"))]
    assert got[4] == want[4] and got[6] == 0.0 and got[7] == 0.0, (got, want)
    return max(e)


def _device(c, drop, form):
    """host case -> device tensors and out=.  stacked: SB3's [B, K, Q] tensors, the gradient a [B, K, Q] slice between two guard rows;
    list: K contiguous [B, Q] tensors; wide: K tensors with the row stride Q + 1 whose last column is a guard, the gradients also
    between guard rows"""
    import torch
    B, K, Q = c["quantiles"].shape
    d = {k: _t(v) for k, v in c.items()}
    dt = d["quantiles"].dtype
    if form == "stacked":
        g = _full((B + 2, K, Q), dt)
        d["guards"], grad = [g], g[1:B + 1]
    else:
        pad = 1 if form == "wide" else 0
        for name in ("quantiles", "next_quantiles"):
            ws = [_full((B, Q + pad), dt) for _ in range(K)]
            for k in range(K):
                ws[k][:, :Q] = d[name][:, k]
            d[name + "_wide"], d[name] = ws, [w[:, :Q] for w in ws]
        gs = [_full((B + 2, Q + pad), dt) for _ in range(K)]
        d["guards"], grad = gs, [g[1:B + 1, :Q] for g in gs]
    d["out"] = (_full((8,), torch.float64), grad, _full((B, K * (Q - drop)), dt))
    return d


def _grad_of(d, form):
    """the gradients as [B, K, Q]"""
    import torch
    g = d["out"][1]
    return g if form == "stacked" else torch.stack(list(g), dim=1)


def _guards_untouched(d, form):
    for g in d["guards"]:
        assert bool((g[0] == SENTINEL).all()) and bool((g[-1] == SENTINEL).all())
        if form == "wide":
            assert bool((g[:, -1] == SENTINEL).all())
    if form == "wide":
        for name in ("quantiles_wide", "next_quantiles_wide"):
            assert all(bool((w[:, -1] == SENTINEL).all()) for w in d[name])


def _mode_kw(mode, log_alpha=LOG_ALPHA):
    import torch
    if mode == "host":
        return dict(ent_coef=qr.ALPHA), qr.ALPHA
    if mode == "dev":
        return dict(ent_coef=torch.tensor([qr.ALPHA], dtype=torch.float64, device="cuda")), qr.ALPHA
    return dict(log_ent_coef=torch.tensor([log_alpha], dtype=torch.float64, device="cuda")), None


def _alpha_of(stats, mode, alpha, log_alpha=LOG_ALPHA):
    """the alpha the restatement is fed: the given one, which stats[5] must equal -- or, for a log alpha, the kernel's own stats[5],
    held to np.exp within 2 float64 spacings"""
    got = float(stats[5])
    if mode != "log":
        assert got == alpha
        return alpha
    want = float(np.exp(log_alpha))
    dist = abs(got - want) / float(np.spacing(want))
    _worst["exp_spacings"] = max(_worst["exp_spacings"], dist)
    assert dist <= 2.0, (got, want)
    return got


_refs = {}


def _ref(key, c, drop, alpha, gamma=qr.GAMMA):
    """the restatement of a case, computed once per (case, alpha) and left unchanged"""
    key = key + (alpha, gamma)
    if key not in _refs:
        _refs[key] = qr.quantile_loss(c["quantiles"], c["next_quantiles"], c["rewards"], c["dones"], c["next_log_prob"], gamma, drop, alpha)
    return _refs[key]


def _check(eng, key, c, drop, form, mode, ws=None):
    kw, alpha = _mode_kw(mode)
    d = _device(c, drop, form)
    res = eng.quantile_loss(d["quantiles"], d["next_quantiles"], d["rewards"], d["dones"], d["next_log_prob"], qr.GAMMA, drop, want_target=True,
                            out=d["out"], workspace=ws, **kw)
    eng.sync()
    ref = _ref(key, c, drop, _alpha_of(res.stats, mode, alpha))
    assert not ref["bad"].any() and res.stats is d["out"][0] and res.grad_quantiles is d["out"][1]
    _same_bits(_grad_of(d, form), ref["grad"])
    _same_bits(res.target, ref["y"])
    _guards_untouched(d, form)
    return _means_err(res.stats, ref)


@pytest.mark.parametrize("B", qr.BS)
def test_over_every_shape(B):
    """B at the one-block edge (1 .. 4 one launch, 5 two), the block edges 8 | 9, the reference's 290 and 1 029 rows = 258 partials, where
    the final pass crosses its 256-thread lap; (K, Q, d) with 1, 50, 60, 64, 99 and 256 pairs a row and M from 1 to 256; float32 and float64
    quantiles; the three layouts, guard rows and columns untouched; the reward / done dtype pairs; the three alpha forms; the planted rows
    of tests/quantile_loss_restatement.py.  The docstring of the file says how the cross product is thinned"""
    eng = _engine()
    worst, runs = 0.0, 0
    for s, (K, Q, drop) in enumerate(qr.GPU_SHAPES):
        for t, dt in enumerate(qr.DTYPES):
            turn = s + 2 * t + qr.BS.index(B)
            rdt, ddt = RD_DTYPES[turn % 4]
            c = qr.case(B, K, Q, drop, dt, rdt=rdt, ddt=ddt)
            key = (B, K, Q, drop, dt, rdt, ddt)
            square = [(f, m) for f in FORMS for m in MODES] if (K, Q, drop) == (2, 30, 2) else [(FORMS[turn % 3], MODES[(turn // 3) % 3])]
            for form, mode in square:
                worst = max(worst, _check(eng, key, c, drop, form, mode))
                runs += 1
    print(f"quantile loss B={B}: {runs} calls; means, max error / tolerance {worst:.2e}; exp(log alpha) against np.exp: {_worst['exp_spacings']:.2f} spacings")
    assert worst <= 1.0


def test_every_layout_reward_pair_and_alpha_form_at_the_reference_shape():
    """B = 290, (K, Q, d) = (2, 30, 2): the four reward / done dtype pairs x both quantile dtypes x the three layouts, the alpha form
    rotating -- the axes that test_over_every_shape walks diagonally, here in full where the reference trains"""
    eng = _engine()
    worst = 0.0
    for t, dt in enumerate(qr.DTYPES):
        for r, (rdt, ddt) in enumerate(RD_DTYPES):
            c = qr.case(290, 2, 30, 2, dt, rdt=rdt, ddt=ddt)
            for f, form in enumerate(FORMS):
                worst = max(worst, _check(eng, (290, 2, 30, 2, dt, rdt, ddt), c, 2, form, MODES[(t + r + f) % 3]))
    print(f"reference shape: means, max error / tolerance {worst:.2e}")
    assert worst <= 1.0


def test_two_runs_give_identical_bits():
    import torch
    eng = _engine()
    for B, dt, form in ((290, np.float32, "stacked"), (1029, np.float64, "wide"), (3, np.float32, "list")):
        c = qr.case(B, 2, 30, 2, dt)
        runs = []
        for _ in range(2):
            d = _device(c, 2, form)
            res = eng.quantile_loss(d["quantiles"], d["next_quantiles"], d["rewards"], d["dones"], d["next_log_prob"], qr.GAMMA, 2,
                                    log_ent_coef=torch.tensor([LOG_ALPHA], dtype=torch.float64, device="cuda"), out=d["out"])
            eng.sync()
            runs.append([res.stats.clone(), res.target.clone()] + [g.clone() for g in d["guards"]])
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(*runs)) and bool(torch.isfinite(runs[0][0]).all())


# ------------------------------------------------------------------------------------------------- the autograd wrapper
def _torch_loss(qs, nqs, d, gamma, alpha, drop):
    """sb3_contrib's lines on the device; the float32 columns of a replay sample are widened first"""
    import torch
    cur, nxt = torch.stack(list(qs), dim=1), torch.stack(list(nqs), dim=1)
    K, Q = cur.shape[1], cur.shape[2]
    return qr.tqc_lines(torch, cur, nxt, d["rewards"].double().reshape(-1, 1), d["dones"].double().reshape(-1, 1), d["next_log_prob"].double(), gamma, alpha,
                        K * Q - drop * K)[0]


def _grad_share(params, ref):
    return max(float((p.grad - r).abs().max()) / (1e-12 * max(1.0, float(r.abs().max()))) for p, r in zip(params, ref))


def test_the_wrapper_drives_networks_as_torch_autograd_does():
    """two float64 Linear(41, 30) critics: after loss.backward() through rl_ptg_amd.tqc_critic_loss the parameter gradients equal those of
    sb3_contrib's lines under torch autograd on the device within 1e-12 * max(1, max |ref|), the loss within 1e-12 * max(1, |ref|) -- with the
    critics' outputs as a list and stacked to SB3's [B, K, Q]"""
    import torch
    from rl_ptg_amd import tqc_critic_loss
    eng = _engine()
    B, K, Q, drop = 290, 2, 30, 2
    torch.manual_seed(7)
    f64 = dict(dtype=torch.float64, device="cuda")
    c = qr.case(B, K, Q, drop, np.float64)
    d = {k: _t(v) for k, v in c.items() if k not in ("quantiles", "next_quantiles")}
    sa, nsa = torch.randn(B, 41, **f64), torch.randn(B, 41, **f64)
    critics = [torch.nn.Linear(41, Q).double().cuda() for _ in range(K)]
    targets = [torch.nn.Linear(41, Q).double().cuda() for _ in range(K)]
    params = [p for m in critics for p in m.parameters()]
    log_alpha = torch.tensor([LOG_ALPHA], **f64)
    with torch.no_grad():
        nqs = [m(nsa) for m in targets]
    _torch_loss([m(sa) for m in critics], nqs, d, qr.GAMMA, log_alpha.exp(), drop).backward()
    ref = [p.grad.clone() for p in params]
    ref_loss = float(_torch_loss([m(sa) for m in critics], nqs, d, qr.GAMMA, log_alpha.exp(), drop).detach())
    worst = 0.0
    for stacked in (False, True):
        for p in params:
            p.grad = None
        qs = [m(sa) for m in critics]
        loss, stats = tqc_critic_loss(eng, torch.stack(qs, dim=1) if stacked else qs, torch.stack(nqs, dim=1) if stacked else nqs, d["rewards"], d["dones"],
                                      d["next_log_prob"], gamma=qr.GAMMA, top_quantiles_to_drop_per_net=drop, log_ent_coef=log_alpha)
        assert loss.dim() == 0 and loss.dtype == torch.float64 and loss.requires_grad and not stats.requires_grad
        loss.backward()
        eng.sync()
        worst = max(worst, _grad_share(params, ref))
        assert abs(float(loss.detach()) - ref_loss) <= 1e-12 * max(1.0, abs(ref_loss)) and float(stats[0]) == float(loss.detach())
    print(f"parameter gradients: max error / tolerance {worst:.2e}")
    assert worst <= 1.0
    # a float32 network: the loss comes back in float32, twice the loss gives twice the gradients
    net32 = torch.nn.Linear(41, K * Q).cuda()
    d32 = {k: _t(v) for k, v in qr.case(B, K, Q, drop, np.float32).items()}
    grads = []
    for scale in (1.0, 2.0):
        net32.zero_grad()
        loss, _ = tqc_critic_loss(eng, net32(sa.float()).view(B, K, Q), d32["next_quantiles"], d32["rewards"], d32["dones"], d32["next_log_prob"], gamma=qr.GAMMA,
                                  top_quantiles_to_drop_per_net=drop, ent_coef=0.2)
        assert loss.dtype == torch.float32
        (loss * scale).backward()
        grads.append(net32.weight.grad.clone())
    eng.sync()
    assert torch.equal(grads[0] * 2.0, grads[1]) and float(grads[0].abs().max()) > 0


# ------------------------------------------------------------------------------------------------- chains and streams
def test_behind_a_replay_chain_and_in_front_of_the_optimiser():
    """DeviceReplayBuffer.add -> sample -> two quantile critics -> tqc_critic_loss -> backward -> DeviceOptimizer.step(tau=0.005): the loss
    call reads what sample() delivered ([B, 1] columns, float32 rewards and dones beside float64 critics) bit for bit, and the step behind
    it moves parameters and targets"""
    import torch
    from rl_ptg_amd import DeviceOptimizer, DeviceReplayBuffer, tqc_critic_loss
    N, T, B, K, Q, drop = 64, 30, 290, 2, 30, 2
    eng = _engine(N, fresh=True)
    buf = DeviceReplayBuffer(eng, 25 * N, seed=3)
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    prev = eng.rows(eng.reset()).clone()
    acts = torch.randint(0, 5, (T, N), dtype=torch.int64, device="cuda", generator=g)
    obs, rew, done = eng.rollout(acts)
    buf.add(prev, obs[:25], rew[:25], done[:25], actions=acts[:25])
    s = buf.sample(B)
    torch.manual_seed(11)
    F = eng.obs_dim
    critics = [torch.nn.Linear(F + 1, Q).double().cuda() for _ in range(K)]
    targets = [torch.nn.Linear(F + 1, Q).double().cuda() for _ in range(K)]
    cp, tp = [p for m in critics for p in m.parameters()], [p for m in targets for p in m.parameters()]
    sa = torch.cat([s.observations.double(), s.actions.double()], dim=1)
    with torch.no_grad():
        nsa = torch.cat([s.next_observations.double(), ((s.actions + 1) % 5).double()], dim=1)
        nqs = [m(nsa) for m in targets]
        lp = -s.next_observations.double().abs().sum(dim=1) / F
    log_alpha = torch.tensor([LOG_ALPHA], dtype=torch.float64, device="cuda")
    qs = [m(sa) for m in critics]
    loss, stats = tqc_critic_loss(eng, qs, nqs, s.rewards, s.dones, lp, gamma=qr.GAMMA, top_quantiles_to_drop_per_net=drop, log_ent_coef=log_alpha)
    loss.backward()
    eng.sync()
    h = lambda t: t.detach().cpu().numpy()
    ref = qr.quantile_loss([h(q) for q in qs], [h(q) for q in nqs], h(s.rewards), h(s.dones), h(lp), qr.GAMMA, drop, _alpha_of(stats, "log", None))
    assert not ref["bad"].any() and s.rewards.dtype == torch.float32 and s.rewards.shape == (B, 1)
    e_means = _means_err(stats, ref)
    assert e_means <= 1.0
    ref_g = torch.autograd.grad(_torch_loss([m(sa) for m in critics], nqs, dict(rewards=s.rewards, dones=s.dones, next_log_prob=lp), qr.GAMMA, log_alpha.exp(), drop), cp)
    e_grads = _grad_share(cp, ref_g)
    print(f"replay chain B={B}: means, max error / tolerance {e_means:.2e}; parameter gradients {e_grads:.2e}")
    assert e_grads <= 1.0
    before, t_before = [p.detach().clone() for p in cp], [p.detach().clone() for p in tp]
    opt = DeviceOptimizer(eng, cp, kind="adam", lr=3e-4, targets=tp, tau=0.005, zero_grad=True)
    opt.step()
    eng.sync()
    for p, b, q, tb in zip(cp, before, tp, t_before):
        assert not torch.equal(p.detach(), b) and bool((p.grad == 0).all())
        want = (1.0 - 0.005) * tb + 0.005 * p.detach()
        assert float((q.detach() - want).abs().max()) <= 1e-15 * max(1.0, float(want.abs().max()))
    eng.close()


def test_on_a_side_stream():
    import torch
    eng = _engine()
    c = qr.case(9, 3, 33, 5, np.float64)
    side = torch.cuda.Stream()
    d = _device(c, 5, "wide")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = eng.quantile_loss(d["quantiles"], d["next_quantiles"], d["rewards"], d["dones"], d["next_log_prob"], qr.GAMMA, 5, ent_coef=0.2, want_target=True,
                                out=d["out"])
        eng.sync()
    torch.cuda.current_stream().wait_stream(side)
    ref = _ref(("side",), c, 5, 0.2)
    _same_bits(_grad_of(d, "wide"), ref["grad"])
    _same_bits(res.target, ref["y"])
    assert _means_err(res.stats, ref) <= 1.0


@pytest.mark.parametrize("B", [3, 290])
def test_captured_and_replayed_three_times_with_rewritten_inputs(B):
    """one launch (3 rows) and two (290) captured on a side stream with out= and workspace=, replayed three times with other quantiles,
    rewards, dones and log-probs written into the graph's inputs and another log alpha written into its device scalar; gamma and d stay.
    The hardware-queue setting is the machine's default"""
    import torch
    eng = _engine()
    K, Q, drop = 2, 30, 2
    cases = [qr.case(B, K, Q, drop, np.float32, seed=k) for k in range(4)]
    logs = [LOG_ALPHA, -0.25, 0.5, -3.0]
    d = _device(cases[0], drop, "stacked")
    la = torch.tensor([logs[0]], dtype=torch.float64, device="cuda")
    ws = eng.quantile_loss_workspace(B)
    run = lambda: eng.quantile_loss(d["quantiles"], d["next_quantiles"], d["rewards"], d["dones"], d["next_log_prob"], qr.GAMMA, drop, log_ent_coef=la,
                                    out=d["out"], workspace=ws)

    def load(k):
        for name, v in cases[k].items():
            d[name].copy_(_t(v))
        la.fill_(logs[k])

    def check(k):
        stats, grad, y = d["out"]
        ref = _ref(("graph", B, k), cases[k], drop, _alpha_of(stats, "log", None, logs[k]))
        _same_bits(grad, ref["grad"])
        _same_bits(y, ref["y"])
        assert _means_err(stats, ref) <= 1.0, k

    run()                                                    # eager once: code objects are loaded before the capture
    eng.sync()
    check(0)
    d["guards"][0].fill_(SENTINEL)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert bool((d["guards"][0] == SENTINEL).all())          # capturing enqueued nothing
    for k in (1, 2, 3):
        load(k)
        graph.replay()
        torch.cuda.synchronize()
        check(k)
        want = float(np.exp(logs[k]))
        print(f"B={B} replay {k}: exp({logs[k]}) is {abs(float(d['out'][0][5]) - want) / float(np.spacing(want)):.2f} spacings from np.exp")
    eng.sync()


def _equal_state(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_equal_state(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def test_no_host_synchronisation_no_allocation_and_nothing_else_touched():
    """A condition, not a timing: the stream is busy with milliseconds of fused steps before the calls and still busy when they have
    returned; with out= and workspace= the allocator hands out nothing during them.  Afterwards env state, finished ring, vn statistics
    and a replay cursor equal a twin's that made no call."""
    import torch
    from rl_ptg_amd import DeviceReplayBuffer
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    n, T, calls, B = 65536, 250, 8, 4096
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
    c = qr.case(B, 2, 30, 2, np.float32)
    ds, dl = _device(c, 2, "stacked"), _device(c, 2, "wide")
    la = torch.tensor([LOG_ALPHA], dtype=torch.float64, device="cuda")
    ws = eng.quantile_loss_workspace(B)
    one = lambda d, **kw: eng.quantile_loss(d["quantiles"], d["next_quantiles"], d["rewards"], d["dones"], d["next_log_prob"], qr.GAMMA, 2, out=d["out"],
                                            workspace=ws, **kw)
    both = lambda: (one(ds, ent_coef=qr.ALPHA), one(dl, log_ent_coef=la))
    obs, rew, done = eng.alloc_obs(T), torch.empty((T, n), device="cuda"), torch.empty((T, n), dtype=torch.uint8, device="cuda")
    eng.rollout(acts, obs, rew, done)                                            # warm: first-launch work is not part of the condition
    twin.rollout(acts)
    both()
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    assert stream.query() is True
    for _ in range(calls):
        eng.rollout(acts, obs, rew, done)
    busy_before = stream.query()
    allocs = torch.cuda.memory_stats()["allocation.all.allocated"]
    both()
    allocs_after = torch.cuda.memory_stats()["allocation.all.allocated"]
    busy_after = stream.query()
    assert busy_before is False, "the rollouts were over before the calls: the check would prove nothing"
    assert busy_after is False, "the stream was idle when the calls had returned: a call waited for the device"
    assert allocs_after == allocs, "a call with out= and workspace= allocated device memory"
    eng.sync()
    ref = _ref(("busy",), c, 2, qr.ALPHA)
    _same_bits(ds["out"][1], ref["grad"])
    assert _means_err(ds["out"][0], ref) <= 1.0
    for _ in range(calls):
        twin.rollout(acts)
    twin.sync()
    a, b = eng.state_dict(), twin.state_dict()
    assert _equal_state(a["fields"], b["fields"]) and _equal_state(a["vn"], b["vn"])
    assert buf.cursor() == (0, 0)
    assert len(eng.finished_episodes()[0]) == len(twin.finished_episodes()[0])
    eng.close(); twin.close()


# ------------------------------------------------------------------------------------------------- bad rows and refusals
def test_bad_rows():
    """planted as data, which the kernel must classify: a NaN current quantile, a +Inf reward, a -Inf next quantile (the lowest: it is
    kept), alpha = NaN in its three forms -- NaN gradients over the whole row, y as computed, statistics NaN, PTG_E_NONFINITE once; the
    other rows correct; a NaN and a +Inf among the dropped tops are NOT flagged; with d = 0 the same NaN is; a clean call syncs clean"""
    import torch
    from rl_ptg_amd import _lib
    from rl_ptg_amd.engine import PtgError
    eng = _engine()
    B, K, Q, drop = 290, 2, 30, 2                            # 73 blocks: the two-launch route

    def expect(code):
        with pytest.raises(PtgError) as ei:
            eng.sync()
        assert ei.value.code == code
        eng.sync()

    run = lambda d, drop=drop, **kw: eng.quantile_loss(d["quantiles"], d["next_quantiles"], d["rewards"], d["dones"], d["next_log_prob"], qr.GAMMA, drop,
                                                       want_target=True, out=d["out"], **kw)
    for dt, form in zip(qr.DTYPES, ("wide", "stacked")):
        c = qr.case(B, K, Q, drop, dt)                        # rows 8 and 9 hold a NaN and a +Inf among the dropped tops: legal
        d = _device(c, drop, form)
        res = run(d, ent_coef=0.2)
        eng.sync()                                           # not flagged
        ref = _ref(("bad", dt, "legal"), c, drop, 0.2)
        assert not ref["bad"].any() and bool(torch.isfinite(res.stats).all())
        _same_bits(_grad_of(d, form), ref["grad"]); _same_bits(res.target, ref["y"])
        c["quantiles"][20, 1, 7] = np.nan
        c["rewards"][277] = np.inf
        c["next_quantiles"][30, 0, 3] = -np.inf
        c["dones"][30] = 0.0
        d = _device(c, drop, form)
        res = run(d, ent_coef=0.2)
        expect(_lib.E_NONFINITE)
        ref = _ref(("bad", dt, "planted"), c, drop, 0.2)
        assert np.nonzero(ref["bad"])[0].tolist() == [20, 30, 277]
        grad = _grad_of(d, form)
        _same_bits(grad, ref["grad"]); _same_bits(res.target, ref["y"])
        rows_nan = torch.isnan(grad).reshape(B, -1)
        assert int(rows_nan.all(dim=1).sum()) == 3 and int(rows_nan.any(dim=1).sum()) == 3
        assert bool(torch.isnan(res.stats[:5]).all()) and float(res.stats[5]) == 0.2
        assert bool((res.target[277] == np.inf).all()) and float(res.target[30, 0]) == -np.inf and bool(torch.isfinite(res.target[30, 1:]).all())
        _guards_untouched(d, form)
        c = qr.case(B, K, Q, drop, dt)                        # d = 0 keeps everything: the NaN of row 8 and the +Inf of row 9 now count
        d = _device(c, 0, form)
        res = run(d, drop=0, ent_coef=0.2)
        expect(_lib.E_NONFINITE)
        ref = _ref(("bad", dt, "d0"), c, 0, 0.2)
        assert np.nonzero(ref["bad"])[0].tolist() == [8, 9]
        _same_bits(_grad_of(d, form), ref["grad"]); _same_bits(res.target, ref["y"])
        small = {k: v[:3].copy() for k, v in c.items()}      # the one-launch route
        small["quantiles"][1, 0, 0] = np.inf
        d = _device(small, drop, form)
        res = run(d, ent_coef=0.2)
        expect(_lib.E_NONFINITE)
        ref = _ref(("bad", dt, "small"), small, drop, 0.2)
        assert np.nonzero(ref["bad"])[0].tolist() == [1] and bool(torch.isnan(res.stats[:5]).all())
        _same_bits(_grad_of(d, form), ref["grad"]); _same_bits(res.target, ref["y"])
        for kw in (dict(ent_coef=float("nan")), dict(ent_coef=torch.tensor([np.nan], dtype=torch.float64, device="cuda")),
                   dict(log_ent_coef=torch.tensor([np.nan], dtype=torch.float64, device="cuda"))):      # alpha = NaN: every row that is not done
            c = qr.case(B, K, Q, drop, dt)
            c["dones"][:] = 0.0
            d = _device(c, drop, form)
            res = run(d, **kw)
            expect(_lib.E_NONFINITE)
            assert bool(torch.isnan(_grad_of(d, form)).all()) and bool(torch.isnan(res.target).all()) and bool(torch.isnan(res.stats[:6]).all())
    c = qr.case(B, K, Q, drop, np.float32)
    d = _device(c, drop, "list")
    res = run(d, ent_coef=0.2)                                # a clean call syncs clean
    eng.sync()
    assert bool(torch.isfinite(res.stats).all())


def test_refused_arguments_enqueue_nothing():
    import torch
    from rl_ptg_amd import _lib
    eng = _engine()
    B, K, Q, drop = 290, 2, 30, 2
    L, h, stream = eng._L, eng._h, eng._stream()
    d = _device(qr.case(B, K, Q, drop, np.float32), drop, "wide")
    a64 = torch.tensor([0.2], dtype=torch.float64, device="cuda")
    ws = eng.quantile_loss_workspace(B)
    ws.fill_(0x5A)
    torch.cuda.synchronize()
    ptrs = lambda xs: [x.data_ptr() for x in xs]

    def desc(**kw):
        a = dict(flags=0, n_critics=K, n_quantiles=Q, n_drop=drop, q_dtype=_lib.OUT_F32, rew_dtype=_lib.OUT_F32, done_dtype=_lib.OUT_F32, batch=B,
                 cur_dev=ptrs(d["quantiles"]), cur_s_n=[Q + 1] * K, next_dev=ptrs(d["next_quantiles"]), next_s_n=[Q + 1] * K,
                 grad_dev=ptrs(d["out"][1]), g_s_n=[Q + 1] * K, rew_dev=d["rewards"].data_ptr(), done_dev=d["dones"].data_ptr(),
                 next_logp_dev=d["next_log_prob"].data_ptr(), gamma=qr.GAMMA, alpha=0.2, stats_dev=d["out"][0].data_ptr(), y_dev=d["out"][2].data_ptr(),
                 ws_dev=ws.data_ptr())
        a.update(kw)
        ds = _lib.PtgQl()
        for k, v in a.items():
            if isinstance(v, (list, tuple)):
                for j, x in enumerate(v):
                    getattr(ds, k)[j] = x
            else:
                setattr(ds, k, v)
        return ds

    q0, q1 = ptrs(d["quantiles"])
    bad = [desc(cur_dev=[q0, None]), desc(next_dev=[None, q1]), desc(grad_dev=[None, None]), desc(rew_dev=None), desc(done_dev=None), desc(next_logp_dev=None),
           desc(stats_dev=None), desc(ws_dev=None), desc(ws_dev=ws.data_ptr() + 4), desc(flags=2), desc(flags=4), desc(flags=-1), desc(flags=_lib.QL_LOG_ALPHA),
           desc(q_dtype=2), desc(q_dtype=-1), desc(rew_dtype=2), desc(done_dtype=3), desc(n_critics=0), desc(n_critics=5), desc(n_critics=-1),
           desc(n_quantiles=0), desc(n_quantiles=65, cur_s_n=[65, 65], next_s_n=[65, 65], g_s_n=[65, 65]), desc(n_quantiles=-3), desc(n_drop=-1), desc(n_drop=Q),
           desc(n_drop=Q + 5), desc(batch=0), desc(batch=-3), desc(batch=2 ** 31 + 1), desc(batch=2 ** 40), desc(cur_s_n=[Q + 1, Q - 1]), desc(next_s_n=[Q - 1, Q + 1]),
           desc(g_s_n=[Q + 1, Q - 1]), desc(cur_s_n=[0, Q]), desc(g_s_n=[-1, Q])]
    for k, ds in enumerate(bad):
        assert L.ptg_quantile_loss(h, C.byref(ds), stream) == _lib.E_INVALID, k
        assert b"ptg_quantile_loss" in L.ptg_last_error(h)
        assert torch.cuda.current_stream().query() is True, k
    assert L.ptg_quantile_loss(h, None, stream) == _lib.E_INVALID and L.ptg_quantile_loss(None, C.byref(desc()), stream) == _lib.E_INVALID
    assert torch.cuda.current_stream().query() is True
    assert all(bool((g == SENTINEL).all()) for g in d["guards"]) and bool((d["out"][0] == SENTINEL).all()) and bool((d["out"][2] == SENTINEL).all())
    assert bool((ws == 0x5A).all())
    good = [desc(), desc(y_dev=None), desc(batch=1), desc(batch=4), desc(reserved=77), desc(alpha_dev=a64.data_ptr()),
            desc(flags=_lib.QL_LOG_ALPHA, alpha_dev=a64.data_ptr()), desc(n_critics=1, cur_dev=[q0, None]), desc(n_drop=1, y_dev=None), desc(n_drop=Q - 1)]      # rows 8 and 9 hold a NaN and a +Inf: d >= 1 drops them
    for k, ds in enumerate(good):
        assert L.ptg_quantile_loss(h, C.byref(ds), stream) == 0, (k, L.ptg_last_error(h))
    eng.sync()
    assert bool(torch.isfinite(d["out"][0]).all())
