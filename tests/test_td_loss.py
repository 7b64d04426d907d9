"""ptg_td_loss, HipEngine.td_loss and rl_ptg_amd.loss's dqn_loss / td3_critic_loss / sac_critic_loss (include/ptg_env.h) -- the TD
target, the loss of DQN or of the TD3 / SAC critics, five statistics and the gradients with respect to the current Q-values in one
pass -- against the NumPy restatement (tests/td_loss_restatement.py, pinned against torch autograd by tests/test_td_loss_host.py).

Bounds, derived and not measured.  The per-row outputs (the target y and every gradient) hold no reduction and no transcendental:
float64 arithmetic in the header's operand order, every operation rounded once.  They are compared BIT FOR BIT through integer views:
float64 outputs equal the restatement, float32 outputs equal the restatement rounded once.  With a log alpha on the device the
restatement is fed the alpha the kernel reports in stats[5], which itself is held to np.exp within 2 float64 spacings (1 ulp is the
published error of the device library's double exp, NumPy's libm is within 1 ulp of the true value too).
  every mean         within (B * 2^-53 + 1e-12) * max(1, mean |term|): summation of the terms in any order plus the per-term bound
  stats[4]           exact: a count divided once
Each test prints its measured maxima in units of its tolerance."""
import ctypes as C

import numpy as np
import pytest

import td_loss_restatement as tr

pytestmark = pytest.mark.gpu

SENTINEL = 7.5
ALPHA, LOG_ALPHA = 0.2173, -1.3125
_engines = {}
_spec = []
RD_DTYPES = [(np.float32, np.float32), (np.float64, np.float32), (np.float32, np.float64), (np.float64, np.float64)]      # rewards, dones
MODES = ["td3", "sac_host", "sac_dev", "sac_log"]
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


def _same_bits(got, ref64, skip=None):
    """a per-row output against the restatement rounded once to the output's dtype, through integer views; rows in skip (untouched by
    the kernel) are left out; a NaN must meet a NaN"""
    got = got.detach().cpu().numpy()
    ref = np.asarray(ref64, np.float64).reshape(got.shape).astype(got.dtype)
    if skip is not None:
        got, ref = got[~skip], ref[~skip]
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    iv = np.int32 if got.dtype == np.float32 else np.int64
    assert np.array_equal(got[~nan].view(iv), ref[~nan].view(iv)), float(np.abs(got[~nan].astype(np.float64) - ref[~nan]).max())


def _means_err(stats, ref, B):
    """max error of stats[0..3] in units of their tolerance; stats[4] and the tail must be exact"""
    got, want, am = stats.cpu().numpy(), ref["stats"], ref["abs_mean"]
    u = B * 2.0 ** -53 + 1e-12
    e = [abs(got[i] - want[i]) / (u * max(1.0, am[k])) for i, k in enumerate(("loss", "q", "y", "abs_delta"))]
    assert got[4] == want[4] and got[6] == 0.0 and got[7] == 0.0, (got, want)
    return max(e)


# ------------------------------------------------------------------------------------------------- DQN
def _dqn_device(c, wide):
    """host case -> device tensors and out=; wide: q, next_q and the gradient are the first A columns of [B, A + 1] tensors whose last
    column is a guard (the gradient also has a guard row above and below)"""
    import torch
    B, A = c["q"].shape
    d = {k: _t(v) for k, v in c.items()}
    dt = d["q"].dtype
    if wide:
        for k in ("q", "next_q"):
            w = _full((B, A + 1), dt)
            w[:, :A] = d[k]
            d[k + "_wide"], d[k] = w, w[:, :A]
        g = _full((B + 2, A + 1), dt)
        d["guard"], grad = g, g[1:B + 1, :A]
    else:
        grad = _full((B, A), dt)
    d["out"] = (_full((8,), torch.float64), grad, _full((B,), dt))
    return d


def _check_dqn(eng, c, wide, gamma=tr.GAMMA["dqn"], ws=None):
    import torch
    B, A = c["q"].shape
    d = _dqn_device(c, wide)
    res = eng.td_loss("dqn", d["q"], d["next_q"], d["rewards"], d["dones"], gamma, actions=d["actions"], want_target=True, out=d["out"], workspace=ws)
    eng.sync()
    ref = tr.td_loss("dqn", c["q"], c["next_q"], c["rewards"], c["dones"], gamma, actions=c["actions"])
    assert not ref["bad"].any() and not ref["oob"].any() and res.stats is d["out"][0]
    _same_bits(res.grad_q, ref["grad_q"])
    _same_bits(res.target, ref["y"])
    assert float(res.stats[5]) == 0.0
    if wide:
        g = d["guard"]
        assert bool((g[0] == SENTINEL).all()) and bool((g[-1] == SENTINEL).all()) and bool((g[:, A] == SENTINEL).all())
        assert bool((d["q_wide"][:, A] == SENTINEL).all()) and bool((d["next_q_wide"][:, A] == SENTINEL).all())
    return _means_err(res.stats, ref, B)


@pytest.mark.parametrize("B", tr.BS)
def test_dqn_over_every_shape(B):
    """B at 1, 2, around the wave, around the edge between the one-launch and the two-launch route (256 | 257), DQN's 544 and a ragged
    last block; A in {2, 5, 32}; float32 and float64 Q; int32 and int64 actions; row stride A and A + 1 (guard columns untouched);
    float32 / float64 rewards and dones, each on its own; the planted rows of tests/td_loss_restatement.py"""
    eng = _engine()
    worst = 0.0
    for A in tr.AS:
        for dt in tr.DTYPES:
            for adt in (np.int32, np.int64):
                for rdt, ddt in RD_DTYPES:
                    c = tr.dqn_case(B, A, dt, rdt=rdt, ddt=ddt, adt=adt)
                    for wide in (False, True):
                        worst = max(worst, _check_dqn(eng, c, wide))
    print(f"dqn B={B}: means, max error / tolerance {worst:.4f}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------- the critics
def _critics_device(c, cols):
    """cols: the current critics, the target critics and the gradients are columns of one [B, K] tensor each (the gradients with a
    guard column and guard rows); else SB3's tuples: [B, 1] tensors for the current critics, [B] for the targets, and a mix as gradients"""
    import torch
    K, B = len(c["q"]), c["rewards"].shape[0]
    d = {k: _t(v) for k, v in c.items() if k not in ("q", "next_q")}
    dt = _t(c["q"][0]).dtype
    if cols:
        Q, NQ = _t(np.stack(c["q"], axis=1)), _t(np.stack(c["next_q"], axis=1))
        g = _full((B + 2, K + 1), dt)
        d["q"], d["next_q"], d["guard"] = [Q[:, k] for k in range(K)], [NQ[:, k] for k in range(K)], g
        grads = [g[1:B + 1, k] for k in range(K)]
    else:
        d["q"], d["next_q"] = [_t(x).view(-1, 1) for x in c["q"]], [_t(x) for x in c["next_q"]]
        grads = [_full((B, 1), dt) if k % 2 == 0 else _full((B,), dt) for k in range(K)]
    d["out"] = (_full((8,), torch.float64), grads, _full((B,), dt))
    return d


def _mode_kw(mode):
    import torch
    if mode == "td3":
        return "td3", {}, None
    if mode == "sac_host":
        return "sac", dict(ent_coef=ALPHA), ALPHA
    if mode == "sac_dev":
        return "sac", dict(ent_coef=torch.tensor([ALPHA], dtype=torch.float64, device="cuda")), ALPHA
    return "sac", dict(log_ent_coef=torch.tensor([LOG_ALPHA], dtype=torch.float64, device="cuda")), None


def _alpha_of(stats, mode, alpha, log_alpha=LOG_ALPHA):
    """the alpha the restatement is fed: the given one, which stats[5] must equal -- or, for a log alpha, the kernel's own stats[5],
    held to np.exp within 2 float64 spacings"""
    got = float(stats[5])
    if mode == "td3":
        assert got == 0.0
        return None
    if mode != "sac_log":
        assert got == alpha
        return alpha
    want = float(np.exp(log_alpha))
    dist = abs(got - want) / float(np.spacing(want))
    _worst["exp_spacings"] = max(_worst["exp_spacings"], dist)
    assert dist <= 2.0, (got, want)
    return got


def _check_critics(eng, c, cols, mode, ws=None):
    import torch
    K, B = len(c["q"]), c["rewards"].shape[0]
    kind, kw, alpha = _mode_kw(mode)
    gamma = tr.GAMMA[kind]
    d = _critics_device(c, cols)
    res = eng.td_loss(kind, d["q"], d["next_q"], d["rewards"], d["dones"], gamma, next_log_prob=d["next_log_prob"] if kind == "sac" else None,
                      want_target=True, out=d["out"], workspace=ws, **kw)
    eng.sync()
    ref = tr.td_loss(kind, c["q"], c["next_q"], c["rewards"], c["dones"], gamma, next_log_prob=c["next_log_prob"], alpha=_alpha_of(res.stats, mode, alpha))
    assert not ref["bad"].any() and res.grad_q is d["out"][1]
    for k in range(K):
        _same_bits(res.grad_q[k], ref["grad_q"][k])
    _same_bits(res.target, ref["y"])
    if cols:
        g = d["guard"]
        assert bool((g[0] == SENTINEL).all()) and bool((g[-1] == SENTINEL).all()) and bool((g[:, K] == SENTINEL).all())
    return _means_err(res.stats, ref, B)


@pytest.mark.parametrize("B", tr.BS)
def test_critics_over_every_shape(B):
    """the same batch sizes; K in {1, 2, 4}; separate tensors and columns of one [B, K] tensor; TD3 (c = 1), SAC (c = 1/2) with a host
    alpha, a device alpha and a device log alpha; float32 and float64 Q; float32 / float64 rewards and dones"""
    eng = _engine()
    worst = 0.0
    for K in tr.KS:
        for dt in tr.DTYPES:
            for rdt, ddt in RD_DTYPES:
                c = tr.critics_case(B, K, dt, rdt=rdt, ddt=ddt)
                for cols in (False, True):
                    for mode in MODES:
                        worst = max(worst, _check_critics(eng, c, cols, mode))
    print(f"critics B={B}: means, max error / tolerance {worst:.4f}; exp(log alpha) against np.exp: {_worst['exp_spacings']:.2f} spacings")
    assert worst <= 1.0


@pytest.mark.parametrize("kind", ["dqn", "td3", "sac"])
def test_a_batch_that_crosses_the_partial_boundaries(kind):
    """70 001 rows = 274 blocks of 256: the final kernel's 256 threads walk the block partials in laps of 256, so 18 threads take a second
    partial; the last block is ragged (113 rows, its last wave 49)"""
    eng = _engine()
    worst = 0.0
    for dt in tr.DTYPES:
        if kind == "dqn":
            worst = max(worst, _check_dqn(eng, tr.dqn_case(tr.B_BIG, 5, dt, rdt=dt), True))
        else:
            worst = max(worst, _check_critics(eng, tr.critics_case(tr.B_BIG, 2, dt, rdt=dt), True, "td3" if kind == "td3" else "sac_log"))
    print(f"{kind} B={tr.B_BIG}: means, max error / tolerance {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("kind", ["dqn", "td3"])
def test_thread_0_of_the_final_pass_adds_two_partials(kind):
    """65 793 rows = 256 * 257 + 1: more than 256 block partials, so thread 0 of the final kernel adds the partials of blocks 0 and 256
    before the block's tree; the last block holds one row.  float32, the smallest A and K of the sweeps."""
    eng = _engine()
    B = 256 * 257 + 1
    if kind == "dqn":
        worst = _check_dqn(eng, tr.dqn_case(B, tr.AS[0], np.float32), False)
    else:
        worst = _check_critics(eng, tr.critics_case(B, tr.KS[0], np.float32), False, "td3")
    print(f"{kind} B={B}: means, max error / tolerance {worst:.4f}")
    assert worst <= 1.0


def test_two_runs_give_identical_bits():
    import torch
    eng = _engine()
    for B in (544, tr.B_BIG):
        c = tr.dqn_case(B, 5, np.float32)
        runs = []
        for _ in range(2):
            d = _dqn_device(c, True)
            res = eng.td_loss("dqn", d["q"], d["next_q"], d["rewards"], d["dones"], 0.97, actions=d["actions"], out=d["out"])
            eng.sync()
            runs.append((res.stats.clone(), d["guard"].clone(), res.target.clone()))
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(*runs)) and bool(torch.isfinite(runs[0][0]).all())
        c = tr.critics_case(B, 2, np.float64)
        runs = []
        for _ in range(2):
            d = _critics_device(c, True)
            res = eng.td_loss("sac", d["q"], d["next_q"], d["rewards"], d["dones"], 0.96, next_log_prob=d["next_log_prob"],
                              log_ent_coef=torch.tensor([LOG_ALPHA], dtype=torch.float64, device="cuda"), out=d["out"])
            eng.sync()
            runs.append((res.stats.clone(), d["guard"].clone(), res.target.clone()))
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(*runs)) and bool(torch.isfinite(runs[0][0]).all())


# ------------------------------------------------------------------------------------------------- the autograd wrappers
def _sb3_dqn(q_values, next_q, d, gamma):
    """SB3's lines on the device; the float32 columns of a replay sample are widened first (torch would keep (1 - dones) * gamma in
    float32, gamma rounded with it)"""
    import torch
    import torch.nn.functional as F
    with torch.no_grad():
        nq, _ = next_q.max(dim=1)
        target = d["rewards"].double().reshape(-1, 1) + (1 - d["dones"].double().reshape(-1, 1)) * gamma * nq.reshape(-1, 1)
    return F.smooth_l1_loss(torch.gather(q_values, dim=1, index=d["actions"].long().reshape(-1, 1)), target)


def _sb3_critics(kind, qs, next_qs, d, gamma, alpha):
    import torch
    import torch.nn.functional as F
    with torch.no_grad():
        nq, _ = torch.min(torch.cat(next_qs, dim=1), dim=1, keepdim=True)
        if kind == "sac":
            nq = nq - alpha * d["next_log_prob"].reshape(-1, 1)
        target = d["rewards"].double().reshape(-1, 1) + (1 - d["dones"].double().reshape(-1, 1)) * gamma * nq
    loss = sum(F.mse_loss(q, target) for q in qs)
    return 0.5 * loss if kind == "sac" else loss


def _grad_share(params, ref):
    return max(float((p.grad - r).abs().max()) / (1e-12 * max(1.0, float(r.abs().max()))) for p, r in zip(params, ref))


def test_the_wrappers_drive_networks_as_torch_autograd_does():
    """a float64 Linear(40, A) for DQN, two Linear(41, 1) critics for TD3 and SAC: after loss.backward() through rl_ptg_amd.loss the
    parameter gradients equal those of SB3's lines under torch autograd on the device within 1e-12 * max(1, max |ref|); the loss too"""
    import torch
    from rl_ptg_amd import dqn_loss, sac_critic_loss, td3_critic_loss
    eng = _engine()
    B, A = 544, 5
    torch.manual_seed(7)
    f64 = dict(dtype=torch.float64, device="cuda")
    obs, nobs = torch.randn(B, 40, **f64), torch.randn(B, 40, **f64)
    c = tr.dqn_case(B, A, np.float64)
    d = {k: _t(v) for k, v in c.items()}
    net, tgt = torch.nn.Linear(40, A).double().cuda(), torch.nn.Linear(40, A).double().cuda()
    gamma = tr.GAMMA["dqn"]
    with torch.no_grad():
        nq = tgt(nobs)
    _sb3_dqn(net(obs), nq, d, gamma).backward()
    ref = [p.grad.clone() for p in net.parameters()]
    ref_loss = float(_sb3_dqn(net(obs), nq, d, gamma).detach())
    net.zero_grad()
    loss, stats = dqn_loss(eng, net(obs), nq, d["actions"], d["rewards"], d["dones"], gamma=gamma)
    assert loss.dim() == 0 and loss.dtype == torch.float64 and loss.requires_grad and not stats.requires_grad
    loss.backward()
    eng.sync()
    worst = _grad_share(net.parameters(), ref)
    assert abs(float(loss.detach()) - ref_loss) <= 1e-12 * max(1.0, abs(ref_loss)) and float(stats[0]) == float(loss.detach())
    # the critics: (s, a) -> Q through two Linear(41, 1)
    c = tr.critics_case(B, 2, np.float64)
    d = {k: _t(v) for k, v in c.items() if k not in ("q", "next_q")}
    sa, nsa = torch.randn(B, 41, **f64), torch.randn(B, 41, **f64)
    critics = [torch.nn.Linear(41, 1).double().cuda() for _ in range(2)]
    targets = [torch.nn.Linear(41, 1).double().cuda() for _ in range(2)]
    params = [p for m in critics for p in m.parameters()]
    log_alpha = torch.tensor([LOG_ALPHA], **f64)
    with torch.no_grad():
        nqs = [m(nsa) for m in targets]
    for kind in ("td3", "sac"):
        gamma = tr.GAMMA[kind]
        for p in params:
            p.grad = None
        _sb3_critics(kind, [m(sa) for m in critics], nqs, d, gamma, log_alpha.exp()).backward()
        ref = [p.grad.clone() for p in params]
        ref_loss = float(_sb3_critics(kind, [m(sa) for m in critics], nqs, d, gamma, log_alpha.exp()).detach())
        for p in params:
            p.grad = None
        if kind == "td3":
            loss, stats = td3_critic_loss(eng, [m(sa) for m in critics], nqs, d["rewards"], d["dones"], gamma=gamma)
        else:
            loss, stats = sac_critic_loss(eng, [m(sa) for m in critics], nqs, d["rewards"], d["dones"], d["next_log_prob"], gamma=gamma, log_ent_coef=log_alpha)
        loss.backward()
        eng.sync()
        worst = max(worst, _grad_share(params, ref))
        assert abs(float(loss.detach()) - ref_loss) <= 1e-12 * max(1.0, abs(ref_loss)), kind
    print(f"parameter gradients: max error / tolerance {worst:.4f}")
    assert worst <= 1.0
    # a float32 network: the loss comes back in float32, twice the loss gives twice the gradients, a refused row adds nothing
    net32 = torch.nn.Linear(40, A).cuda()
    d = {k: _t(v) for k, v in tr.dqn_case(B, A, np.float32).items()}
    grads = []
    for scale in (1.0, 2.0):
        net32.zero_grad()
        loss, _ = dqn_loss(eng, net32(obs.float()), nq.float(), d["actions"], d["rewards"], d["dones"], gamma=0.97)
        assert loss.dtype == torch.float32
        (loss * scale).backward()
        grads.append(net32.weight.grad.clone())
    eng.sync()
    assert torch.equal(grads[0] * 2.0, grads[1]) and float(grads[0].abs().max()) > 0
    # a row refused for its action: the wrapper's fresh gradients are zeroed, so the row adds nothing -- on a leaf Q its gradient row is
    # zero, and a network's weight gradient is that of the other rows alone
    from rl_ptg_amd import _lib
    from rl_ptg_amd.engine import PtgError
    acts = d["actions"].clone()
    acts[3] = A
    q_leaf = net32(obs.float()).detach().requires_grad_(True)
    loss, stats = dqn_loss(eng, q_leaf, nq.float(), acts, d["rewards"], d["dones"], gamma=0.97)
    loss.backward()
    with pytest.raises(PtgError) as ei:
        eng.sync()
    assert ei.value.code == _lib.E_INDEX and bool(torch.isnan(stats[:5]).all())
    assert bool((q_leaf.grad[3] == 0).all()) and int((q_leaf.grad != 0).any(dim=1).sum()) >= B - 2 and bool(torch.isfinite(q_leaf.grad).all())
    net32.zero_grad()
    loss, _ = dqn_loss(eng, net32(obs.float()), nq.float(), acts, d["rewards"], d["dones"], gamma=0.97)
    loss.backward()
    with pytest.raises(PtgError):
        eng.sync()
    got = net32.weight.grad.clone()
    net32.zero_grad()
    net32(obs.float()).backward(q_leaf.grad)                # the leaf's gradient rows, row 3 being zero, through the same network
    eng.sync()
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    assert float((got - net32.weight.grad).abs().max()) <= 1e-6 * float(got.abs().max())


# ------------------------------------------------------------------------------------------------- chains and streams
def test_behind_a_replay_chain_and_in_front_of_the_optimiser():
    """DeviceReplayBuffer.add -> sample -> two critics -> sac_critic_loss -> backward -> DeviceOptimizer.step(tau): the loss call
    reads what sample() delivered ([B, 1] columns, float32 rewards and dones beside float64 critics) bit for bit, and the step behind it
    moves parameters and targets"""
    import torch
    from rl_ptg_amd import DeviceOptimizer, DeviceReplayBuffer, sac_critic_loss
    N, T, B = 64, 30, 470
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
    critics = [torch.nn.Linear(F + 1, 1).double().cuda() for _ in range(2)]
    targets = [torch.nn.Linear(F + 1, 1).double().cuda() for _ in range(2)]
    cp, tp = [p for m in critics for p in m.parameters()], [p for m in targets for p in m.parameters()]
    sa = torch.cat([s.observations.double(), s.actions.double()], dim=1)
    with torch.no_grad():
        nsa = torch.cat([s.next_observations.double(), ((s.actions + 1) % 5).double()], dim=1)
        nqs = [m(nsa) for m in targets]
        lp = -s.next_observations.double().abs().sum(dim=1) / F
    log_alpha = torch.tensor([LOG_ALPHA], dtype=torch.float64, device="cuda")
    qs = [m(sa) for m in critics]
    loss, stats = sac_critic_loss(eng, qs, nqs, s.rewards, s.dones, lp, gamma=tr.GAMMA["sac"], log_ent_coef=log_alpha)
    loss.backward()
    eng.sync()
    h = lambda t: t.detach().cpu().numpy().reshape(-1)
    ref = tr.td_loss("sac", [h(q) for q in qs], [h(q) for q in nqs], h(s.rewards), h(s.dones), tr.GAMMA["sac"], next_log_prob=h(lp), alpha=float(stats[5]))
    assert not ref["bad"].any() and s.rewards.dtype == torch.float32 and s.rewards.shape == (B, 1)
    e_means = _means_err(stats, ref, B)
    assert e_means <= 1.0
    ref_g = torch.autograd.grad(_sb3_critics("sac", [m(sa) for m in critics], nqs, dict(rewards=s.rewards.double(), dones=s.dones.double(), next_log_prob=lp),
                                             tr.GAMMA["sac"], log_alpha.exp()), cp)
    e_grads = _grad_share(cp, ref_g)
    print(f"replay chain B={B}: means, max error / tolerance {e_means:.4f}; parameter gradients {e_grads:.4f}")
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
    c = tr.dqn_case(257, 5, np.float64)
    side = torch.cuda.Stream()
    d = _dqn_device(c, True)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = eng.td_loss("dqn", d["q"], d["next_q"], d["rewards"], d["dones"], 0.97, actions=d["actions"], want_target=True, out=d["out"])
        eng.sync()
    torch.cuda.current_stream().wait_stream(side)
    ref = tr.td_loss("dqn", c["q"], c["next_q"], c["rewards"], c["dones"], 0.97, actions=c["actions"])
    _same_bits(res.grad_q, ref["grad_q"])
    assert _means_err(res.stats, ref, 257) <= 1.0


@pytest.mark.parametrize("B", [203, 544])
def test_captured_and_replayed_three_times_with_rewritten_inputs(B):
    """one launch (203) and two (544) captured on a side stream with out= and workspace=, replayed three times with other Q-values,
    rewards, dones and log-probs written into the graph's inputs and another log alpha written into its device scalar; gamma stays"""
    import torch
    eng = _engine()
    K = 2
    cases = [tr.critics_case(B, K, np.float32, seed=k) for k in range(4)]
    logs = [LOG_ALPHA, -0.25, 0.5, -3.0]
    d = _critics_device(cases[0], True)
    la = torch.tensor([logs[0]], dtype=torch.float64, device="cuda")
    ws = eng.td_loss_workspace(B)
    gamma = tr.GAMMA["sac"]
    run = lambda: eng.td_loss("sac", d["q"], d["next_q"], d["rewards"], d["dones"], gamma, next_log_prob=d["next_log_prob"], log_ent_coef=la,
                              out=d["out"], workspace=ws)

    def load(k):
        src = _critics_device(cases[k], True)
        for j in range(K):
            d["q"][j].copy_(src["q"][j]); d["next_q"][j].copy_(src["next_q"][j])
        for name in ("rewards", "dones", "next_log_prob"):
            d[name].copy_(src[name])
        la.fill_(logs[k])

    def check(k):
        stats, grads, y = d["out"]
        c = cases[k]
        ref = tr.td_loss("sac", c["q"], c["next_q"], c["rewards"], c["dones"], gamma, next_log_prob=c["next_log_prob"], alpha=_alpha_of(stats, "sac_log", None, logs[k]))
        for j in range(K):
            _same_bits(grads[j], ref["grad_q"][j])
        _same_bits(y, ref["y"])
        assert _means_err(stats, ref, B) <= 1.0, k

    run()                                                    # eager once: code objects are loaded before the capture
    eng.sync()
    check(0)
    d["guard"].fill_(SENTINEL)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert bool((d["guard"] == SENTINEL).all())              # capturing enqueued nothing
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
    n, T, calls = 65536, 250, 8
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
    c, cc = tr.dqn_case(n, 5, np.float32), tr.critics_case(n, 2, np.float32)
    d, dc = _dqn_device(c, True), _critics_device(cc, True)
    la = torch.tensor([LOG_ALPHA], dtype=torch.float64, device="cuda")
    ws = eng.td_loss_workspace(n)
    dqn = lambda: eng.td_loss("dqn", d["q"], d["next_q"], d["rewards"], d["dones"], 0.97, actions=d["actions"], out=d["out"], workspace=ws)
    sac = lambda: eng.td_loss("sac", dc["q"], dc["next_q"], dc["rewards"], dc["dones"], 0.96, next_log_prob=dc["next_log_prob"], log_ent_coef=la,
                              out=dc["out"], workspace=ws)
    obs, rew, done = eng.alloc_obs(T), torch.empty((T, n), device="cuda"), torch.empty((T, n), dtype=torch.uint8, device="cuda")
    eng.rollout(acts, obs, rew, done)                                            # warm: first-launch work is not part of the condition
    twin.rollout(acts)
    dqn(); sac()
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    assert stream.query() is True
    for _ in range(calls):
        eng.rollout(acts, obs, rew, done)
    busy_before = stream.query()
    allocs = torch.cuda.memory_stats()["allocation.all.allocated"]
    dqn(); sac()
    allocs_after = torch.cuda.memory_stats()["allocation.all.allocated"]
    busy_after = stream.query()
    assert busy_before is False, "the rollouts were over before the calls: the check would prove nothing"
    assert busy_after is False, "the stream was idle when the calls had returned: a call waited for the device"
    assert allocs_after == allocs, "a call with out= and workspace= allocated device memory"
    eng.sync()
    ref = tr.td_loss("dqn", c["q"], c["next_q"], c["rewards"], c["dones"], 0.97, actions=c["actions"])
    _same_bits(d["out"][1], ref["grad_q"])
    assert _means_err(d["out"][0], ref, n) <= 1.0
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
    """planted as data, which the kernel must classify: an action of -1 and of A (the row's gradients and y untouched, PTG_E_INDEX
    once); a NaN in a non-maximal next-Q column, a +Inf reward, alpha = NaN (NaN gradients, y as computed, PTG_E_NONFINITE once); the
    other rows correct; statistics NaN; the legal rows legal; a clean call syncs clean"""
    import torch
    from rl_ptg_amd import _lib
    from rl_ptg_amd.engine import PtgError
    eng = _engine()
    B, A = 300, 5                                            # two blocks: the two-launch route

    def expect(code, then_clean=True):
        with pytest.raises(PtgError) as ei:
            eng.sync()
        assert ei.value.code == code
        if then_clean:
            eng.sync()

    for dt in tr.DTYPES:
        c = tr.dqn_case(B, A, dt)
        a = c["actions"]
        for r in (20, 277):                                  # a NaN beside the maximum, on a row of either block
            c["next_q"][r, (int(np.argmax(c["next_q"][r])) + 1) % A] = np.nan
        c["rewards"][30] = np.inf
        c["q"][40, a[40]] = -np.inf
        c["next_q"][50, (int(np.argmax(c["next_q"][50])) + 1) % A] = -np.inf      # legal
        c["q"][60, (a[60] + 1) % A] = np.nan                                        # legal: not read
        d = _dqn_device(c, True)
        run = lambda d: eng.td_loss("dqn", d["q"], d["next_q"], d["rewards"], d["dones"], 0.97, actions=d["actions"], want_target=True, out=d["out"])
        res = run(d)
        expect(_lib.E_NONFINITE)
        ref = tr.td_loss("dqn", c["q"], c["next_q"], c["rewards"], c["dones"], 0.97, actions=a)
        assert np.nonzero(ref["bad"])[0].tolist() == [20, 30, 40, 277]
        _same_bits(res.grad_q, ref["grad_q"]); _same_bits(res.target, ref["y"])
        assert int(torch.isnan(res.grad_q).all(dim=1).sum()) == 4 and int(torch.isnan(res.grad_q).any(dim=1).sum()) == 4
        assert bool(torch.isnan(res.stats[:5]).all()) and float(res.stats[5]) == 0.0 and float(res.target[30]) == np.inf
        c["actions"][5] = A; c["actions"][299] = -1           # two actions out of range beside them: one error each
        d = _dqn_device(c, True)
        res = run(d)
        expect(_lib.E_INDEX, then_clean=False)               # one error per sync: the index word first, then the other, then none
        expect(_lib.E_NONFINITE)
        ref = tr.td_loss("dqn", c["q"], c["next_q"], c["rewards"], c["dones"], 0.97, actions=c["actions"])
        assert np.nonzero(ref["oob"])[0].tolist() == [5, 299]
        assert bool((d["guard"][1:-1][[5, 299]] == SENTINEL).all()) and bool((res.target[[5, 299]] == SENTINEL).all())
        _same_bits(res.grad_q, ref["grad_q"], skip=ref["oob"]); _same_bits(res.target, ref["y"], skip=ref["oob"])
        small = {k: v[:100].copy() for k, v in tr.dqn_case(B, A, dt, adt=np.int32).items()}
        small["actions"][7] = 2 ** 31 - 1                     # an int32 action out of range alone, in the one-launch route
        d = _dqn_device(small, False)
        res = run(d)
        expect(_lib.E_INDEX)
        assert bool((res.grad_q[7] == SENTINEL).all()) and bool(torch.isnan(res.stats[:5]).all())
        ref = tr.td_loss("dqn", small["q"], small["next_q"], small["rewards"], small["dones"], 0.97, actions=small["actions"])
        _same_bits(res.grad_q, ref["grad_q"], skip=ref["oob"])
        # the critics
        c = tr.critics_case(B, 2, dt)
        c["next_q"][1][20] = np.nan; c["rewards"][277] = np.inf; c["next_log_prob"][30] = -np.inf; c["q"][1][40] = np.nan; c["dones"][50] = np.nan
        c["next_q"][0][60] = np.inf                           # legal beside a finite minimum
        d = _critics_device(c, True)
        sac = lambda d, **kw: eng.td_loss("sac", d["q"], d["next_q"], d["rewards"], d["dones"], 0.96, next_log_prob=d["next_log_prob"], want_target=True,
                                          out=d["out"], **kw)
        res = sac(d, ent_coef=ALPHA)
        expect(_lib.E_NONFINITE)
        ref = tr.td_loss("sac", c["q"], c["next_q"], c["rewards"], c["dones"], 0.96, next_log_prob=c["next_log_prob"], alpha=ALPHA)
        assert np.nonzero(ref["bad"])[0].tolist() == [20, 30, 40, 50, 277]
        for k in range(2):
            _same_bits(res.grad_q[k], ref["grad_q"][k])
        _same_bits(res.target, ref["y"])
        assert bool(torch.isnan(res.stats[:5]).all()) and float(res.stats[5]) == ALPHA
        c = tr.critics_case(B, 2, dt)                         # alpha = NaN: every row
        for kw in (dict(ent_coef=float("nan")), dict(ent_coef=torch.tensor([np.nan], dtype=torch.float64, device="cuda")),
                   dict(log_ent_coef=torch.tensor([np.nan], dtype=torch.float64, device="cuda"))):
            d = _critics_device(c, False)
            res = sac(d, **kw)
            expect(_lib.E_NONFINITE)
            assert all(bool(torch.isnan(g).all()) for g in res.grad_q) and bool(torch.isnan(res.target).all()) and bool(torch.isnan(res.stats[:6]).all())
    res = eng.td_loss("td3", [_t(x) for x in c["q"]], [_t(x) for x in c["next_q"]], _t(c["rewards"]), _t(c["dones"]), 0.96)      # a clean call syncs clean
    eng.sync()
    assert bool(torch.isfinite(res.stats).all())


def test_refused_arguments_enqueue_nothing():
    import torch
    from rl_ptg_amd import _lib
    eng = _engine()
    B, A = 300, 5
    L, h, stream = eng._L, eng._h, eng._stream()
    d = _dqn_device(tr.dqn_case(B, A, np.float32, adt=np.int32), True)
    dc = _critics_device(tr.critics_case(B, 2, np.float32), True)
    a64 = torch.tensor([ALPHA], dtype=torch.float64, device="cuda")
    ws = eng.td_loss_workspace(B)
    ws.fill_(0x5A)
    torch.cuda.synchronize()

    def fill(ds, kw):
        for k, v in kw.items():
            if isinstance(v, (list, tuple)):
                for j, x in enumerate(v):
                    getattr(ds, k)[j] = x
            else:
                setattr(ds, k, v)
        return ds

    def dqn(**kw):
        a = dict(kind=_lib.TD_DQN, n_actions=A, q_dtype=_lib.OUT_F32, act_kind=_lib.ACT_I32, rew_dtype=_lib.OUT_F32, done_dtype=_lib.OUT_F32, batch=B,
                 q_dev=[d["q"].data_ptr()], q_s_n=[A + 1], next_q_dev=[d["next_q"].data_ptr()], next_s_n=[A + 1], act_dev=d["actions"].data_ptr(),
                 rew_dev=d["rewards"].data_ptr(), done_dev=d["dones"].data_ptr(), gamma=0.97, stats_dev=d["out"][0].data_ptr(),
                 grad_q_dev=[d["out"][1].data_ptr()], g_s_n=[A + 1], y_dev=d["out"][2].data_ptr(), ws_dev=ws.data_ptr())
        a.update(kw)
        return fill(_lib.PtgTd(), a)

    def crit(**kw):
        a = dict(kind=_lib.TD_CRITICS, flags=_lib.TD_ENTROPY, n_critics=2, q_dtype=_lib.OUT_F32, rew_dtype=_lib.OUT_F32, done_dtype=_lib.OUT_F32, batch=B,
                 q_dev=[x.data_ptr() for x in dc["q"]], q_s_n=[2, 2], next_q_dev=[x.data_ptr() for x in dc["next_q"]], next_s_n=[2, 2],
                 rew_dev=dc["rewards"].data_ptr(), done_dev=dc["dones"].data_ptr(), next_logp_dev=dc["next_log_prob"].data_ptr(), gamma=0.96, alpha=ALPHA, scale=0.5,
                 stats_dev=dc["out"][0].data_ptr(), grad_q_dev=[x.data_ptr() for x in dc["out"][1]], g_s_n=[3, 3], ws_dev=ws.data_ptr())
        a.update(kw)
        return fill(_lib.PtgTd(), a)

    q0, q1 = dc["q"][0].data_ptr(), dc["q"][1].data_ptr()
    bad = [dqn(q_dev=[None]), dqn(next_q_dev=[None]), dqn(grad_q_dev=[None]), dqn(act_dev=None), dqn(rew_dev=None), dqn(done_dev=None), dqn(stats_dev=None),
           dqn(ws_dev=None), dqn(ws_dev=ws.data_ptr() + 4), dqn(kind=2), dqn(kind=-1), dqn(flags=4), dqn(flags=8), dqn(flags=_lib.TD_ENTROPY),
           dqn(flags=_lib.TD_ENTROPY, next_logp_dev=dc["next_log_prob"].data_ptr()), dqn(flags=_lib.TD_LOG_ALPHA, alpha_dev=a64.data_ptr()),
           dqn(q_dtype=2), dqn(q_dtype=-1), dqn(rew_dtype=2), dqn(done_dtype=3), dqn(act_kind=_lib.ACT_F32), dqn(act_kind=3),
           dqn(n_actions=1), dqn(n_actions=33, q_s_n=[33], next_s_n=[33], g_s_n=[33]), dqn(batch=0), dqn(batch=-3), dqn(batch=2 ** 31 + 1), dqn(batch=2 ** 40),
           dqn(q_s_n=[A - 1]), dqn(next_s_n=[A - 1]), dqn(g_s_n=[A - 1]), dqn(q_s_n=[0]), dqn(g_s_n=[-1]),
           crit(n_critics=0), crit(n_critics=5), crit(n_critics=-1), crit(q_dev=[q0, None]), crit(next_q_dev=[None, q1]), crit(grad_q_dev=[q0, None]),
           crit(q_s_n=[2, 0]), crit(next_s_n=[0, 2]), crit(g_s_n=[3, -1]), crit(next_logp_dev=None), crit(flags=_lib.TD_ENTROPY | _lib.TD_LOG_ALPHA),
           crit(flags=_lib.TD_LOG_ALPHA, alpha_dev=a64.data_ptr()), crit(flags=_lib.TD_ENTROPY | 4), crit(rew_dev=None), crit(ws_dev=None), crit(stats_dev=None),
           crit(q_dtype=7), crit(batch=0)]
    for k, ds in enumerate(bad):
        assert L.ptg_td_loss(h, C.byref(ds), stream) == _lib.E_INVALID, k
        assert b"ptg_td_loss" in L.ptg_last_error(h)
        assert torch.cuda.current_stream().query() is True, k
    assert L.ptg_td_loss(h, None, stream) == _lib.E_INVALID and L.ptg_td_loss(None, C.byref(dqn()), stream) == _lib.E_INVALID
    assert torch.cuda.current_stream().query() is True
    for out, guard in ((d["out"], d["guard"]), (dc["out"], dc["guard"])):
        assert bool((guard == SENTINEL).all()) and bool((out[0] == SENTINEL).all()) and bool((out[2] == SENTINEL).all())
    assert bool((ws == 0x5A).all())
    good = [dqn(), dqn(y_dev=None), dqn(batch=1), dqn(n_critics=77, scale=float("nan")), crit(), crit(flags=0, next_logp_dev=None), crit(alpha_dev=a64.data_ptr()),
            crit(flags=_lib.TD_ENTROPY | _lib.TD_LOG_ALPHA, alpha_dev=a64.data_ptr()), crit(n_critics=1, q_dev=[q0, None]), crit(n_actions=99, act_kind=9)]
    for k, ds in enumerate(good):
        assert L.ptg_td_loss(h, C.byref(ds), stream) == 0, (k, L.ptg_last_error(h))
    eng.sync()
    assert bool(torch.isfinite(d["out"][0]).all()) and bool(torch.isfinite(dc["out"][0]).all())
