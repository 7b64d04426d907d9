"""ppo_loss / a2c_loss: the fused policy loss (HipEngine.policy_loss, include/ptg_env.h: ptg_policy_loss) behind torch autograd;
ppo_loss_group / a2c_loss_group: the losses of up to eight independent agents in the launches of one (HipEngine.policy_loss_group,
ptg_policy_loss_group) under ONE autograd function;
ppo_sde_loss / a2c_sde_loss: the same for a policy with gSDE (HipEngine.sde_policy_loss, ptg_sde_policy_loss); sde_squashed_rsample: SAC's
and TQC's actor head with gSDE (HipEngine.sde_rsample / sde_rsample_backward, ptg_sde_rsample);
dqn_loss / td3_critic_loss / sac_critic_loss: the fused TD losses (HipEngine.td_loss, ptg_td_loss) likewise, and tqc_critic_loss: TQC's
quantile-Huber critic loss (HipEngine.quantile_loss, ptg_quantile_loss); squashed_rsample (HipEngine.rsample / rsample_backward,
ptg_rsample) and sac_actor_loss / tqc_actor_loss / td3_actor_loss / ent_coef_loss (HipEngine.actor_loss, ptg_actor_loss): the actor
half of an off-policy step; dqn_loss_group / td3_critic_loss_group / sac_critic_loss_group, squashed_rsample_group, sac_actor_loss_group /
tqc_actor_loss_group / td3_actor_loss_group and ent_coef_loss_group: those of up to eight independent agents in the launches of one
(HipEngine.td_loss_group, rsample_group / rsample_backward_group, actor_loss_group) -- see the end of the file.

    out = net(obs)                                            # [B, A + 1]: logits and a value column
    loss, stats = ppo_loss(engine, out[:, :A], out[:, A], actions, old_log_prob, advantages, returns, clip_range=0.2)
    loss.backward()                                           # drives the network exactly as SB3's loss.backward() does

Forward launches the kernel, which computes the loss, SB3's logged statistics and d loss / d logits (or means), d loss / d values
and d loss / d log_std in one pass; backward hands those to autograd, scaled by the incoming gradient.  Nothing else of the call is
differentiable: actions, old log-probs, advantages, returns and old values are data, as they are in SB3.  Without out= the gradient
tensors are allocated zeroed, so a row the kernel leaves untouched (an action out of range, reported at the next sync) adds nothing
to the network's gradients; with out= the caller's tensors are used as they are and must not be reused before backward has run.  There is no torch
fall-back: without the library or a GPU the engine does not exist."""
import torch


class _PolicyLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, kind, head_input, values, log_std, actions, old_log_prob, advantages, returns, old_values, kw):
        if kw.get("out") is None:                            # fresh gradients are zeroed here: a row refused for its action (PTG_E_INDEX at the next
            dev, dt = head_input.device, head_input.dtype    # sync) then contributes nothing to the network's gradients instead of uninitialised memory
            kw = dict(kw, out=(torch.empty(8, dtype=torch.float64, device=dev), torch.zeros(head_input.shape, dtype=dt, device=dev),
                               torch.zeros(values.shape[0], dtype=dt, device=dev), None if log_std is None else torch.zeros(1, dtype=dt, device=dev)))
        res = engine.policy_loss(kind, head_input.detach(), values.detach(), actions, old_log_prob, advantages, returns, old_values=old_values,
                                 log_std=None if log_std is None else log_std.detach(), **kw)
        ctx.res = res
        ctx.shapes = (head_input.shape, values.shape, None if log_std is None else log_std.shape)
        stats = res.stats
        ctx.mark_non_differentiable(stats)
        return res.stats[0].to(head_input.dtype, copy=True), stats

    @staticmethod
    def backward(ctx, grad_loss, _grad_stats):
        res, (s_in, s_val, s_ls) = ctx.res, ctx.shapes
        g_ls = None if s_ls is None else (res.grad_log_std * grad_loss).reshape(s_ls)
        return (None, None, (res.grad_input * grad_loss).reshape(s_in), (res.grad_values * grad_loss).reshape(s_val), g_ls,
                None, None, None, None, None, None)


def _call(kind, engine, head_input, values, actions, old_log_prob, advantages, returns, old_values, log_std, kw):
    return _PolicyLossFn.apply(engine, kind, head_input, values, log_std, actions, old_log_prob, advantages, returns, old_values, kw)


def ppo_loss(engine, head_input, values, actions, old_log_prob, advantages, returns, *, clip_range, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5,
             normalize_advantage=True, old_values=None, log_std=None, out=None, workspace=None):
    """SB3's PPO.train loss of one minibatch -> (loss, stats): loss a 0-dim tensor in head_input's dtype that carries the graph,
    stats float64 [8] = loss, policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction, adv mean, adv std (read stats[4]
    for target_kl).  head_input: logits [B, A] with integer actions, or the Gaussian head's means with log_std (a 1-element
    parameter) and the stored raw samples as actions.  Arguments as HipEngine.policy_loss."""
    kw = dict(clip_range=clip_range, clip_range_vf=clip_range_vf, ent_coef=ent_coef, vf_coef=vf_coef, normalize_advantage=normalize_advantage,
              out=out, workspace=workspace)
    return _call("ppo", engine, head_input, values, actions, old_log_prob, advantages, returns, old_values, log_std, kw)


def a2c_loss(engine, head_input, values, actions, advantages, returns, *, ent_coef=0.0, vf_coef=0.5, normalize_advantage=False, log_std=None,
             out=None, workspace=None):
    """SB3's A2C.train loss of its one batch -> (loss, stats) as ppo_loss gives them (approx_kl and clip_fraction are 0)."""
    kw = dict(ent_coef=ent_coef, vf_coef=vf_coef, normalize_advantage=normalize_advantage, out=out, workspace=workspace)
    return _call("a2c", engine, head_input, values, actions, None, advantages, returns, None, log_std, kw)


# ------------------------------------------------------------------------------------------------- G agents' losses in one's launches
#     outs = nets(obs_batches)                                  # TrainMLPGroup: policy and value net of every agent
#     losses, stats = ppo_loss_group(engine, [dict(head_input=outs[2 * i], values=outs[2 * i + 1], actions=..., old_log_prob=...,
#                                                  advantages=..., returns=...) for i in range(G)], clip_range=[0.2, 0.1, ...])
#     torch.autograd.backward(losses)                           # ONE pass: every agent's gradients go to its own networks
class _PolicyLossGroupFn(torch.autograd.Function):
    """forward: one policy_loss_group over the members; backward: each member's gradients, scaled by its loss's incoming gradient, to
    its head_input, values and log_std; a loss that received no gradient hands None to its networks"""

    @staticmethod
    def forward(ctx, engine, kind, members, *diff):          # diff: head_input, values, log_std (or None) of every member
        calls, shapes = [], []
        for i, m in enumerate(members):
            hi, val, ls = diff[3 * i:3 * i + 3]
            kw = dict(m, head_input=hi.detach(), values=val.detach(), log_std=None if ls is None else ls.detach())
            if kw.get("out") is None:                        # fresh gradients are zeroed, as _PolicyLossFn's are
                dev, dt = hi.device, hi.dtype
                kw["out"] = (torch.empty(8, dtype=torch.float64, device=dev), torch.zeros(hi.shape, dtype=dt, device=dev),
                             torch.zeros(val.shape[0], dtype=dt, device=dev), None if ls is None else torch.zeros(1, dtype=dt, device=dev))
            calls.append(kw)
            shapes.append((hi.shape, val.shape, None if ls is None else ls.shape))
        res = engine.policy_loss_group(kind, calls)
        ctx.res, ctx.shapes = res, shapes
        stats = [r.stats for r in res]
        ctx.mark_non_differentiable(*stats)
        ctx.set_materialize_grads(False)                     # an unused loss's gradient arrives as None, not as a zero
        return (*[r.stats[0].to(d.dtype, copy=True) for r, d in zip(res, diff[::3])], *stats)

    @staticmethod
    def backward(ctx, *grads):
        out = []
        for r, (s_in, s_val, s_ls), g in zip(ctx.res, ctx.shapes, grads):
            if g is None:
                out += [None, None, None]
                continue
            out += [(r.grad_input * g).reshape(s_in), (r.grad_values * g).reshape(s_val), None if s_ls is None else (r.grad_log_std * g).reshape(s_ls)]
        return (None, None, None, *out)


_GROUP_TENSORS = ("head_input", "values", "actions", "old_log_prob", "advantages", "returns", "old_values", "log_std", "out", "workspace")


def _group_call(who, kind, engine, members, scalars):
    if not isinstance(members, (list, tuple)) or not members or not all(isinstance(m, dict) for m in members):
        raise TypeError(f"{who}: members must be a non-empty list of dicts (head_input, values, actions, advantages, returns, ...), got {type(members).__name__}")
    G = len(members)
    calls = []
    for i, m in enumerate(members):
        unknown = [k for k in m if k not in _GROUP_TENSORS]
        if unknown:
            raise TypeError(f"{who}: member {i} names {unknown}; a member holds the tensors {_GROUP_TENSORS}, the scalars are keyword arguments")
        missing = [k for k in ("head_input", "values") if not torch.is_tensor(m.get(k))]
        if missing:
            raise TypeError(f"{who}: member {i} needs the tensors {missing}")
        kw = dict(m)
        for name, v in scalars.items():                      # one value for all, or a list with one per member
            if isinstance(v, (list, tuple)):
                if len(v) != G:
                    raise ValueError(f"{who}: {name} must have one entry per member, {G}, or be one value for all; got {len(v)}")
                v = v[i]
            kw[name] = v
        if kind == "a2c":
            kw["old_log_prob"] = None
        calls.append(kw)
    diff = [t for m in calls for t in (m.get("head_input"), m.get("values"), m.get("log_std"))]
    out = _PolicyLossGroupFn.apply(engine, kind, calls, *diff)
    return list(out[:G]), list(out[G:])


def ppo_loss_group(engine, members, *, clip_range, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True):
    """ppo_loss for G independent agents' minibatches of one batch size, 1 <= G <= 8, in the launches of ONE ppo_loss
    (HipEngine.policy_loss_group) -> (losses, stats): two lists of G, member i's what ppo_loss gives for its
    arguments, bit for bit.  members: a list of dicts of ppo_loss's tensors by name (head_input, values, actions, old_log_prob,
    advantages, returns; old_values, log_std, out, workspace).  clip_range, clip_range_vf, ent_coef, vf_coef: one value for all, or a
    list with one per member (clip_range_vf: given for all or for none); normalize_advantage: one value.  The G losses belong in ONE
    backward pass -- torch.autograd.backward(losses) -- which hands each member's gradients to its own networks; a loss left out of it
    leaves its networks' gradients alone.
    Cost (profiles/train_group_cost.txt; DESIGN.md section 26, whose one condition held at every shape): see DeviceOptimizerGroup's docstring."""
    scalars = dict(clip_range=clip_range, clip_range_vf=clip_range_vf, ent_coef=ent_coef, vf_coef=vf_coef, normalize_advantage=normalize_advantage)
    return _group_call("ppo_loss_group", "ppo", engine, members, scalars)


def a2c_loss_group(engine, members, *, ent_coef=0.0, vf_coef=0.5, normalize_advantage=False):
    """a2c_loss for G independent agents -> (losses, stats) as ppo_loss_group gives them (no old_log_prob, no clipping)."""
    return _group_call("a2c_loss_group", "a2c", engine, members, dict(ent_coef=ent_coef, vf_coef=vf_coef, normalize_advantage=normalize_advantage))


# ------------------------------------------------------------------------------------------------- the on-policy losses with gSDE
#     out = net(obs)                                            # TrainMLP: [B, 2], the mean and a value column
#     latent = net.hidden[-1]                                   # [B, L]: data, as under SB3's learn_features=False
#     loss, stats = ppo_sde_loss(engine, out[:, 0], out[:, 1], latent, log_std, actions, old_log_prob, advantages, returns, clip_range=0.2)
#     loss.backward()                                           # fills the network's gradients and log_std.grad
# The gradient reaches the latent only when it requires grad (learn_features=True); then the kernel writes d loss / d latent too.
class _SdePolicyLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, kind, mean, values, latent, log_std, actions, old_log_prob, advantages, returns, old_values, kw):
        res = engine.sde_policy_loss(kind, mean.detach(), values.detach(), latent.detach(), log_std.detach(), actions, old_log_prob, advantages, returns,
                                     old_values=old_values, want_grad_latent=latent.requires_grad, **kw)
        ctx.res = res
        ctx.shapes = (mean.shape, values.shape, latent.shape, log_std.shape)
        ctx.mark_non_differentiable(res.stats)
        return res.stats[0].to(mean.dtype, copy=True), res.stats

    @staticmethod
    def backward(ctx, grad_loss, _grad_stats):
        res, (s_mu, s_val, s_lat, s_ls) = ctx.res, ctx.shapes
        g_lat = None if res.grad_latent is None else (res.grad_latent * grad_loss).reshape(s_lat)
        return (None, None, (res.grad_input * grad_loss).reshape(s_mu), (res.grad_values * grad_loss).reshape(s_val), g_lat,
                (res.grad_log_std * grad_loss).reshape(s_ls), None, None, None, None, None, None)


def ppo_sde_loss(engine, mean, values, latent, log_std, actions, old_log_prob, advantages, returns, *, clip_range, clip_range_vf=None, ent_coef=0.0,
                 vf_coef=0.5, normalize_advantage=True, old_values=None, out=None, workspace=None):
    """ppo_loss for a policy with gSDE (SB3's use_sde=True): SB3's PPO.train loss of one minibatch on StateDependentNoiseDistribution
    -> (loss, stats) as ppo_loss gives them.  mean [B] / [B, 1], values [B], latent [B, L] the policy's last hidden layer, log_std the
    [L] / [L, 1] parameter, actions the stored raw samples.  Gradients go to mean, values and log_std, and to latent when it requires
    grad.  Arguments as HipEngine.sde_policy_loss."""
    kw = dict(clip_range=clip_range, clip_range_vf=clip_range_vf, ent_coef=ent_coef, vf_coef=vf_coef, normalize_advantage=normalize_advantage,
              out=out, workspace=workspace)
    return _SdePolicyLossFn.apply(engine, "ppo", mean, values, latent, log_std, actions, old_log_prob, advantages, returns, old_values, kw)


def a2c_sde_loss(engine, mean, values, latent, log_std, actions, advantages, returns, *, ent_coef=0.0, vf_coef=0.5, normalize_advantage=False, out=None,
                 workspace=None):
    """a2c_loss for a policy with gSDE -> (loss, stats) as ppo_sde_loss gives them (approx_kl and clip_fraction are 0)."""
    kw = dict(ent_coef=ent_coef, vf_coef=vf_coef, normalize_advantage=normalize_advantage, out=out, workspace=workspace)
    return _SdePolicyLossFn.apply(engine, "a2c", mean, values, latent, log_std, actions, None, advantages, returns, None, kw)


# ------------------------------------------------------------------------------------------------- SAC / TQC with gSDE
#     noise.reset_train_noise(log_std)                          # SquashedSdeNoise: once per gradient step, as SB3's actor.reset_noise()
#     with torch.no_grad():
#         next_actions, next_log_prob = sde_squashed_rsample(noise, mu(trunk(next_obs)), trunk_out, log_std)       # the same row
#     latent = trunk(obs)                                       # TrainMLP, its hidden activation as out_activation
#     actions, log_prob = sde_squashed_rsample(noise, mu(latent), latent, log_std)
#     loss, stats = sac_actor_loss(engine, critics(obs, actions), log_prob, ent_coef=alpha); loss.backward()
# The backward is a kernel (HipEngine.sde_rsample_backward): it fills the gradients of the mean, of the latent (learn_features=True)
# and of log_std, the last through the variance AND through the resampled row E = exp(log_std) * z, which SB3 draws with rsample().
class _SdeRSampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, noise, mean, latent, log_std, deterministic):
        eng = noise.engine
        keep = any(ctx.needs_input_grad[1:4])                # False under torch.no_grad(): nothing is kept
        row = None if deterministic else noise.train_row
        res = eng.sde_rsample(mean.detach(), latent.detach(), log_std.detach(), row, clip_mean=noise.clip_mean, deterministic=deterministic, want_saved=keep)
        if keep:
            ctx.save_for_backward(mean.detach(), latent.detach(), log_std.detach())
            ctx.eng, ctx.row, ctx.saved, ctx.clip_mean, ctx.deterministic = eng, None if row is None else row.clone(), res.saved, noise.clip_mean, deterministic
            ctx.want = (ctx.needs_input_grad[2], ctx.needs_input_grad[3] and not deterministic)
        return res.actions.reshape(mean.shape), res.log_prob.reshape(mean.shape)

    @staticmethod
    def backward(ctx, grad_actions, grad_log_prob):
        mean, latent, log_std = ctx.saved_tensors
        ga = None if grad_actions is None else grad_actions.contiguous()
        gl = None if grad_log_prob is None else grad_log_prob.contiguous()
        g = ctx.eng.sde_rsample_backward(mean, latent, log_std, ctx.row, ctx.saved, ga, gl, clip_mean=ctx.clip_mean, deterministic=ctx.deterministic,
                                         want_grad_latent=ctx.want[0], want_grad_log_std=ctx.want[1])
        g_ls = None if g.grad_log_std is None else g.grad_log_std.reshape(log_std.shape)
        return None, g.grad_mean.reshape(mean.shape), g.grad_latent, g_ls, None


def sde_squashed_rsample(noise, mean, latent, log_std, deterministic=False):
    """SB3's Actor.action_log_prob of SAC / TQC with use_sde on a replay batch -> (actions, log_prob), shaped like mean, with a
    grad_fn: noise a SquashedSdeNoise whose reset_train_noise() drew this gradient step's row, mean [B] / [B, 1] the mu layer's
    UNCLIPPED output, latent [B, L] the trunk's output, log_std the [L] / [L, 1] parameter.  The forward is HipEngine.sde_rsample, the
    backward HipEngine.sde_rsample_backward on the saved (noise, V) pairs and a copy of the row.  Under torch.no_grad() (the next
    observations, for the critic target) nothing is kept."""
    return _SdeRSampleFn.apply(noise, mean, latent, log_std, deterministic)


# ------------------------------------------------------------------------------------------------- the off-policy losses
#     batch = buffer.sample(256)                                # DeviceReplayBuffer: observations, next observations, columns
#     with torch.no_grad():
#         next_q = [c(next_in) for c in critic_targets]         # K target critics on (s', a')
#     loss, stats = sac_critic_loss(engine, [c(cur_in) for c in critics], next_q, rewards, dones, next_log_prob, gamma=0.96,
#                                   log_ent_coef=log_alpha)
#     loss.backward()
# Only the current Q tensors are differentiable: the target Q-values, rewards, dones, log-probs and alpha are data, as they are under
# SB3's torch.no_grad().  Without out= the gradient tensors are allocated zeroed, so a DQN row refused for its action adds nothing.
class _TdLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, kind, next_q, rewards, dones, gamma, kw, *q):
        dqn = kind == "dqn"
        if kw.get("out") is None:
            dev, dt = q[0].device, q[0].dtype
            grads = [torch.zeros(t.shape, dtype=dt, device=dev) for t in q]
            kw = dict(kw, out=(torch.empty(8, dtype=torch.float64, device=dev), grads[0] if dqn else grads, None))
        qd = [t.detach() for t in q]
        res = engine.td_loss(kind, qd[0] if dqn else qd, next_q, rewards, dones, gamma, **kw)
        ctx.grads = [res.grad_q] if dqn else list(res.grad_q)
        ctx.shapes = [t.shape for t in q]
        ctx.mark_non_differentiable(res.stats)
        return res.stats[0].to(q[0].dtype, copy=True), res.stats

    @staticmethod
    def backward(ctx, grad_loss, _grad_stats):
        return (None,) * 7 + tuple((g * grad_loss).reshape(s) for g, s in zip(ctx.grads, ctx.shapes))


def dqn_loss(engine, q, next_q, actions, rewards, dones, *, gamma, out=None, workspace=None):
    """SB3's DQN.train loss of one replay batch -> (loss, stats): smooth_l1_loss(q.gather(1, actions), rewards + (1 - dones) * gamma *
    next_q.max(1)).  q = q_net(obs) [B, A] carries the graph, next_q = q_net_target(next_obs) [B, A] is data.  stats float64 [8] =
    loss, mean chosen Q, mean target, mean |delta|, share of |delta| >= 1, 0, 0, 0.  Arguments as HipEngine.td_loss."""
    return _TdLossFn.apply(engine, "dqn", next_q.detach(), rewards, dones, gamma, dict(actions=actions, out=out, workspace=workspace), q)


def td3_critic_loss(engine, q, next_q, rewards, dones, *, gamma, out=None, workspace=None):
    """SB3's TD3.train critic loss -> (loss, stats): sum_k mse_loss(q[k], rewards + (1 - dones) * gamma * min_k next_q[k]).  q: the list
    of the K critics' outputs [B] / [B, 1] on (obs, actions), carrying the graph; next_q: the K target critics' outputs on (next_obs,
    the smoothed target action), data."""
    return _TdLossFn.apply(engine, "td3", [t.detach() for t in next_q], rewards, dones, gamma, dict(out=out, workspace=workspace), *q)


def sac_critic_loss(engine, q, next_q, rewards, dones, next_log_prob, *, gamma, ent_coef=None, log_ent_coef=None, out=None, workspace=None):
    """SB3's SAC.train critic loss -> (loss, stats): 0.5 * sum_k mse_loss(q[k], rewards + (1 - dones) * gamma * (min_k next_q[k] -
    alpha * next_log_prob)).  alpha: ent_coef (a float, or a float64 device tensor of 1 element) or exp(log_ent_coef) (SAC's learned
    parameter, a float64 device tensor of 1 element read when the kernel runs); stats[5] holds the alpha that was used."""
    kw = dict(next_log_prob=next_log_prob.detach(), ent_coef=ent_coef.detach() if torch.is_tensor(ent_coef) else ent_coef,
              log_ent_coef=log_ent_coef.detach() if torch.is_tensor(log_ent_coef) else log_ent_coef, out=out, workspace=workspace)
    return _TdLossFn.apply(engine, "sac", [t.detach() for t in next_q], rewards, dones, gamma, kw, *q)


# ------------------------------------------------------------------------------------------------- TQC's quantile critics
#     with torch.no_grad():
#         next_quantiles = critic_target(next_obs, next_actions)          # [B, K, Q]
#     loss, stats = tqc_critic_loss(engine, critic(obs, actions), next_quantiles, rewards, dones, next_log_prob, gamma=0.9639,
#                                   top_quantiles_to_drop_per_net=2, log_ent_coef=log_alpha)
#     loss.backward()
# Only the current quantiles are differentiable; the sort, the dropped tops, the entropy term and the targets are data, as they are
# under sb3_contrib's torch.no_grad().
class _QuantileLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, as_list, next_quantiles, rewards, dones, next_log_prob, gamma, drop, kw, *q):
        res = engine.quantile_loss([t.detach() for t in q] if as_list else q[0].detach(), next_quantiles, rewards, dones, next_log_prob, gamma, drop, **kw)
        ctx.grads = list(res.grad_quantiles) if as_list else [res.grad_quantiles]
        ctx.mark_non_differentiable(res.stats)
        return res.stats[0].to(q[0].dtype, copy=True), res.stats

    @staticmethod
    def backward(ctx, grad_loss, _grad_stats):
        return (None,) * 9 + tuple(g * grad_loss for g in ctx.grads)


def tqc_critic_loss(engine, quantiles, next_quantiles, rewards, dones, next_log_prob, *, gamma, top_quantiles_to_drop_per_net, ent_coef=None,
                    log_ent_coef=None, out=None, workspace=None):
    """sb3_contrib's TQC.train critic loss -> (loss, stats): quantile_huber_loss(quantiles, rewards + (1 - dones) * gamma * (the lowest
    K * (Q - d) of the sorted next_quantiles - alpha * next_log_prob), sum_over_quantiles=False).  quantiles: the critics' output on
    (obs, actions), a [B, K, Q] tensor or a list of K [B, Q] tensors, carrying the graph; next_quantiles: the target critics' on
    (next_obs, next_actions), data.  alpha: ent_coef (a float, or a float64 device tensor of 1 element) or exp(log_ent_coef) (a float64
    device tensor of 1 element read when the kernel runs); stats float64 [8] = loss, mean current quantile, mean target, mean |delta|,
    share of the pairs with |delta| > 1, alpha as used, 0, 0.  Arguments as HipEngine.quantile_loss."""
    as_list = isinstance(quantiles, (list, tuple))
    det = lambda t: t.detach() if torch.is_tensor(t) else t
    kw = dict(ent_coef=det(ent_coef), log_ent_coef=det(log_ent_coef), out=out, workspace=workspace)
    nxt = [det(t) for t in next_quantiles] if isinstance(next_quantiles, (list, tuple)) else det(next_quantiles)
    return _QuantileLossFn.apply(engine, as_list, nxt, rewards, dones, det(next_log_prob), gamma, top_quantiles_to_drop_per_net, kw,
                                 *(quantiles if as_list else (quantiles,)))


# ------------------------------------------------------------------------------------------------- the actor half of an off-policy step
#     mean, log_std = actor(obs)                                            # [B, 1] each; log_std unclamped
#     actions, log_prob = squashed_rsample(engine, mean, log_std, counter, seed=seed)
#     a_loss, _ = ent_coef_loss(engine, log_prob, log_alpha, target_entropy=-1.0)     # SB3's order: before the critic update
#     ...
#     loss, stats = sac_actor_loss(engine, [c(obs, actions) for c in critics], log_prob, ent_coef=a_stats[4:5])
#     loss.backward()                                                       # through the critics into actions and log_prob, then
#                                                                           # through rsample_backward into the actor
# squashed_rsample is the first op here whose backward is a kernel too: the reparametrised path through tanh(mean + sigma * z) IS
# SAC's actor gradient.  The draw itself is data; the backward reads the noise the forward stored, not the counter.
class _RSampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, mean, log_std, counter, seed, deterministic, out):
        res = engine.rsample(mean.detach(), log_std.detach(), counter, seed=seed, deterministic=deterministic, out=out)
        if res.noise is None:
            raise ValueError("squashed_rsample: out.noise is None, but the backward reads it")
        ctx.engine, ctx.noise = engine, res.noise
        ctx.save_for_backward(mean, log_std)
        return res.actions, res.log_prob

    @staticmethod
    def backward(ctx, grad_actions, grad_log_prob):
        mean, log_std = ctx.saved_tensors
        ga = None if grad_actions is None else grad_actions.contiguous()
        gl = None if grad_log_prob is None else grad_log_prob.contiguous()
        g = ctx.engine.rsample_backward(mean.detach(), log_std.detach(), ctx.noise, ga, gl)
        return None, g.grad_mean, g.grad_log_std, None, None, None, None


def squashed_rsample(engine, mean, log_std, counter, *, seed=0, deterministic=False, out=None):
    """SB3's Actor.action_log_prob (SAC / TQC) -> (actions, log_prob), shaped like mean and differentiable in mean and log_std: the
    forward is HipEngine.rsample, the backward HipEngine.rsample_backward on the stored noise.  Under torch.no_grad() (the next
    observations, for the critic target) nothing is kept.  Arguments as HipEngine.rsample."""
    return _RSampleFn.apply(engine, mean, log_std, counter, seed, deterministic, out)


class _ActorLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, kind, as_list, n_q, kw, *diff):
        # diff: the tensors a gradient may go back to, per kind as below; everything else of the call travels in kw
        d = [t.detach() for t in diff]
        if kind == "ent_coef":                               # diff = (log_prob, log_ent_coef): the gradient goes to the latter alone
            res = engine.actor_loss(kind, log_prob=d[0], log_ent_coef=d[1], **kw)
            ctx.grads = [None, res.grad_log_ent_coef]
        elif kind == "td3":                                  # diff = (q1,)
            res = engine.actor_loss(kind, q=d[0], **kw)
            ctx.grads = [res.grad_q]
        else:                                                # diff = the critics' outputs (one tensor when stacked), then log_prob
            res = engine.actor_loss(kind, q=d[:n_q] if as_list else d[0], log_prob=d[n_q], **kw)
            ctx.grads = (list(res.grad_q) if as_list else [res.grad_q]) + [res.grad_log_prob]
        ctx.shapes = [t.shape for t in diff]
        ctx.mark_non_differentiable(res.stats)
        if kind == "ent_coef":
            return res.stats[1].clone(), res.stats
        return res.stats[0].to(diff[0].dtype, copy=True), res.stats

    @staticmethod
    def backward(ctx, grad_loss, _grad_stats):
        return (None,) * 5 + tuple(None if g is None else (g * grad_loss).reshape(s) for g, s in zip(ctx.grads, ctx.shapes))


def _det(t):
    return t.detach() if torch.is_tensor(t) else t


def sac_actor_loss(engine, q, log_prob, *, ent_coef=None, log_ent_coef=None, out=None, workspace=None):
    """SB3's SAC.train actor loss -> (loss, stats): (alpha * log_prob - min_k q[k]).mean().  q: the list of the K critics' outputs [B] /
    [B, 1] on (obs, actions_pi); q and log_prob carry the graph, alpha is data: ent_coef (a float, or a float64 device tensor of 1
    element) or exp(log_ent_coef), as SB3 detaches it.  stats as HipEngine.actor_loss gives them."""
    kw = dict(ent_coef=_det(ent_coef), log_ent_coef=_det(log_ent_coef), out=out, workspace=workspace)
    return _ActorLossFn.apply(engine, "sac", True, len(q), kw, *q, log_prob)


def tqc_actor_loss(engine, quantiles, log_prob, *, ent_coef=None, log_ent_coef=None, out=None, workspace=None):
    """sb3_contrib's TQC.train actor loss -> (loss, stats): (alpha * log_prob - quantiles.mean(2).mean(1)).mean().  quantiles: the
    critics' output on (obs, actions_pi), a [B, K, Q] tensor or a list of K [B, Q] tensors, carrying the graph."""
    as_list = isinstance(quantiles, (list, tuple))
    kw = dict(ent_coef=_det(ent_coef), log_ent_coef=_det(log_ent_coef), out=out, workspace=workspace)
    qs = tuple(quantiles) if as_list else (quantiles,)
    return _ActorLossFn.apply(engine, "tqc", as_list, len(qs), kw, *qs, log_prob)


def td3_actor_loss(engine, q1, *, out=None, workspace=None):
    """SB3's TD3.train actor loss -> (loss, stats): -critic.q1_forward(obs, actor(obs)).mean().  q1 [B] / [B, 1] carries the graph."""
    return _ActorLossFn.apply(engine, "td3", False, 1, dict(out=out, workspace=workspace), q1)


def ent_coef_loss(engine, log_prob, log_ent_coef, *, target_entropy, out=None, workspace=None):
    """SB3's entropy-coefficient loss -> (loss, stats): -(log_ent_coef * (log_prob + target_entropy).detach()).mean(), a 0-dim float64
    tensor differentiable in log_ent_coef (a float64 device tensor of 1 element) alone.  stats[4:5] is the alpha = exp(log_ent_coef)
    of this call on the device: hand it as ent_coef= to the critic loss and to the later actor loss, as SB3 uses the alpha from before
    the alpha optimiser's step for both."""
    kw = dict(target_entropy=target_entropy, out=out, workspace=workspace)
    return _ActorLossFn.apply(engine, "ent_coef", False, 0, kw, log_prob.detach(), log_ent_coef)


# ------------------------------------------------------------------------------------------------- G agents' off-policy steps in one's launches
#     qs = critics(cur_in)                                      # TrainMLPGroup: the K critics of every agent, agent by agent
#     losses, stats = sac_critic_loss_group(engine, [dict(q=qs[K * i:K * i + K], next_q=..., rewards=..., dones=..., next_log_prob=...,
#                                                         ent_coef=alpha_i) for i in range(G)], gamma=[0.96, 0.97, ...])
#     torch.autograd.backward(losses)                           # ONE pass: every agent's gradients go to its own critics
# Each *_group function is ONE autograd function over the members (HipEngine.td_loss_group / rsample_group / rsample_backward_group /
# actor_loss_group): member i's loss, statistics and gradients are, bit for bit, what the single function gives
# for its arguments.  A member dict holds the single function's tensors by name (and out, workspace); its scalars are keyword
# arguments, one value for all or a list with one per member.  A loss left out of the backward pass leaves its networks alone.
def _group_members(who, members, takes, needs, scalars):
    """the members as a list of call dicts: every name known, the needed tensors there, the scalars spread (a list: one per member)"""
    if not isinstance(members, (list, tuple)) or not members or not all(isinstance(m, dict) for m in members):
        raise TypeError(f"{who}: members must be a non-empty list of dicts {needs}, got {type(members).__name__}")
    G = len(members)
    calls = []
    for i, m in enumerate(members):
        unknown = [k for k in m if k not in takes]
        if unknown:
            raise TypeError(f"{who}: member {i} names {unknown}; a member holds {takes}, the scalars are keyword arguments")
        missing = [k for k in needs if m.get(k) is None]
        if missing:
            raise TypeError(f"{who}: member {i} needs {missing}")
        kw = dict(m)
        for name, v in scalars.items():
            if isinstance(v, list):
                if len(v) != G:
                    raise ValueError(f"{who}: {name} must have one entry per member, {G}, or be one value for all; got {len(v)}")
                v = v[i]
            if v is not None and kw.get(name) is None:
                kw[name] = v
        calls.append(kw)
    return calls


def _det_all(x):
    return [_det(t) for t in x] if isinstance(x, (list, tuple)) else _det(x)


class _TdLossGroupFn(torch.autograd.Function):
    """forward: one td_loss_group over the members; backward: each member's gradients, scaled by its loss's incoming gradient, to its
    current Q tensors; a loss that received no gradient hands None to its networks"""

    @staticmethod
    def forward(ctx, engine, kind, members, n_q, *q):        # q: the current Q tensors of every member, n_q[i] of member i
        dqn = kind == "dqn"
        calls, at = [], 0
        for m, n in zip(members, n_q):
            mine, at = q[at:at + n], at + n
            kw = dict(m)
            if kw.get("out") is None:                        # fresh gradients are zeroed, as _TdLossFn's are
                dev, dt = mine[0].device, mine[0].dtype
                grads = [torch.zeros(t.shape, dtype=dt, device=dev) for t in mine]
                kw["out"] = (torch.empty(8, dtype=torch.float64, device=dev), grads[0] if dqn else grads, None)
            qd = [t.detach() for t in mine]
            calls.append(dict(kw, q=qd[0] if dqn else qd))
        res = engine.td_loss_group(kind, calls)
        ctx.grads = [[r.grad_q] if dqn else list(r.grad_q) for r in res]
        ctx.shapes = [t.shape for t in q]
        stats = [r.stats for r in res]
        ctx.mark_non_differentiable(*stats)
        ctx.set_materialize_grads(False)                     # an unused loss's gradient arrives as None, not as a zero
        return (*[r.stats[0].to(gs[0].dtype, copy=True) for r, gs in zip(res, ctx.grads)], *stats)

    @staticmethod
    def backward(ctx, *grads):
        out, shapes = [], iter(ctx.shapes)
        for gs, g in zip(ctx.grads, grads):
            out += [None if g is None else (x * g).reshape(s) for x, s in zip(gs, shapes)]
        return (None, None, None, None, *out)


def _td_group(who, kind, engine, members, needs, scalars):
    calls = _group_members(who, members, needs + ("out", "workspace", "ent_coef", "log_ent_coef")[:4 if kind == "sac" else 2], needs, scalars)
    q = [[m.pop("q")] if kind == "dqn" else list(m.pop("q")) for m in calls]
    calls = [{k: _det_all(v) if k != "out" else v for k, v in m.items()} for m in calls]
    out = _TdLossGroupFn.apply(engine, kind, calls, [len(x) for x in q], *[t for x in q for t in x])
    return list(out[:len(calls)]), list(out[len(calls):])


def dqn_loss_group(engine, members, *, gamma):
    """dqn_loss for G independent agents' replay batches of one batch size, 1 <= G <= 8, in the launches of ONE dqn_loss -> (losses,
    stats): two lists of G.  members: dicts of q, next_q, actions, rewards, dones (out, workspace); gamma: one value or a list."""
    return _td_group("dqn_loss_group", "dqn", engine, members, ("q", "next_q", "actions", "rewards", "dones"), dict(gamma=gamma))


def td3_critic_loss_group(engine, members, *, gamma):
    """td3_critic_loss for G independent agents -> (losses, stats).  members: dicts of q, next_q (lists of K critic outputs), rewards,
    dones (out, workspace); gamma: one value or a list."""
    return _td_group("td3_critic_loss_group", "td3", engine, members, ("q", "next_q", "rewards", "dones"), dict(gamma=gamma))


def sac_critic_loss_group(engine, members, *, gamma, ent_coef=None):
    """sac_critic_loss for G independent agents -> (losses, stats).  members: dicts of q, next_q (lists of K critic outputs), rewards,
    dones, next_log_prob and one of ent_coef (a float or a float64 device tensor of 1 element) and log_ent_coef (out, workspace); all
    members bring log_ent_coef or none does.  gamma, ent_coef: one value or a list with one per member."""
    return _td_group("sac_critic_loss_group", "sac", engine, members, ("q", "next_q", "rewards", "dones", "next_log_prob"), dict(gamma=gamma, ent_coef=ent_coef))


class _RSampleGroupFn(torch.autograd.Function):
    """forward: one rsample_group; backward: one rsample_backward_group over the members whose outputs received a gradient"""

    @staticmethod
    def forward(ctx, engine, members, deterministic, *diff):     # diff: mean, log_std of every member
        calls = [dict(m, mean=diff[2 * i].detach(), log_std=diff[2 * i + 1].detach()) for i, m in enumerate(members)]
        res = engine.rsample_group(calls, deterministic=deterministic)
        if any(r.noise is None for r in res):
            raise ValueError("squashed_rsample_group: out.noise is None, but the backward reads it")
        ctx.engine, ctx.noise = engine, [r.noise for r in res]
        ctx.save_for_backward(*diff)
        ctx.set_materialize_grads(False)
        return tuple(t for r in res for t in (r.actions, r.log_prob))

    @staticmethod
    def backward(ctx, *grads):
        diff = ctx.saved_tensors
        live, calls = [], []
        for i, noise in enumerate(ctx.noise):
            ga, gl = grads[2 * i], grads[2 * i + 1]
            if ga is None and gl is None:
                continue
            live.append(i)
            calls.append(dict(mean=diff[2 * i].detach(), log_std=diff[2 * i + 1].detach(), noise=noise, grad_actions=None if ga is None else ga.contiguous(),
                              grad_log_prob=None if gl is None else gl.contiguous()))
        out = [None] * len(diff)
        if calls:
            for i, g in zip(live, ctx.engine.rsample_backward_group(calls)):
                out[2 * i], out[2 * i + 1] = g.grad_mean, g.grad_log_std
        return (None, None, None, *out)


def squashed_rsample_group(engine, members, *, seed=0, deterministic=False):
    """squashed_rsample for G independent actors' outputs of one batch size, 1 <= G <= 8, in the launches of ONE squashed_rsample -> a
    list of G (actions, log_prob) pairs, each differentiable in its member's mean and log_std.  members: dicts of mean, log_std, counter
    (out); every member its own counter.  seed: one value or a list with one per member.  The backward is one
    HipEngine.rsample_backward_group call over the members whose outputs received a gradient."""
    calls = _group_members("squashed_rsample_group", members, ("mean", "log_std", "counter", "out"), ("mean", "log_std"), dict(seed=seed))
    diff = [t for m in calls for t in (m.pop("mean"), m.pop("log_std"))]
    out = _RSampleGroupFn.apply(engine, calls, deterministic, *diff)
    return [(out[2 * i], out[2 * i + 1]) for i in range(len(calls))]


class _ActorLossGroupFn(torch.autograd.Function):
    """forward: one actor_loss_group over the members; backward: each member's gradients, scaled by its loss's incoming gradient"""

    @staticmethod
    def forward(ctx, engine, kind, members, layout, *diff):  # layout[i] = (as_list, n_q, tensors of member i in diff); diff as _ActorLossFn's, member by member
        calls, at = [], 0
        for m, (as_list, n_q, n) in zip(members, layout):
            d, at = [t.detach() for t in diff[at:at + n]], at + n
            if kind == "ent_coef":
                calls.append(dict(m, log_prob=d[0], log_ent_coef=d[1]))
            elif kind == "td3":
                calls.append(dict(m, q=d[0]))
            else:
                calls.append(dict(m, q=d[:n_q] if as_list else d[0], log_prob=d[n_q]))
        res = engine.actor_loss_group(kind, calls)
        ctx.grads = []
        for r, (as_list, n_q, n) in zip(res, layout):
            if kind == "ent_coef":
                ctx.grads.append([None, r.grad_log_ent_coef])
            elif kind == "td3":
                ctx.grads.append([r.grad_q])
            else:
                ctx.grads.append((list(r.grad_q) if as_list else [r.grad_q]) + [r.grad_log_prob])
        ctx.shapes = [t.shape for t in diff]
        stats = [r.stats for r in res]
        ctx.mark_non_differentiable(*stats)
        ctx.set_materialize_grads(False)
        if kind == "ent_coef":
            return (*[r.stats[1].clone() for r in res], *stats)
        firsts, at = [], 0
        for _, _, n in layout:
            firsts.append(diff[at].dtype)
            at += n
        return (*[r.stats[0].to(dt, copy=True) for r, dt in zip(res, firsts)], *stats)

    @staticmethod
    def backward(ctx, *grads):
        out, shapes = [], iter(ctx.shapes)
        for gs, g in zip(ctx.grads, grads):
            for x in gs:
                s = next(shapes)
                out.append(None if g is None or x is None else (x * g).reshape(s))
        return (None, None, None, None, *out)


def _actor_group(who, kind, engine, members, needs, scalars, q_name):
    takes = needs + ("out", "workspace") + (("ent_coef", "log_ent_coef") if kind in ("sac", "tqc") else ())
    calls = _group_members(who, members, takes, needs, scalars)
    layout, diff = [], []
    for m in calls:
        if kind == "ent_coef":
            mine, as_list, n_q = [m.pop("log_prob").detach(), m.pop("log_ent_coef")], False, 0
        elif kind == "td3":
            mine, as_list, n_q = [m.pop(q_name)], False, 1
        else:
            q = m.pop(q_name)
            as_list = isinstance(q, (list, tuple))
            qs = list(q) if as_list else [q]
            mine, n_q = qs + [m.pop("log_prob")], len(qs)
        for k in ("ent_coef", "log_ent_coef"):
            if k in m:
                m[k] = _det(m[k])
        layout.append((as_list, n_q, len(mine)))
        diff += mine
    out = _ActorLossGroupFn.apply(engine, kind, calls, layout, *diff)
    return list(out[:len(calls)]), list(out[len(calls):])


def sac_actor_loss_group(engine, members, *, ent_coef=None):
    """sac_actor_loss for G independent agents of one batch size, 1 <= G <= 8, in the launches of ONE sac_actor_loss -> (losses, stats).
    members: dicts of q (the list of K critic outputs on (obs, actions_pi)), log_prob and one of ent_coef and log_ent_coef (out,
    workspace); ent_coef: one value or a list with one per member."""
    return _actor_group("sac_actor_loss_group", "sac", engine, members, ("q", "log_prob"), dict(ent_coef=ent_coef), "q")


def tqc_actor_loss_group(engine, members, *, ent_coef=None):
    """tqc_actor_loss for G independent agents -> (losses, stats).  members: dicts of quantiles (a [B, K, Q] tensor or a list of K
    [B, Q] tensors, all members alike), log_prob and one of ent_coef and log_ent_coef (out, workspace)."""
    return _actor_group("tqc_actor_loss_group", "tqc", engine, members, ("quantiles", "log_prob"), dict(ent_coef=ent_coef), "quantiles")


def td3_actor_loss_group(engine, members):
    """td3_actor_loss for G independent agents -> (losses, stats).  members: dicts of q1 [B] / [B, 1] (out, workspace)."""
    return _actor_group("td3_actor_loss_group", "td3", engine, members, ("q1",), {}, "q1")


def ent_coef_loss_group(engine, members, *, target_entropy):
    """ent_coef_loss for G independent agents -> (losses, stats): each loss a 0-dim float64 tensor differentiable in its member's
    log_ent_coef alone; stats[i][4:5] is member i's alpha on the device.  members: dicts of log_prob, log_ent_coef (out, workspace);
    target_entropy: one value or a list with one per member."""
    return _actor_group("ent_coef_loss_group", "ent_coef", engine, members, ("log_prob", "log_ent_coef"), dict(target_entropy=target_entropy), None)
