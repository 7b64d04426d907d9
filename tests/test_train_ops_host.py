"""The training-side wrappers of the engine (vn_*, gae, minibatch, replay_*, act_*, policy_loss, td_loss, quantile_loss, actor_loss,
rsample, rsample_backward, smooth_target_action) without a device: what every accepted
call passes to the library -- each scalar, each pointer as "which tensor's data_ptr()", the order of the library calls -- pinned in one
table, and what the Python layer refuses, on CPU tensors through the engine shells of tests/helpers.py.  The marshalling table was
written against the wrappers while they still lived in engine.py and holds unchanged for rl_ptg_amd/train_ops.py; the entries of
the ops that never lived there were rendered from train_ops.py before its repeated blocks became helpers."""
import ctypes as C

import numpy as np
import pytest

from helpers import host_engine, recording_engine


# ------------------------------------------------------------------------------------------------- rendering a recorded call
def _render(calls, names):
    """the recorded library calls as one line each: pointers by the name of the tensor they came from (NULL; fresh<k> in the order of
    appearance for memory the wrapper allocated itself), structs as {field=value} without their zero / NULL fields"""
    fresh = {}

    def ptr(v):
        if not v:
            return "NULL"
        if v not in names:
            fresh.setdefault(v, f"fresh{len(fresh)}")
        return names.get(v) or fresh[v]

    def arr(a):
        items = [ptr(v) if a._type_ is C.c_void_p else str(v) for v in a]
        while items and items[-1] in ("NULL", "0"):
            items.pop()
        return "[" + ", ".join(items) + "]"

    def one(a):
        if a is None:
            return "NULL"
        if isinstance(a, C.c_void_p):
            return ptr(a.value)
        if isinstance(a, C.Array):
            return arr(a)
        if isinstance(a, C._Pointer):
            return ptr(C.cast(a, C.c_void_p).value)
        if hasattr(a, "_obj"):                                               # byref(struct)
            out = []
            for f, t in a._obj._fields_:
                v = getattr(a._obj, f)
                s = arr(v) if isinstance(v, C.Array) else ptr(v) if t is C.c_void_p else repr(v)
                if s not in ("NULL", "0", "0.0", "[]"):
                    out.append(f"{f}={s}")
            return "{" + ", ".join(out) + "}"
        return repr(a)

    return [f"{name}({', '.join(one(a) for a in args)})" for name, args in calls]


def _names(**tensors):
    out = {}
    for k, t in tensors.items():
        if t is not None:
            out.setdefault(t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr(), k)
    return out


def _storage(torch, S, N, F, dt, col_dts):
    from rl_ptg_amd.replay import ReplayStorage
    return ReplayStorage(torch.zeros(S, N, F, dtype=dt), torch.zeros(S, N, F, dtype=dt), [torch.zeros(S, N, dtype=d) for d in col_dts],
                         torch.zeros(2, dtype=torch.int64))


def _st_names(st):
    return dict(obs_ring=st.obs_ring, next_ring=st.next_ring, cursor=st.cursor, **{f"ring{c}": x for c, x in enumerate(st.col_rings)})


# ------------------------------------------------------------------------------------------------- the accepted calls
# each case: (engine, {name: tensor}) after ONE public call (minibatches: one loop) on a recording engine
N = 6


def case_vn_init():
    eng = recording_engine(N)
    eng.vn_init(0.9, 1e-6, 5.0)
    assert eng._vn_hyper == {"gamma": 0.9, "epsilon": 1e-6, "clip_reward": 5.0}
    return eng, {}


def case_vn_normalize_training_2d_fresh():
    import torch
    eng = recording_engine(N)
    rew, done = torch.zeros(4, N), torch.zeros(4, N, dtype=torch.uint8)
    res = eng.vn_normalize(rew, done)
    assert res.shape == (4, N) and res.dtype == torch.float32
    return eng, dict(rew=rew, done=done, res=res)


def case_vn_normalize_frozen_1d_out():
    import torch
    eng = recording_engine(N, out_dtype=torch.float64)
    rew, done, out = torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.bool), torch.zeros(N, dtype=torch.float64)
    res = eng.vn_normalize(rew, done, training=False, out=out)
    assert res.shape == (N,) and res.data_ptr() == out.data_ptr()
    return eng, dict(rew=rew, done=done, out=out)


def case_vn_get():
    eng = recording_engine(N)
    st, ret = eng.vn_get()
    assert st == dict(mean=0.0, var=0.0, count=0.0) and ret.shape == (N,)
    return eng, dict(returns=ret)


def case_vn_set_both():
    eng = recording_engine(N)
    ret = np.zeros(N)
    eng.vn_set(stats=dict(mean=1.0, var=2.0, count=3.0), returns=ret)
    return eng, dict(returns=ret)


def case_vn_set_nothing():
    eng = recording_engine(N)
    eng.vn_set()
    return eng, {}


def case_gae_f32_2d_fresh():
    import torch
    eng = recording_engine(N)
    rew, val, done, last = torch.zeros(20, N), torch.zeros(20, N), torch.zeros(20, N, dtype=torch.uint8), torch.zeros(N)
    adv, ret = eng.gae(rew, val, done, last, 0.99, 0.95)
    assert adv.shape == ret.shape == (20, N) and adv.dtype == torch.float32
    return eng, dict(rew=rew, values=val, done=done, last=last, adv=adv, ret=ret)


def case_gae_f64_1d_in_place():
    import torch
    eng = recording_engine(N)                                                # a float32 engine: gae takes either float dtype
    f64 = dict(dtype=torch.float64)
    rew, val, done, last = torch.zeros(N, **f64), torch.zeros(N, **f64), torch.zeros(N, dtype=torch.bool), torch.zeros(N, **f64)
    adv, ret = eng.gae(rew, val, done, last, 0.5, 1, adv=rew, ret=val)
    assert adv.shape == ret.shape == (N,) and adv.data_ptr() == rew.data_ptr()
    return eng, dict(rew=rew, values=val, done=done, last=last)


def case_minibatch_row_major_fresh():
    import torch
    eng = recording_engine(N)
    obs, c0, c1 = eng.alloc_obs(5), torch.zeros(5, N), torch.zeros(5, N, dtype=torch.uint8)
    idx = torch.zeros(64, dtype=torch.int64)
    o, outs = eng.minibatch(idx, obs, [c0, c1])
    assert o.shape == (64, 3) and [(x.shape, x.dtype) for x in outs] == [((64,), torch.float32), ((64,), torch.uint8)]
    return eng, dict(idx=idx, obs=obs, c0=c0, c1=c1, obs_out=o, out0=outs[0], out1=outs[1])


def case_minibatch_columns_only_i32_given():
    import torch
    eng = recording_engine(N)
    c0 = torch.zeros(5, N, dtype=torch.float64)
    idx, o0 = torch.zeros(7, dtype=torch.int32), torch.zeros(7, dtype=torch.float64)
    o, outs = eng.minibatch(idx, None, [c0], columns_out=[o0])
    assert o is None and outs[0] is o0
    return eng, dict(idx=idx, c0=c0, out0=o0)


def case_minibatch_feature_major_pitch():
    import torch
    eng = recording_engine(N, feature_major=True, pitch=N + 2, out_dtype=torch.float64)
    obs = eng.alloc_obs(5)
    assert obs.shape == (5, 3, N) and obs.stride() == (3 * (N + 2), N + 2, 1)
    idx, out = torch.zeros(9, dtype=torch.int64), torch.zeros(9, 3, dtype=torch.float64)
    o, outs = eng.minibatch(idx, obs, obs_out=out)
    assert o is out and outs == []
    return eng, dict(idx=idx, obs=obs, obs_out=out)


def case_minibatches_short_last_slice():
    import torch
    eng = recording_engine(N)
    c0 = torch.zeros(5, N)
    perm = torch.arange(10)
    got = [(o, outs[0]) for o, outs in eng.minibatches(perm, 4, columns=[c0])]
    assert [x.shape[0] for _, x in got] == [4, 4, 2]
    return eng, dict(perm=perm, perm4=perm[4:], perm8=perm[8:], c0=c0, out_a=got[0][1], out_b=got[1][1], out_c=got[2][1])


def case_replay_add_plain():
    import torch
    eng = recording_engine(N)
    st = _storage(torch, 8, N, 3, torch.float32, [torch.float32, torch.int64])
    obs, prev = torch.zeros(4, N, 3), torch.zeros(N, 3)
    c0, c1 = torch.zeros(4, N), torch.zeros(4, N, dtype=torch.int64)
    eng.replay_add(st, prev, obs, [c0, c1])
    return eng, dict(obs=obs, prev=prev, c0=c0, c1=c1, **_st_names(st))


def case_replay_add_done_col_final_obs_feature_major_rows():
    import torch
    eng = recording_engine(N)
    st = _storage(torch, 8, N, 3, torch.float64, [torch.float64, torch.float32])
    buf, fbuf, pbuf = (torch.zeros(2, 3, N, dtype=torch.float64), torch.zeros(2, 3, N, dtype=torch.float64), torch.zeros(3, N, dtype=torch.float64))
    obs, fo, prev = buf.transpose(1, 2), fbuf.transpose(1, 2), pbuf.t()      # the row views of feature-major buffers
    c0, done = torch.zeros(2, N, dtype=torch.float64), torch.zeros(2, N, dtype=torch.uint8)
    eng.replay_add(st, prev, obs, [c0, None], done=done, final_obs=fo, done_col=1)
    return eng, dict(obs=obs, prev=prev, final_obs=fo, c0=c0, done=done, **_st_names(st))


def case_replay_add_one_step_done_only():
    import torch
    eng = recording_engine(N)
    st = _storage(torch, 8, N, 3, torch.float32, [])
    obs, prev, done = torch.zeros(1, N, 3), torch.zeros(N, 3), torch.zeros(1, N, dtype=torch.bool)
    eng.replay_add(st, prev, obs, done=done)
    return eng, dict(obs=obs, prev=prev, done=done, **_st_names(st))


def case_replay_sample_by_index_fresh():
    import torch
    eng = recording_engine(N)
    st = _storage(torch, 8, N, 3, torch.float32, [torch.float32, torch.int64])
    idx = torch.zeros(64, dtype=torch.int64)
    o0, o1, outs, io = eng.replay_sample(st, idx=idx)
    assert o0.shape == o1.shape == (64, 3) and [x.dtype for x in outs] == [torch.float32, torch.int64] and io is None
    return eng, dict(idx=idx, o_obs=o0, o_next=o1, out0=outs[0], out1=outs[1], **_st_names(st))


def case_replay_sample_by_draw_hole_norm_col():
    import torch
    eng = recording_engine(N)
    st = _storage(torch, 8, N, 3, torch.float32, [torch.int64, torch.float32, torch.float32])
    o0, o1, outs, io = eng.replay_sample(st, batch_size=5, seed=2 ** 64 + 7, want_obs=False, want_cols=[True, False, True], norm_col=2, want_idx=True)
    assert o0 is None and o1.shape == (5, 3) and outs[1] is None and io.shape == (5,) and io.dtype == torch.int64
    return eng, dict(o_next=o1, out0=outs[0], out2=outs[2], o_idx=io, **_st_names(st))


def case_replay_sample_out_given():
    import torch
    eng = recording_engine(N)
    st = _storage(torch, 8, N, 3, torch.float32, [torch.float32])
    out = (torch.zeros(4, 3), None, [torch.zeros(4)], torch.zeros(4, dtype=torch.int64))
    got = eng.replay_sample(st, batch_size=4, seed=3, out=out)
    assert got[0] is out[0] and got[1] is None and got[2][0] is out[2][0] and got[3] is out[3]
    return eng, dict(o_obs=out[0], out0=out[2][0], o_idx=out[3], **_st_names(st))


def case_act_categorical_f32_defaults():
    import torch
    eng = recording_engine(N)
    x, cnt = torch.zeros(N, 5), eng.new_draw_counter()
    assert cnt.shape == (1,) and cnt.dtype == torch.int64 and eng._L.calls == []
    r = eng.act_categorical(x, cnt, seed=-1)
    assert r.actions.dtype == torch.int32 and r.log_prob.dtype == r.entropy.dtype == torch.float32
    return eng, dict(logits=x, counter=cnt, actions=r.actions, log_prob=r.log_prob, entropy=r.entropy)


def case_act_categorical_f64_slice_i64_deterministic():
    import torch
    eng = recording_engine(N)
    wide = torch.zeros(N, 6, dtype=torch.float64)
    x = wide[:, 1:]                                                          # 5 logits, row stride 6
    r = eng.act_categorical(x, None, deterministic=True, want_entropy=False, act_dtype=torch.int64)
    assert r.actions.dtype == torch.int64 and r.entropy is None and r.log_prob.dtype == torch.float64
    return eng, dict(logits=x, actions=r.actions, log_prob=r.log_prob)


def case_act_categorical_out_reused():
    import torch
    eng = recording_engine(N)
    x, cnt = torch.zeros(N, 2), torch.zeros(1, dtype=torch.int64)
    out = (torch.zeros(N, dtype=torch.int64), None, torch.zeros(N))
    r = eng.act_categorical(x, cnt, seed=9, out=out, want_logp=False)
    assert r.actions is out[0] and r.log_prob is None and r.entropy is out[2]
    return eng, dict(logits=x, counter=cnt, actions=out[0], entropy=out[2])


def case_act_eps_greedy_float_eps():
    import torch
    eng = recording_engine(N)
    q, cnt = torch.zeros(N, 4), torch.zeros(1, dtype=torch.int64)
    r = eng.act_eps_greedy(q, 0.25, cnt, seed=5)
    return eng, dict(q=q, counter=cnt, actions=r.actions)


def case_act_eps_greedy_tensor_eps_i64():
    import torch
    eng = recording_engine(N)
    q, cnt, eps = torch.zeros(N, 4, dtype=torch.float64), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.float64)
    r = eng.act_eps_greedy(q, eps, cnt, act_dtype=torch.int64)
    return eng, dict(q=q, counter=cnt, eps=eps, actions=r.actions)


def case_act_eps_greedy_deterministic_no_eps():
    import torch
    eng = recording_engine(N)
    q = torch.zeros(N, 4)
    r = eng.act_eps_greedy(q, None, None, deterministic=True)
    return eng, dict(q=q, actions=r.actions)


def case_act_gaussian_column_mean_plain():
    import torch
    eng = recording_engine(N)
    mean, ls, cnt = torch.zeros(N, 1), torch.zeros(1), torch.zeros(1, dtype=torch.int64)
    r = eng.act_gaussian(mean, ls, cnt, seed=11)
    assert r.actions.dtype == torch.float32 and r.raw is not None and r.entropy is not None
    return eng, dict(mean=mean, log_std=ls, counter=cnt, actions=r.actions, raw=r.raw, log_prob=r.log_prob, entropy=r.entropy)


def case_act_gaussian_squash_per_env_f64_strided_deterministic():
    import torch
    eng = recording_engine(N)
    wide = torch.zeros(N, 3, dtype=torch.float64)
    mean, ls = wide[:, 2], torch.zeros(N, dtype=torch.float64)               # stride 3
    r = eng.act_gaussian(mean, ls, None, clip=(-2, 0.5), squash=True, deterministic=True, want_raw=False)
    assert r.raw is None and r.entropy is None and r.log_prob.dtype == torch.float64 and r.actions.dtype == torch.float32
    return eng, dict(mean=mean, log_std=ls, actions=r.actions, log_prob=r.log_prob)


def case_policy_loss_workspace():
    import torch
    eng = recording_engine(N)
    ws = eng.policy_loss_workspace(300)
    assert ws.dtype == torch.uint8 and ws.shape == (32 + 2 * 88,)
    return eng, {}


def case_policy_loss_ppo_slices_clip_vf_fresh():
    import torch
    eng = recording_engine(N)
    B, A = 256, 5
    net = torch.zeros(B, A + 1)                                              # an actor-critic output: logits | value
    act, col = torch.zeros(B, dtype=torch.int64), [torch.zeros(B) for _ in range(4)]
    r = eng.policy_loss("ppo", net[:, :A], net[:, A], act, col[0], col[1], col[2], clip_range=0.2, clip_range_vf=0.3, old_values=col[3], ent_coef=0.01)
    assert r.stats.shape == (8,) and r.stats.dtype == torch.float64 and r.grad_input.shape == (B, A) and r.grad_values.shape == (B,) and r.grad_log_std is None
    return eng, dict(logits=net, values=net[:, A], actions=act, old_log_prob=col[0], advantages=col[1], returns=col[2], old_values=col[3],
                     stats=r.stats, grad_input=r.grad_input, grad_values=r.grad_values)


def case_policy_loss_a2c_gaussian_f64_out_workspace():
    import torch
    eng = recording_engine(N)
    B, f64 = 7, dict(dtype=torch.float64)
    mean, val, raw, adv, ret, ls = torch.zeros(B, 1, **f64), torch.zeros(B, 1, **f64), torch.zeros(B, **f64), torch.zeros(B, **f64), torch.zeros(B, **f64), torch.zeros(1, **f64)
    out = (torch.zeros(8, **f64), torch.zeros(B, 1, **f64), torch.zeros(B, **f64), torch.zeros(1, **f64))
    ws = torch.zeros(4096, dtype=torch.uint8)
    r = eng.policy_loss("a2c", mean, val, raw, None, adv, ret, normalize_advantage=True, vf_coef=0.25, log_std=ls, out=out, workspace=ws)
    assert r.stats is out[0] and r.grad_input.shape == (B,) and r.grad_values is out[2] and r.grad_log_std is out[3]
    return eng, dict(mean=mean, values=val, actions=raw, advantages=adv, returns=ret, log_std=ls, stats=out[0], grad_input=out[1], grad_values=out[2],
                     grad_log_std=out[3], workspace=ws)


def case_policy_loss_ppo_i32_out_views_of_one_tensor():
    import torch
    eng = recording_engine(N)
    B, A = 3, 2
    x, val, act, col = torch.zeros(B, A), torch.zeros(B), torch.zeros(B, dtype=torch.int32), torch.zeros(B)
    g = torch.zeros(B, A + 1)
    out = (torch.zeros(8, dtype=torch.float64), g[:, :A], g[:, A], None)
    r = eng.policy_loss("ppo", x, val, act, col, col, col, clip_range=0.1, normalize_advantage=False, out=out)
    assert r.grad_input is out[1]
    return eng, dict(logits=x, values=val, actions=act, col=col, stats=out[0], grad_input=g, grad_values=g[:, A])


def _views(prefix, xs):
    """the K [B, Q] views of a stacked [B, K, Q] tensor (or the K tensors of a list) under the names <prefix>0, <prefix>1, ..."""
    xs = xs if isinstance(xs, (list, tuple)) else [xs[:, k] for k in range(xs.shape[1])]
    return {f"{prefix}{k}": x for k, x in enumerate(xs)}


def case_td_loss_dqn_fresh_want_target():
    import torch
    eng = recording_engine(N)
    B, A = 300, 4
    wide = torch.zeros(B, A + 2)
    q, nq = wide[:, 1:A + 1], torch.zeros(B, A)                              # 4 Q-values, row stride 6
    act, rew, done = torch.zeros(B, dtype=torch.int64), torch.zeros(B, 1), torch.zeros(B, dtype=torch.float64)
    r = eng.td_loss("dqn", q, nq, rew, done, 0.97, actions=act, want_target=True)
    assert r.stats.shape == (8,) and r.stats.dtype == torch.float64 and r.grad_q.shape == (B, A) and r.target.shape == (B,) and r.target.dtype == torch.float32
    return eng, dict(q=q, next_q=nq, actions=act, rewards=rew, dones=done, stats=r.stats, grad_q=r.grad_q, target=r.target)


def case_td_loss_td3_critics_out_workspace():
    import torch
    eng = recording_engine(N)
    B, f64 = 5, dict(dtype=torch.float64)
    both, nboth = torch.zeros(B, 2, **f64), torch.zeros(B, 2, **f64)          # the columns of one [B, K] tensor: stride 2
    qs, nqs = [both[:, 0], both[:, 1]], (nboth[:, :1], nboth[:, 1:])
    rew, done = torch.zeros(B), torch.zeros(B, 1, **f64)
    out = (torch.zeros(8, **f64), [torch.zeros(B, **f64), torch.zeros(B, 1, **f64)], torch.zeros(B, **f64))
    ws = torch.zeros(4096, dtype=torch.uint8)
    r = eng.td_loss("td3", qs, nqs, rew, done, 0.99, out=out, workspace=ws)
    assert r.stats is out[0] and r.grad_q is out[1] and r.target is out[2]
    return eng, dict(q0=qs[0], q1=qs[1], nq0=nqs[0], nq1=nqs[1], rewards=rew, dones=done, stats=out[0], g0=out[1][0], g1=out[1][1], target=out[2],
                     workspace=ws)


def case_td_loss_sac_log_ent_coef():
    import torch
    eng = recording_engine(N)
    B = 257
    qs, nqs = [torch.zeros(B, 1), torch.zeros(B)], [torch.zeros(B), torch.zeros(B, 1)]
    rew, done, lp, la = torch.zeros(B), torch.zeros(B), torch.zeros(B, 1), torch.zeros(1, dtype=torch.float64)
    r = eng.td_loss("sac", qs, nqs, rew, done, 0.5, next_log_prob=lp, log_ent_coef=la)
    assert [tuple(g.shape) for g in r.grad_q] == [(B, 1), (B,)] and r.target is None
    return eng, dict(q0=qs[0], q1=qs[1], nq0=nqs[0], nq1=nqs[1], rewards=rew, dones=done, next_log_prob=lp, log_ent_coef=la, stats=r.stats,
                     g0=r.grad_q[0], g1=r.grad_q[1])


def case_quantile_loss_stacked_fresh():
    import torch
    eng = recording_engine(N)
    B, K, Q = 9, 2, 5
    wide = torch.zeros(B, K, Q + 1)
    q, nq = wide[:, :, :Q], torch.zeros(B, K, Q)                             # row stride K * (Q + 1), critic stride Q + 1
    rew, done, lp = torch.zeros(B, dtype=torch.float64), torch.zeros(B, 1), torch.zeros(B)
    r = eng.quantile_loss(q, nq, rew, done, lp, 0.99, 2, ent_coef=0.2, want_target=True)
    assert r.grad_quantiles.shape == (B, K, Q) and r.target.shape == (B, K * (Q - 2)) and r.stats.dtype == torch.float64
    return eng, dict(rewards=rew, dones=done, next_log_prob=lp, stats=r.stats, target=r.target, **_views("q", q), **_views("nq", nq),
                     **_views("g", r.grad_quantiles))


def case_quantile_loss_list_out():
    import torch
    eng = recording_engine(N)
    B, K, Q, f64 = 4, 3, 2, dict(dtype=torch.float64)
    qs, nqs = [torch.zeros(B, Q, **f64) for _ in range(K)], [torch.zeros(B, Q + 1, **f64)[:, 1:] for _ in range(K)]
    rew, done, lp, alpha = torch.zeros(B, 1), torch.zeros(B), torch.zeros(B, 1, **f64), torch.zeros(1, **f64)
    out = (torch.zeros(8, **f64), [torch.zeros(B, Q, **f64) for _ in range(K)], None)
    r = eng.quantile_loss(qs, nqs, rew, done, lp, 0.9, 0, ent_coef=alpha, out=out)
    assert r.stats is out[0] and r.grad_quantiles is out[1] and r.target is None
    return eng, dict(rewards=rew, dones=done, next_log_prob=lp, ent_coef=alpha, stats=out[0], **_views("q", qs), **_views("nq", nqs), **_views("g", out[1]))


def case_actor_loss_sac_target_entropy():
    import torch
    eng = recording_engine(N)
    B = 300
    both = torch.zeros(B, 2)
    qs, lp, la = [both[:, 0], both[:, 1:]], torch.zeros(B, 1), torch.zeros(1, dtype=torch.float64)
    r = eng.actor_loss("sac", qs, lp, log_ent_coef=la, target_entropy=-1.0)
    assert [tuple(g.shape) for g in r.grad_q] == [(B,), (B, 1)] and r.grad_log_prob.shape == (B, 1)
    assert r.grad_log_ent_coef.shape == (1,) and r.grad_log_ent_coef.dtype == torch.float64
    return eng, dict(q0=qs[0], q1=qs[1], log_prob=lp, log_ent_coef=la, stats=r.stats, g0=r.grad_q[0], g1=r.grad_q[1], grad_log_prob=r.grad_log_prob,
                     grad_log_ent_coef=r.grad_log_ent_coef)


def case_actor_loss_tqc_stacked():
    import torch
    eng = recording_engine(N)
    B, K, Q, f64 = 6, 2, 3, dict(dtype=torch.float64)
    q, lp = torch.zeros(B, K, Q, **f64), torch.zeros(B, **f64)
    r = eng.actor_loss("tqc", q, lp, ent_coef=0.3)
    assert r.grad_q.shape == (B, K, Q) and r.grad_log_prob.shape == (B,) and r.grad_log_ent_coef is None
    return eng, dict(log_prob=lp, stats=r.stats, grad_log_prob=r.grad_log_prob, **_views("q", q), **_views("g", r.grad_q))


def case_actor_loss_td3_bare_tensor():
    import torch
    eng = recording_engine(N)
    B = 5
    q = torch.zeros(B, 1)
    out = (torch.zeros(8, dtype=torch.float64), torch.zeros(B, 1), None, None)
    ws = torch.zeros(64, dtype=torch.uint8)
    r = eng.actor_loss("td3", q, out=out, workspace=ws)
    assert r.stats is out[0] and r.grad_q is out[1] and r.grad_log_prob is None and r.grad_log_ent_coef is None
    return eng, dict(q=q, stats=out[0], grad_q=out[1], workspace=ws)


def case_actor_loss_ent_coef():
    import torch
    eng = recording_engine(N)
    B = 7
    lp, la = torch.zeros(B, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    r = eng.actor_loss("ent_coef", log_prob=lp, log_ent_coef=la, target_entropy=-2.5)
    assert r.grad_q is None and r.grad_log_prob is None and r.grad_log_ent_coef.shape == (1,)
    return eng, dict(log_prob=lp, log_ent_coef=la, stats=r.stats, grad_log_ent_coef=r.grad_log_ent_coef)


def case_rsample_column_mean_fresh():
    import torch
    eng = recording_engine(N)
    B = 10                                                                   # B is not tied to the engine's env count
    wide = torch.zeros(B, 2)
    mean, ls, cnt = wide[:, :1], wide[:, 1], torch.zeros(1, dtype=torch.int64)      # the two columns of one actor output: stride 2
    r = eng.rsample(mean, ls, cnt, seed=-3)
    assert r.actions.shape == r.log_prob.shape == r.noise.shape == (B, 1) and r.noise.dtype == torch.float64 and r.actions.dtype == torch.float32
    return eng, dict(mean=mean, log_std=ls, counter=cnt, actions=r.actions, log_prob=r.log_prob, noise=r.noise)


def case_rsample_f64_deterministic_out():
    import torch
    eng = recording_engine(N)
    B, f64 = 4, dict(dtype=torch.float64)
    mean, ls = torch.zeros(B, **f64), torch.zeros(B, 1, **f64)
    out = (torch.zeros(B, 1, **f64), None, torch.zeros(B, **f64))
    r = eng.rsample(mean, ls, None, deterministic=True, out=out)
    assert r.actions is out[0] and r.log_prob is None and r.noise is out[2]
    return eng, dict(mean=mean, log_std=ls, actions=out[0], noise=out[2])


def case_rsample_backward_fresh_one_gradient():
    import torch
    eng = recording_engine(N)
    B = 10
    wide = torch.zeros(B, 2)
    mean, ls, noise, gl = wide[:, 0], wide[:, 1:], torch.zeros(B, dtype=torch.float64), torch.zeros(B, 1)
    r = eng.rsample_backward(mean, ls, noise, None, gl)
    assert r.grad_mean.shape == (B,) and r.grad_log_std.shape == (B, 1) and r.grad_mean.dtype == torch.float32
    return eng, dict(mean=mean, log_std=ls, noise=noise, grad_log_prob=gl, grad_mean=r.grad_mean, grad_log_std=r.grad_log_std)


def case_rsample_backward_f64_out_strided():
    import torch
    eng = recording_engine(N)
    B, f64 = 3, dict(dtype=torch.float64)
    mean, ls, noise, ga, gl = torch.zeros(B, 1, **f64), torch.zeros(B, **f64), torch.zeros(B, 1, **f64), torch.zeros(B, **f64), torch.zeros(B, **f64)
    g = torch.zeros(B, 2, **f64)
    out = (g[:, 0], g[:, 1:])
    r = eng.rsample_backward(mean, ls, noise, ga, gl, out=out)
    assert r.grad_mean is out[0] and r.grad_log_std is out[1]
    return eng, dict(mean=mean, log_std=ls, noise=noise, grad_actions=ga, grad_log_prob=gl, grad_mean=out[0], grad_log_std=out[1])


def case_smooth_target_action_fresh():
    import torch
    eng = recording_engine(N)
    B = 8
    mean, cnt = torch.zeros(B, 3)[:, 2], torch.zeros(1, dtype=torch.int64)   # stride 3
    r = eng.smooth_target_action(mean, cnt, 0.2, 0.5, seed=2 ** 64 + 4)
    assert r.shape == (B,) and r.dtype == torch.float32
    return eng, dict(mean=mean, counter=cnt, out=r)


def case_smooth_target_action_f64_column_out():
    import torch
    eng = recording_engine(N)
    B, f64 = 5, dict(dtype=torch.float64)
    mean, cnt, out = torch.zeros(B, 1, **f64), torch.zeros(1, dtype=torch.int64), torch.zeros(B, 1, **f64)
    r = eng.smooth_target_action(mean, cnt, 0.0, 0.0, clip=(-2, 0.5), out=out)
    assert r is out
    return eng, dict(mean=mean, counter=cnt, out=out)


# what the wrappers passed while they lived in engine.py (rendered by _render): 'H' the handle, the last argument the stream
EXPECTED = {
    "act_categorical_f32_defaults": [
        "ptg_act('H', {n_actions=5, in_dev=logits, in_s_n=5, seed=18446744073709551615, counter_dev=counter, act_dev=actions, logp_dev=log_prob, ent_dev=entropy}, NULL)",
    ],
    "act_categorical_f64_slice_i64_deterministic": [
        "ptg_act('H', {flags=1, n_actions=5, in_dtype=1, in_dev=logits, in_s_n=6, act_kind=2, act_dev=actions, logp_dev=log_prob}, NULL)",
    ],
    "act_categorical_out_reused": [
        "ptg_act('H', {n_actions=2, in_dev=logits, in_s_n=2, act_kind=2, seed=9, counter_dev=counter, act_dev=actions, ent_dev=entropy}, NULL)",
    ],
    "act_eps_greedy_deterministic_no_eps": [
        "ptg_act('H', {kind=1, flags=1, n_actions=4, in_dev=q, in_s_n=4, act_dev=actions}, NULL)",
    ],
    "act_eps_greedy_float_eps": [
        "ptg_act('H', {kind=1, n_actions=4, in_dev=q, in_s_n=4, param_dev=fresh0, seed=5, counter_dev=counter, act_dev=actions}, NULL)",
    ],
    "act_eps_greedy_tensor_eps_i64": [
        "ptg_act('H', {kind=1, n_actions=4, in_dtype=1, in_dev=q, in_s_n=4, param_dev=eps, act_kind=2, counter_dev=counter, act_dev=actions}, NULL)",
    ],
    "act_gaussian_column_mean_plain": [
        "ptg_act('H', {kind=2, in_dev=mean, in_s_n=1, param_dev=log_std, act_kind=1, clip_lo=-1.0, clip_hi=1.0, seed=11, counter_dev=counter, act_dev=actions, raw_dev=raw, logp_dev=log_prob, ent_dev=entropy}, NULL)",
    ],
    "act_gaussian_squash_per_env_f64_strided_deterministic": [
        "ptg_act('H', {kind=2, flags=3, in_dtype=1, in_dev=mean, in_s_n=3, param_dev=log_std, param_s_n=1, act_kind=1, clip_lo=-2.0, clip_hi=0.5, act_dev=actions, logp_dev=log_prob}, NULL)",
    ],
    "actor_loss_ent_coef": [
        "ptg_actor_loss_workspace(7)",
        "ptg_actor_loss('H', {kind=2, flags=6, n_quantiles=1, q_dtype=1, batch=7, logp_dev=log_prob, alpha_dev=log_ent_coef, target_entropy=-2.5, stats_dev=stats, grad_log_alpha_dev=grad_log_ent_coef}, NULL)",
    ],
    "actor_loss_sac_target_entropy": [
        "ptg_actor_loss_workspace(300)",
        "ptg_actor_loss('H', {flags=7, n_critics=2, n_quantiles=1, batch=300, q_dev=[q0, q1], q_s_n=[2, 2], logp_dev=log_prob, alpha_dev=log_ent_coef, target_entropy=-1.0, stats_dev=stats, grad_q_dev=[g0, g1], g_s_n=[1, 1], grad_logp_dev=grad_log_prob, grad_log_alpha_dev=grad_log_ent_coef}, NULL)",
    ],
    "actor_loss_td3_bare_tensor": [
        "ptg_actor_loss_workspace(5)",
        "ptg_actor_loss('H', {kind=1, n_critics=1, n_quantiles=1, batch=5, q_dev=[q], q_s_n=[1], stats_dev=stats, grad_q_dev=[grad_q], g_s_n=[1], ws_dev=workspace}, NULL)",
    ],
    "actor_loss_tqc_stacked": [
        "ptg_actor_loss_workspace(6)",
        "ptg_actor_loss('H', {kind=1, flags=1, n_critics=2, n_quantiles=3, q_dtype=1, batch=6, q_dev=[q0, q1], q_s_n=[6, 6], logp_dev=log_prob, alpha=0.3, stats_dev=stats, grad_q_dev=[g0, g1], g_s_n=[6, 6], grad_logp_dev=grad_log_prob}, NULL)",
    ],
    "gae_f32_2d_fresh": [
        "ptg_gae('H', rew, values, done, last, 20, 0, 0.99, 0.95, adv, ret, NULL)",
    ],
    "gae_f64_1d_in_place": [
        "ptg_gae('H', rew, values, done, last, 1, 1, 0.5, 1.0, rew, values, NULL)",
    ],
    "minibatch_columns_only_i32_given": [
        "ptg_minibatch('H', idx, 4, 7, 5, NULL, 0, 0, 0, 0, 0, NULL, 1, [c0], [8], [out0], NULL)",
    ],
    "minibatch_feature_major_pitch": [
        "ptg_minibatch('H', idx, 8, 9, 5, obs, 24, 1, 8, 3, 8, obs_out, 0, [], [], [], NULL)",
    ],
    "minibatch_row_major_fresh": [
        "ptg_minibatch('H', idx, 8, 64, 5, obs, 18, 3, 1, 3, 4, obs_out, 2, [c0, c1], [4, 1], [out0, out1], NULL)",
    ],
    "minibatches_short_last_slice": [
        "ptg_minibatch('H', perm, 8, 4, 5, NULL, 0, 0, 0, 0, 0, NULL, 1, [c0], [4], [out_a], NULL)",
        "ptg_minibatch('H', perm4, 8, 4, 5, NULL, 0, 0, 0, 0, 0, NULL, 1, [c0], [4], [out_b], NULL)",
        "ptg_minibatch('H', perm8, 8, 2, 5, NULL, 0, 0, 0, 0, 0, NULL, 1, [c0], [4], [out_c], NULL)",
    ],
    "policy_loss_a2c_gaussian_f64_out_workspace": [
        "ptg_policy_loss_workspace(7)",
        "ptg_policy_loss('H', {kind=1, head=2, flags=1, in_dtype=1, batch=7, in_dev=mean, in_s_n=1, val_dev=values, val_s_n=1, act_dev=actions, adv_dev=advantages, ret_dev=returns, log_std_dev=log_std, vf_coef=0.25, stats_dev=stats, grad_in_dev=grad_input, g_s_n=1, grad_val_dev=grad_values, gv_s_n=1, grad_log_std_dev=grad_log_std, ws_dev=workspace}, NULL)",
    ],
    "policy_loss_ppo_i32_out_views_of_one_tensor": [
        "ptg_policy_loss_workspace(3)",
        "ptg_policy_loss('H', {n_actions=2, batch=3, in_dev=logits, in_s_n=2, val_dev=values, val_s_n=1, act_dev=actions, old_logp_dev=col, adv_dev=col, ret_dev=col, clip_range=0.1, vf_coef=0.5, stats_dev=stats, grad_in_dev=grad_input, g_s_n=3, grad_val_dev=grad_values, gv_s_n=3, ws_dev=fresh0}, NULL)",
    ],
    "policy_loss_ppo_slices_clip_vf_fresh": [
        "ptg_policy_loss_workspace(256)",
        "ptg_policy_loss('H', {flags=3, n_actions=5, act_kind=2, batch=256, in_dev=logits, in_s_n=6, val_dev=values, val_s_n=6, act_dev=actions, old_logp_dev=old_log_prob, adv_dev=advantages, ret_dev=returns, old_val_dev=old_values, clip_range=0.2, clip_range_vf=0.3, ent_coef=0.01, vf_coef=0.5, stats_dev=stats, grad_in_dev=grad_input, g_s_n=5, grad_val_dev=grad_values, gv_s_n=1, ws_dev=fresh0}, NULL)",
    ],
    "policy_loss_workspace": [
        "ptg_policy_loss_workspace(300)",
    ],
    "quantile_loss_list_out": [
        "ptg_quantile_loss_workspace(4)",
        "ptg_quantile_loss('H', {n_critics=3, n_quantiles=2, q_dtype=1, batch=4, cur_dev=[q0, q1, q2], cur_s_n=[2, 2, 2], next_dev=[nq0, nq1, nq2], next_s_n=[3, 3, 3], grad_dev=[g0, g1, g2], g_s_n=[2, 2, 2], rew_dev=rewards, done_dev=dones, next_logp_dev=next_log_prob, alpha_dev=ent_coef, gamma=0.9, stats_dev=stats}, NULL)",
    ],
    "quantile_loss_stacked_fresh": [
        "ptg_quantile_loss_workspace(9)",
        "ptg_quantile_loss('H', {n_critics=2, n_quantiles=5, n_drop=2, rew_dtype=1, batch=9, cur_dev=[q0, q1], cur_s_n=[12, 12], next_dev=[nq0, nq1], next_s_n=[10, 10], grad_dev=[g0, g1], g_s_n=[10, 10], rew_dev=rewards, done_dev=dones, next_logp_dev=next_log_prob, gamma=0.99, alpha=0.2, stats_dev=stats, y_dev=target}, NULL)",
    ],
    "replay_add_done_col_final_obs_feature_major_rows": [
        "ptg_replay_add('H', {capacity=8, obs_dim=3, obs_bytes=8, obs_ring=obs_ring, next_ring=next_ring, n_cols=2, col_bytes=[8, 4], col_ring=[ring0, ring1], cursor_dev=cursor}, prev, obs, 18, 1, 6, final_obs, done, 1, 2, [c0], 2, NULL)",
    ],
    "replay_add_one_step_done_only": [
        "ptg_replay_add('H', {capacity=8, obs_dim=3, obs_bytes=4, obs_ring=obs_ring, next_ring=next_ring, cursor_dev=cursor}, prev, obs, 18, 3, 1, NULL, done, -1, 0, [], 1, NULL)",
    ],
    "replay_add_plain": [
        "ptg_replay_add('H', {capacity=8, obs_dim=3, obs_bytes=4, obs_ring=obs_ring, next_ring=next_ring, n_cols=2, col_bytes=[4, 8], col_ring=[ring0, ring1], cursor_dev=cursor}, prev, obs, 18, 3, 1, NULL, NULL, -1, 2, [c0, c1], 4, NULL)",
    ],
    "replay_sample_by_draw_hole_norm_col": [
        "ptg_replay_sample('H', {capacity=8, obs_dim=3, obs_bytes=4, obs_ring=obs_ring, next_ring=next_ring, n_cols=3, col_bytes=[8, 4, 4], col_ring=[ring0, ring1, ring2], cursor_dev=cursor}, NULL, 5, 7, NULL, o_next, [out0, NULL, out2], 2, o_idx, NULL)",
    ],
    "replay_sample_by_index_fresh": [
        "ptg_replay_sample('H', {capacity=8, obs_dim=3, obs_bytes=4, obs_ring=obs_ring, next_ring=next_ring, n_cols=2, col_bytes=[4, 8], col_ring=[ring0, ring1], cursor_dev=cursor}, idx, 64, 0, o_obs, o_next, [out0, out1], -1, NULL, NULL)",
    ],
    "replay_sample_out_given": [
        "ptg_replay_sample('H', {capacity=8, obs_dim=3, obs_bytes=4, obs_ring=obs_ring, next_ring=next_ring, n_cols=1, col_bytes=[4], col_ring=[ring0], cursor_dev=cursor}, NULL, 4, 3, o_obs, NULL, [out0], -1, o_idx, NULL)",
    ],
    "rsample_backward_f64_out_strided": [
        "ptg_rsample_backward('H', {q_dtype=1, batch=3, mean_dev=mean, mean_s_n=1, log_std_dev=log_std, log_std_s_n=1, noise_dev=noise, grad_act_dev=grad_actions, grad_logp_dev=grad_log_prob, grad_mean_dev=grad_mean, gm_s_n=2, grad_log_std_dev=grad_log_std, gl_s_n=2}, NULL)",
    ],
    "rsample_backward_fresh_one_gradient": [
        "ptg_rsample_backward('H', {batch=10, mean_dev=mean, mean_s_n=2, log_std_dev=log_std, log_std_s_n=2, noise_dev=noise, grad_logp_dev=grad_log_prob, grad_mean_dev=grad_mean, gm_s_n=1, grad_log_std_dev=grad_log_std, gl_s_n=1}, NULL)",
    ],
    "rsample_column_mean_fresh": [
        "ptg_rsample('H', {batch=10, mean_dev=mean, mean_s_n=2, log_std_dev=log_std, log_std_s_n=2, seed=18446744073709551613, counter_dev=counter, act_dev=actions, logp_dev=log_prob, noise_dev=noise}, NULL)",
    ],
    "rsample_f64_deterministic_out": [
        "ptg_rsample('H', {flags=1, q_dtype=1, batch=4, mean_dev=mean, mean_s_n=1, log_std_dev=log_std, log_std_s_n=1, act_dev=actions, noise_dev=noise}, NULL)",
    ],
    "smooth_target_action_f64_column_out": [
        "ptg_rsample('H', {kind=1, q_dtype=1, batch=5, mean_dev=mean, mean_s_n=1, counter_dev=counter, clip_lo=-2.0, clip_hi=0.5, act_dev=out}, NULL)",
    ],
    "smooth_target_action_fresh": [
        "ptg_rsample('H', {kind=1, batch=8, mean_dev=mean, mean_s_n=3, seed=4, counter_dev=counter, noise_std=0.2, noise_clip=0.5, clip_lo=-1.0, clip_hi=1.0, act_dev=out}, NULL)",
    ],
    "td_loss_dqn_fresh_want_target": [
        "ptg_td_loss_workspace(300)",
        "ptg_td_loss('H', {n_actions=4, act_kind=2, done_dtype=1, batch=300, q_dev=[q], q_s_n=[6], next_q_dev=[next_q], next_s_n=[4], act_dev=actions, rew_dev=rewards, done_dev=dones, gamma=0.97, scale=1.0, stats_dev=stats, grad_q_dev=[grad_q], g_s_n=[4], y_dev=target}, NULL)",
    ],
    "td_loss_sac_log_ent_coef": [
        "ptg_td_loss_workspace(257)",
        "ptg_td_loss('H', {kind=1, flags=3, n_critics=2, batch=257, q_dev=[q0, q1], q_s_n=[1, 1], next_q_dev=[nq0, nq1], next_s_n=[1, 1], rew_dev=rewards, done_dev=dones, next_logp_dev=next_log_prob, alpha_dev=log_ent_coef, gamma=0.5, scale=0.5, stats_dev=stats, grad_q_dev=[g0, g1], g_s_n=[1, 1]}, NULL)",
    ],
    "td_loss_td3_critics_out_workspace": [
        "ptg_td_loss_workspace(5)",
        "ptg_td_loss('H', {kind=1, n_critics=2, q_dtype=1, done_dtype=1, batch=5, q_dev=[q0, q1], q_s_n=[2, 2], next_q_dev=[nq0, nq1], next_s_n=[2, 2], rew_dev=rewards, done_dev=dones, gamma=0.99, scale=1.0, stats_dev=stats, grad_q_dev=[g0, g1], g_s_n=[1, 1], y_dev=target, ws_dev=workspace}, NULL)",
    ],
    "vn_get": [
        "ptg_vn_get('H', fresh0, returns)",
    ],
    "vn_init": [
        "ptg_vn_init('H', 0.9, 1e-06, 5.0)",
    ],
    "vn_normalize_frozen_1d_out": [
        "ptg_vn_apply('H', rew, 1, NULL, out, 0, NULL)",
        "ptg_vn_clear_done('H', done, 1, NULL)",
    ],
    "vn_normalize_training_2d_fresh": [
        "ptg_vn_batch_moments('H', rew, done, 4, fresh0, NULL)",
        "ptg_vn_apply('H', rew, 4, fresh0, res, 1, NULL)",
    ],
    "vn_set_both": [
        "ptg_vn_set('H', fresh0, returns)",
    ],
    "vn_set_nothing": [
        "ptg_vn_set('H', NULL, NULL)",
    ],
}


CASES = sorted(k for k in globals() if k.startswith("case_"))


@pytest.mark.parametrize("case", CASES)
def test_what_reaches_the_library(case):
    eng, tensors = globals()[case]()
    assert _render(eng._L.calls, _names(**tensors)) == EXPECTED[case[5:]]


# ------------------------------------------------------------------------------------------------- what the Python layer refuses
# the cases of the GPU-marked tables (tests/test_gae.py, tests/test_minibatch.py, tests/test_replay.py) that never reach the library,
# on CPU tensors; "another device" is torch.device("meta").  The shell has no library: an accepted call would die on eng._L = None.
def _refusing_engine(n):
    from helpers import CpuTorch
    return host_engine(n, _torch=CpuTorch())


def _all_refused(eng, refused):
    for k, (exc, call) in enumerate(refused):
        with pytest.raises(exc):
            call()
        assert eng._L is None, k


def test_gae_refusals_need_no_device():
    import torch
    T = 4
    eng = _refusing_engine(N)
    r, v, d, l = torch.zeros(T, N), torch.zeros(T, N), torch.zeros(T, N, dtype=torch.uint8), torch.zeros(N)
    adv, ret = torch.zeros(T, N), torch.zeros(T, N)
    other = torch.device("meta")
    g = lambda *a, **kw: eng.gae(*a, 0.99, 0.95, **kw)
    _all_refused(eng, [
        (ValueError, lambda: g(r[:, :3], v[:, :3], d[:, :3], l[:3])),
        (ValueError, lambda: g(r, v[:T - 1], d, l)),
        (ValueError, lambda: g(r, v, d, torch.zeros(N, 1))),
        (ValueError, lambda: g(r.t().contiguous().t(), v, d, l, adv=adv, ret=ret)),
        (ValueError, lambda: g(r, v, d.t().contiguous().t(), l, adv=adv, ret=ret)),
        (ValueError, lambda: g(r, v, d, torch.zeros(2 * N)[::2], adv=adv, ret=ret)),
        (TypeError, lambda: g(r, v.double(), d, l, adv=adv, ret=ret)),
        (TypeError, lambda: g(r, v, d, l.double(), adv=adv, ret=ret)),
        (TypeError, lambda: g(r.half(), v.half(), d, l.half())),
        (TypeError, lambda: g(r.long(), v.long(), d, l.long())),
        (TypeError, lambda: g(r, v, d.int(), l, adv=adv, ret=ret)),
        (ValueError, lambda: g(r, v, d, l, adv=adv.double(), ret=ret)),
        (ValueError, lambda: g(r, v, d, l, adv=adv, ret=ret[:T - 1])),
        (ValueError, lambda: g(r, v, d, l, adv=adv.t().contiguous().t(), ret=ret)),
        (ValueError, lambda: g(r.to(other), v, d, l, adv=adv, ret=ret)),
        (ValueError, lambda: g(r, v, d.to(other), l, adv=adv, ret=ret)),
        (ValueError, lambda: g(r, v, d, l.to(other), adv=adv, ret=ret)),
        (ValueError, lambda: g(r, v, d, l, adv=adv, ret=ret.to(other))),
    ])


def test_minibatch_refusals_need_no_device():
    import torch
    T, B, F = 5, 10, 3
    eng = _refusing_engine(N)
    obs, col = torch.zeros(T, N, F), torch.zeros(T, N, dtype=torch.int32)
    idx = torch.zeros(B, dtype=torch.int64)
    out, out_c = torch.zeros(B, F), torch.zeros(B, dtype=torch.int32)
    other = torch.device("meta")
    m = lambda *a, **kw: eng.minibatch(*a, obs_out=kw.pop("obs_out", out), columns_out=kw.pop("columns_out", [out_c]), **kw)
    _all_refused(eng, [
        (TypeError, lambda: m(idx.float(), obs, [col])),
        (TypeError, lambda: m(idx.to(torch.int16), obs, [col])),
        (TypeError, lambda: m(idx.numpy(), obs, [col])),                                 # a host array
        (ValueError, lambda: m(idx.view(2, 5), obs, [col])),
        (ValueError, lambda: m(torch.cat([idx, idx])[::2], obs, [col])),                 # 1-D, strided
        (ValueError, lambda: m(idx.to(other), obs, [col])),                              # wrong device
        (ValueError, lambda: m(idx, obs.to(other), [col])),
        (ValueError, lambda: m(idx, obs, [col.to(other)])),
        (ValueError, lambda: m(idx, obs, [col], obs_out=out.to(other))),
        (ValueError, lambda: m(idx, obs, [col], columns_out=[out_c.to(other)])),
        (ValueError, lambda: m(idx, obs, [col[:T - 1]])),                                # columns that are not [T, N]
        (ValueError, lambda: m(idx, obs, [col[:, :N - 1]])),
        (ValueError, lambda: m(idx, obs, [col.t()])),
        (ValueError, lambda: m(idx, obs, [col.view(-1)])),
        (ValueError, lambda: m(idx, obs, [col.t().contiguous().t()])),                   # [T, N], not contiguous
        (ValueError, lambda: m(idx, None, [col.t().contiguous()], obs_out=None)),        # columns only: T from the column, N wrong
        (TypeError, lambda: m(idx, obs, [col.to(torch.complex128)])),                    # 16-byte elements
        (ValueError, lambda: m(idx, obs[:, :, :F - 1], [col])),                          # not a buffer of alloc_obs
        (ValueError, lambda: m(idx, obs[:, :N - 1], [col])),
        (ValueError, lambda: m(idx, obs[0], [col])),
        (ValueError, lambda: m(idx, obs.transpose(1, 2).contiguous().transpose(1, 2), [col])),     # the shape, other strides
        (TypeError, lambda: m(idx, obs.half(), [col])),
        (ValueError, lambda: m(idx, obs, [col], obs_out=out[:B - 1])),                   # mismatched outputs
        (ValueError, lambda: m(idx, obs, [col], obs_out=out.double())),
        (ValueError, lambda: m(idx, obs, [col], obs_out=torch.zeros(F, B).t())),
        (ValueError, lambda: m(idx, obs, [col], columns_out=[out_c[:B - 1]])),
        (ValueError, lambda: m(idx, obs, [col], columns_out=[out_c.float()])),
        (ValueError, lambda: m(idx, obs, [col], columns_out=[])),
        (ValueError, lambda: m(idx, obs, [col], columns_out=[out_c, out_c])),
        (ValueError, lambda: m(idx, None, [col])),                                       # an output for observations that are not given
        (ValueError, lambda: m(idx, obs, [col] * 9, columns_out=[out_c] * 9)),           # more than 8 columns
        (ValueError, lambda: m(idx, None, [], obs_out=None, columns_out=None)),          # nothing to gather
        (ValueError, lambda: list(eng.minibatches(idx, 0, obs, [col]))),
    ])
    fm = _refusing_engine(N)
    fm.feature_major, fm.pitch = True, N + 2
    _all_refused(fm, [(ValueError, lambda: fm.minibatch(idx, torch.zeros(T, F, N)))])   # feature-major without the engine's pitch


def test_replay_refusals_need_no_device():
    import torch
    S, F, T, B = 5, 3, 3, 4
    eng = _refusing_engine(N)
    st = _storage(torch, S, N, F, torch.float32, [torch.float64, torch.float32])
    prev, obs, fo, done = torch.zeros(N, F), torch.zeros(T, N, F), torch.zeros(T, N, F), torch.zeros(T, N, dtype=torch.uint8)
    col8 = torch.zeros(T, N, dtype=torch.float64)
    idx = torch.zeros(B, dtype=torch.int64)
    out = (torch.zeros(B, F), torch.zeros(B, F), [torch.zeros(B, dtype=torch.float64), torch.zeros(B)], torch.zeros(B, dtype=torch.int64))
    other = torch.device("meta")
    add = lambda **kw: eng.replay_add(kw.pop("st", st), kw.pop("prev", prev), kw.pop("obs", obs), kw.pop("cols", [col8, None]), done=kw.pop("done", done),
                                      final_obs=kw.pop("fo", fo), done_col=kw.pop("done_col", 1))
    smp = lambda **kw: eng.replay_sample(kw.pop("st", st), idx=kw.pop("idx", idx), out=kw.pop("out", out), **kw)
    ring_h, ring_n = st.obs_ring.half(), torch.zeros(S, N + 1, F)
    _all_refused(eng, [
        (ValueError, lambda: add(obs=torch.zeros(S + 1, N, F), fo=None)),                # T = S + 1
        (ValueError, lambda: add(obs=obs[:0], fo=None)),                                 # T = 0
        (ValueError, lambda: add(obs=obs[0])),                                           # not a window
        (ValueError, lambda: add(obs=obs[:, :N - 1])),
        (ValueError, lambda: add(obs=obs[:, :, :F - 1])),
        (ValueError, lambda: add(obs=obs.to(other))),
        (TypeError, lambda: add(obs=obs.double())),
        (ValueError, lambda: add(prev=prev.t().contiguous().t())),                       # prev_obs with other strides
        (ValueError, lambda: add(prev=prev[:N - 1])),
        (ValueError, lambda: add(fo=torch.zeros(T, F, N).transpose(1, 2))),              # final_obs with other strides
        (ValueError, lambda: add(fo=fo[:T - 1])),
        (ValueError, lambda: add(cols=[col8])),                                          # one column for two rings
        (ValueError, lambda: add(cols=[col8[:T - 1], None])),
        (ValueError, lambda: add(cols=[col8.t().contiguous().t(), None])),               # [T, N], not contiguous
        (ValueError, lambda: add(cols=[col8.to(other), None])),
        (TypeError, lambda: add(cols=[col8.float(), None])),                             # not the ring's dtype
        (ValueError, lambda: add(cols=[None, None])),                                    # a missing column
        (ValueError, lambda: add(done=None)),                                            # final_obs and the done column need done
        (TypeError, lambda: add(done=done.int())),
        (ValueError, lambda: add(done=done[:T - 1])),
        (ValueError, lambda: add(done=done.to(other))),
        (ValueError, lambda: add(done_col=2)),
        (TypeError, lambda: add(done_col=0)),                                            # an 8-byte done column
        (TypeError, lambda: add(st=st._replace(col_rings=[st.col_rings[0], torch.zeros(S, N, dtype=torch.int32)]))),      # a 4-byte done ring, not float32
        (TypeError, lambda: add(st=st._replace(cursor=st.cursor.float()))),
        (ValueError, lambda: add(st=st._replace(cursor=st.cursor.to(other)))),
        (TypeError, lambda: add(st=st._replace(obs_ring=ring_h, next_ring=ring_h))),
        (ValueError, lambda: add(st=st._replace(obs_ring=torch.zeros(S, F, N).transpose(1, 2)))),                         # a ring that is not contiguous
        (ValueError, lambda: add(st=st._replace(obs_ring=ring_n, next_ring=ring_n))),    # rings of another env count
        (ValueError, lambda: add(st=st._replace(col_rings=[st.col_rings[0][:S - 1], st.col_rings[1]]))),
        (ValueError, lambda: add(st=st._replace(col_rings=[st.col_rings[0]] * 9), cols=[col8] * 9, done_col=-1)),
        (TypeError, lambda: smp(idx=idx.int())),
        (TypeError, lambda: smp(idx=idx.numpy())),
        (ValueError, lambda: smp(idx=idx.to(other))),
        (ValueError, lambda: smp(idx=idx.view(2, 2))),
        (ValueError, lambda: smp(idx=torch.cat([idx, idx])[::2])),
        (ValueError, lambda: smp(batch_size=B + 1)),
        (ValueError, lambda: smp(idx=None)),                                             # neither indices nor a batch size
        (ValueError, lambda: smp(idx=None, batch_size=0)),
        (ValueError, lambda: smp(out=(out[0].double(), out[1], out[2], out[3]))),
        (ValueError, lambda: smp(out=(torch.zeros(F, B).t(), out[1], out[2], out[3]))),
        (ValueError, lambda: smp(out=(out[0][:B - 1], out[1], out[2], out[3]))),
        (ValueError, lambda: smp(out=(out[0], out[1].to(other), out[2], out[3]))),
        (ValueError, lambda: smp(out=(out[0], out[1], [torch.zeros(B), out[2][1]], out[3]))),
        (ValueError, lambda: smp(out=(out[0], out[1], out[2][:1], out[3]))),
        (ValueError, lambda: smp(out=(None, None, [None, None], None))),                 # no output
        (ValueError, lambda: smp(out=(out[0], out[1], [out[2][0], None], out[3]), norm_col=1)),          # norm_col without an output
        (ValueError, lambda: smp(want_cols=[True])),
        (ValueError, lambda: smp(norm_col=2)),
        (TypeError, lambda: smp(norm_col=0)),                                            # a float64 column on a float32 engine
    ])


def test_vn_normalize_refusals_need_no_device():
    """vn_normalize raises like the other wrappers (it used to assert, and checked neither out nor any device)"""
    import torch
    T = 4
    eng = _refusing_engine(N)
    rew, done, out = torch.zeros(T, N), torch.zeros(T, N, dtype=torch.uint8), torch.zeros(T, N)
    other = torch.device("meta")
    vn = lambda r=rew, d=done, **kw: eng.vn_normalize(r, d, **kw)
    _all_refused(eng, [
        (TypeError, lambda: vn(rew.numpy())), (TypeError, lambda: vn(d=done.numpy())),
        (TypeError, lambda: vn(rew.double())), (TypeError, lambda: vn(rew.half())),                     # not the engine's out_dtype
        (TypeError, lambda: vn(d=done.int())), (TypeError, lambda: vn(d=done.float())),                 # 4-byte done flags
        (ValueError, lambda: vn(rew[:, :N - 1], done[:, :N - 1])), (ValueError, lambda: vn(torch.zeros(T, N, 1))),
        (ValueError, lambda: vn(rew[0], done)), (ValueError, lambda: vn(rew, done[:T - 1])), (ValueError, lambda: vn(rew, done[0])),
        (ValueError, lambda: vn(rew.t().contiguous().t())), (ValueError, lambda: vn(d=done.t().contiguous().t())),
        (ValueError, lambda: vn(torch.zeros(2 * N)[::2], done[0])),
        (ValueError, lambda: vn(rew.to(other))), (ValueError, lambda: vn(d=done.to(other))),
        (TypeError, lambda: vn(out=out.numpy())), (TypeError, lambda: vn(out=out.double())),
        (ValueError, lambda: vn(out=out[:T - 1])), (ValueError, lambda: vn(out=out[0])), (ValueError, lambda: vn(out=out.t().contiguous().t())),
        (ValueError, lambda: vn(out=out.to(other))), (ValueError, lambda: vn(training=False, out=out.to(other))),
    ])
