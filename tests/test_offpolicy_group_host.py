"""ptg_td_loss_group / ptg_actor_loss_group / ptg_rsample_group / ptg_rsample_backward_group without a device: the header's
declarations and the exported symbols, what the library refuses on a NULL handle, every Python-level refusal of HipEngine.td_loss_group /
actor_loss_group / rsample_group / rsample_backward_group / smooth_target_action_group (the single op's words behind "member i:", nothing
touched), the descriptor arrays an accepted three-member call hands the library, and a group of one against the single op (the same
descriptor bytes).  The arithmetic has no test here: a grouped call is defined as the single calls, which tests/test_offpolicy_group.py
compares bit for bit on the device."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"ptg_td_loss_group": "ptg_td", "ptg_actor_loss_group": "ptg_al", "ptg_rsample_group": "ptg_rs", "ptg_rsample_backward_group": "ptg_rs"}


# ------------------------------------------------------------------------------------------------- the ABI, without a device
def test_the_header_declares_the_four_entries_and_the_library_exports_them():
    from rl_ptg_amd import _lib
    _lib.build()
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "ptg_env.h")).read()
    for name, desc in ENTRIES.items():
        assert hasattr(L, name) and name in _lib.EXPORTS
        assert f"int {name}(ptg_env* env, const {desc}* members, int32_t n_members, void* stream);" in hdr
    assert L.ptg_abi_version() == 13 and "#define PTG_ABI_VERSION 13" in hdr and "#define PTG_TRAIN_GROUP_MAX 8" in hdr
    # eight members by value in the launch arguments: the header states the sizes; the descriptors themselves are no larger than the limit either
    assert "8 x 328 = 2 624" in hdr and "8 x 232 = 1 856" in hdr and "8 x 176 = 1 408" in hdr
    assert all(8 * C.sizeof(T) <= 4096 for T in (_lib.PtgTd, _lib.PtgAl, _lib.PtgRs))


def test_a_null_handle_without_a_device():
    """no handle exists without a device: array and counts are refused with a handle in tests/test_offpolicy_group.py"""
    from rl_ptg_amd import _lib
    L = _lib.lib()
    for name, T in (("ptg_td_loss_group", _lib.PtgTd), ("ptg_actor_loss_group", _lib.PtgAl), ("ptg_rsample_group", _lib.PtgRs), ("ptg_rsample_backward_group", _lib.PtgRs)):
        arr = (T * 9)()
        for n in (0, 1, 8, 9, -1):
            assert getattr(L, name)(None, arr, n, None) == _lib.E_INVALID
        assert getattr(L, name)(None, None, 1, None) == _lib.E_INVALID
    for name, T in (("ptg_td_loss", _lib.PtgTd), ("ptg_actor_loss", _lib.PtgAl), ("ptg_rsample", _lib.PtgRs), ("ptg_rsample_backward", _lib.PtgRs)):
        assert getattr(L, name)(None, C.byref(T()), None) == _lib.E_INVALID and getattr(L, name)(None, None, None) == _lib.E_INVALID


# ------------------------------------------------------------------------------------------------- members on the host
def _td(B=6, K=2, dt=None, with_out=False, **over):
    """a SAC member of td_loss_group"""
    import torch
    dt = dt or torch.float32
    m = dict(q=[torch.zeros(B, dtype=dt) for _ in range(K)], next_q=[torch.zeros(B, dtype=dt) for _ in range(K)], rewards=torch.zeros(B), dones=torch.zeros(B),
             next_log_prob=torch.zeros(B, dtype=dt), ent_coef=0.2, gamma=0.9)
    if with_out:
        m["out"] = (torch.zeros(8, dtype=torch.float64), [torch.zeros(B, dtype=dt) for _ in range(K)], None)
    m.update(over)
    return m


def _dqn(B=6, A=5, **over):
    import torch
    m = dict(q=torch.zeros(B, A), next_q=torch.zeros(B, A), actions=torch.zeros(B, dtype=torch.int64), rewards=torch.zeros(B), dones=torch.zeros(B), gamma=0.9)
    m.update(over)
    return m


def _al(B=6, K=2, dt=None, with_out=False, **over):
    """a SAC member of actor_loss_group"""
    import torch
    dt = dt or torch.float32
    m = dict(q=[torch.zeros(B, dtype=dt) for _ in range(K)], log_prob=torch.zeros(B, dtype=dt), ent_coef=0.2)
    if with_out:
        m["out"] = (torch.zeros(8, dtype=torch.float64), [torch.zeros(B, dtype=dt) for _ in range(K)], torch.zeros(B, dtype=dt), None)
    m.update(over)
    return m


def _rs(B=6, dt=None, with_out=False, **over):
    import torch
    dt = dt or torch.float32
    ml = torch.zeros(B, 2, dtype=dt)
    m = dict(mean=ml[:, :1], log_std=ml[:, 1:], counter=torch.zeros(1, dtype=torch.int64))
    if with_out:
        m["out"] = (torch.zeros(B, 1, dtype=dt), torch.zeros(B, 1, dtype=dt), torch.zeros(B, 1, dtype=torch.float64))
    m.update(over)
    return m


def _bw(B=6, dt=None, with_out=False, **over):
    import torch
    dt = dt or torch.float32
    ml = torch.zeros(B, 2, dtype=dt)
    m = dict(mean=ml[:, :1], log_std=ml[:, 1:], noise=torch.zeros(B, 1, dtype=torch.float64), grad_actions=torch.zeros(B, 1, dtype=dt), grad_log_prob=None)
    if with_out:
        g = torch.zeros(B, 2, dtype=dt)
        m["out"] = (g[:, :1], g[:, 1:])
    m.update(over)
    return m


def _sm(B=6, **over):
    import torch
    m = dict(mean=torch.zeros(B, 1), counter=torch.zeros(1, dtype=torch.int64), noise_std=0.2, noise_clip=0.5)
    m.update(over)
    return m


def _refused(eng, who, call, cases):
    for k, (exc, text, args, kw) in enumerate(cases):
        with pytest.raises(exc, match=text) as e:
            call(*args, **kw)
        assert type(e.value) is exc and str(e.value).startswith(who + ": "), (who, k, str(e.value))
        assert eng._L is None, (who, k)


def test_td_loss_group_refusals_touch_nothing():
    import torch
    from helpers import host_engine
    eng = host_engine(4)
    t, v = TypeError, ValueError
    g3 = lambda **o: [_td(), _td(), _td(**o)]
    shared = _td(with_out=True)
    f64 = torch.float64
    sac = lambda ms, **kw: (("sac", ms), kw)
    cases = [
        (t, "members must be a list of dicts", *sac(_td())), (t, "members must be a list of dicts", *sac([_td(), 3])),
        (v, "1 to 8 members, got 0", *sac([])), (v, "1 to 8 members, got 9", *sac([_td() for _ in range(9)])),
        (t, "member 1: a member names td_loss's arguments; missing \\['dones'\\]", *sac([_td(), {k: x for k, x in _td().items() if k != "dones"}])),
        (t, "member 0: .*unknown \\['clip_range'\\]", *sac([_td(clip_range=0.2)])),
        (v, "gamma must have one entry per member, 2", *sac([_td(), _td()], gamma=[0.9, 0.9, 0.9])),
        (v, "member 0: kind must be", ("ddpg", [_td()]), {}),
        # a bad tensor in member 2, named as such, in the single op's words
        (t, "member 2: rewards must be of torch.float32 or torch.float64", *sac(g3(rewards=torch.zeros(6).long()))),
        (t, "member 2: next_q\\[1\\] must be of torch.float32", *sac(g3(next_q=[torch.zeros(6), torch.zeros(6, dtype=f64)]))),
        (v, "member 2: dones must be \\[6\\]", *sac(g3(dones=torch.zeros(7)))),
        (v, "member 2: next_log_prob lives on meta", *sac(g3(next_log_prob=torch.zeros(6, device="meta")))),
        (v, "member 2: kind 'sac' takes exactly one of ent_coef and log_ent_coef", *sac(g3(log_ent_coef=torch.zeros(1, dtype=f64)))),
        (v, "member 2: gamma must be finite", *sac(g3(gamma=float("inf")))),
        (v, "member 1: out.grad_q must be a list of 2 tensors", *sac([_td(), _td(out=(torch.zeros(8, dtype=f64), [torch.zeros(6)], None))])),
        (v, "member 1: want_target, but out.target is None", *sac([_td(), _td(with_out=True, want_target=True)])),
        # a TypeError of member 0 comes before a ValueError of member 1: member by member, each in check()'s fixed order
        (t, "member 0: rewards", *sac([_td(rewards=torch.zeros(6).long()), _td(dones=torch.zeros(7))])),
        # each field the members must agree in
        (v, "members 0 and 1 disagree in the batch: 6 and 7", *sac([_td(), _td(B=7)])),
        (v, "members 0 and 2 disagree in the number of critics: 2 and 1", *sac([_td(), _td(), _td(K=1)])),
        (v, "members 0 and 1 disagree in the dtype: torch.float32 and torch.float64", *sac([_td(), _td(dt=f64)])),
        (v, "members 0 and 1 disagree in the rewards' dtype", *sac([_td(), _td(rewards=torch.zeros(6, dtype=f64))])),
        (v, "members 0 and 1 disagree in the dones' dtype", *sac([_td(), _td(dones=torch.zeros(6, dtype=f64))])),
        (v, "members 0 and 1 disagree in log_ent_coef given or not", *sac([_td(), _td(ent_coef=None, log_ent_coef=torch.zeros(1, dtype=f64))])),
        (v, "members 0 and 1 disagree in the number of actions: 5 and 4", ("dqn", [_dqn(), _dqn(A=4)]), {}),
        (v, "members 0 and 1 disagree in the actions' dtype", ("dqn", [_dqn(), _dqn(actions=torch.zeros(6, dtype=torch.int32))]), {}),
        # shared outputs: one stats tensor, one gradient tensor, one workspace
        (v, "start at the same address", *sac([shared, _td(out=(shared["out"][0], [torch.zeros(6), torch.zeros(6)], None))])),
        (v, "start at the same address", *sac([shared, _td(out=(torch.zeros(8, dtype=f64), [torch.zeros(6), shared["out"][1][0]], None))])),
    ]
    _refused(eng, "td_loss_group", eng.td_loss_group, cases)
    from rl_ptg_amd import dqn_loss_group, sac_critic_loss_group
    for exc, text, fn in [(v, "gamma must have one entry per member, 2", lambda: sac_critic_loss_group(eng, [{k: x for k, x in _td().items() if k != "gamma"} for _ in range(2)], gamma=[0.1, 0.2, 0.3])),
                          (t, "member 0 names \\['gamma'\\]", lambda: dqn_loss_group(eng, [_dqn()], gamma=0.9)),
                          (t, "members must be a non-empty list", lambda: dqn_loss_group(eng, [], gamma=0.9)),
                          (t, "member 1 needs \\['rewards'\\]", lambda: sac_critic_loss_group(eng, [{k: x for k, x in _td().items() if k != "gamma"},
                                                                                                  {k: x for k, x in _td().items() if k not in ("gamma", "rewards")}], gamma=0.9))]:
        with pytest.raises(exc, match=text):
            fn()
        assert eng._L is None


def test_actor_loss_group_refusals_touch_nothing():
    import torch
    from helpers import host_engine
    eng = host_engine(4)
    t, v = TypeError, ValueError
    f64 = torch.float64
    g3 = lambda **o: [_al(), _al(), _al(**o)]
    shared = _al(with_out=True)
    la = lambda: torch.zeros(1, dtype=f64)
    sac = lambda ms, **kw: (("sac", ms), kw)
    cases = [
        (t, "members must be a list of dicts", *sac(_al())), (v, "1 to 8 members, got 0", *sac([])), (v, "1 to 8 members, got 9", *sac([_al() for _ in range(9)])),
        (t, "member 0: .*unknown \\['gamma'\\]", *sac([_al(gamma=0.9)])),
        (v, "member 0: kind must be", ("ppo", [_al()]), {}),
        (t, "member 2: log_prob must be of torch.float32", *sac(g3(log_prob=torch.zeros(6, dtype=f64)))),
        (v, "member 2: log_prob must be \\[6\\]", *sac(g3(log_prob=torch.zeros(7)))),
        (v, "member 2: kind 'sac' takes exactly one of ent_coef and log_ent_coef", *sac(g3(log_ent_coef=la()))),
        (v, "member 2: the entropy-coefficient loss needs log_ent_coef", *sac(g3(target_entropy=-1.0))),
        (v, "member 1: out.grad_q must be a list of 2 tensors", *sac([_al(), _al(out=(torch.zeros(8, dtype=f64), [torch.zeros(6)], torch.zeros(6), None))])),
        (t, "member 0: q\\[0\\]", *sac([_al(q=[torch.zeros(6).long(), torch.zeros(6)]), _al(log_prob=torch.zeros(7))])),
        (v, "members 0 and 1 disagree in the batch: 6 and 7", *sac([_al(), _al(B=7)])),
        (v, "members 0 and 2 disagree in the number of critics: 2 and 1", *sac([_al(), _al(), _al(K=1)])),
        (v, "members 0 and 1 disagree in the dtype", *sac([_al(), _al(dt=f64)])),
        (v, "members 0 and 1 disagree in log_ent_coef given or not", *sac([_al(), _al(ent_coef=None, log_ent_coef=la())])),
        (v, "members 0 and 1 disagree in target_entropy given or not", *sac([_al(ent_coef=None, log_ent_coef=la()), _al(ent_coef=None, log_ent_coef=la(), target_entropy=-1.0)])),
        (v, "members 0 and 1 disagree in the number of quantiles: 25 and 24",
         ("tqc", [dict(q=torch.zeros(6, 2, 25), log_prob=torch.zeros(6), ent_coef=0.2), dict(q=torch.zeros(6, 2, 24), log_prob=torch.zeros(6), ent_coef=0.2)]), {}),
        (v, "start at the same address", *sac([shared, _al(out=(shared["out"][0], [torch.zeros(6), torch.zeros(6)], torch.zeros(6), None))])),
        (v, "start at the same address", *sac([shared, _al(out=(torch.zeros(8, dtype=f64), [torch.zeros(6), torch.zeros(6)], shared["out"][2], None))])),
    ]
    _refused(eng, "actor_loss_group", eng.actor_loss_group, cases)


def test_rsample_group_refusals_touch_nothing():
    import torch
    from helpers import host_engine
    eng = host_engine(4)
    t, v = TypeError, ValueError
    f64 = torch.float64
    one = _rs(with_out=True)
    call = lambda ms, **kw: ((ms,), kw)
    cases = [
        (t, "members must be a list of dicts", *call(_rs())), (v, "1 to 8 members, got 0", *call([])), (v, "1 to 8 members, got 9", *call([_rs() for _ in range(9)])),
        (t, "member 1: a member names rsample's arguments; missing \\['counter'\\]", *call([_rs(), {k: x for k, x in _rs().items() if k != "counter"}])),
        (t, "member 2: log_std must be of torch.float32", *call([_rs(), _rs(), _rs(log_std=torch.zeros(6, 1, dtype=f64))])),
        (v, "member 2: a stochastic head needs a draw counter", *call([_rs(), _rs(), _rs(counter=None)])),
        (v, "member 1: out.noise must be", *call([_rs(), _rs(out=(torch.zeros(6, 1), torch.zeros(6, 1), torch.zeros(7, 1, dtype=f64)))])),
        (t, "member 0: mean", *call([_rs(mean=torch.zeros(6, 1).long()), _rs(counter=None)])),
        (v, "members 0 and 1 disagree in the batch: 6 and 7", *call([_rs(), _rs(B=7)])), (v, "members 0 and 1 disagree in the dtype", *call([_rs(), _rs(dt=f64)])),
        (v, "start at the same address", *call([one, _rs(out=(one["out"][0], torch.zeros(6, 1), torch.zeros(6, 1, dtype=f64)))])),
        (v, "start at the same address", *call([one, _rs(counter=one["counter"])])),          # the shared counter
    ]
    _refused(eng, "rsample_group", eng.rsample_group, cases)
    gone = _bw(with_out=True)
    cases = [
        (v, "1 to 8 members, got 0", *call([])), (v, "1 to 8 members, got 9", *call([_bw() for _ in range(9)])),
        (t, "member 2: noise must be of torch.float64", *call([_bw(), _bw(), _bw(noise=torch.zeros(6, 1))])),
        (v, "member 1: grad_actions and grad_log_prob are both None", *call([_bw(), _bw(grad_actions=None)])),
        (t, "member 0: noise", *call([_bw(noise=torch.zeros(6, 1)), _bw(grad_actions=None)])),
        (v, "members 0 and 1 disagree in the batch", *call([_bw(), _bw(B=7)])), (v, "members 0 and 1 disagree in the dtype", *call([_bw(), _bw(dt=f64)])),
        (v, "start at the same address", *call([gone, _bw(out=(gone["out"][1], torch.zeros(6, 1)))])),
    ]
    _refused(eng, "rsample_backward_group", eng.rsample_backward_group, cases)
    cases = [
        (v, "1 to 8 members, got 9", *call([_sm() for _ in range(9)])), (v, "member 1: noise_std must be finite", *call([_sm(), _sm(noise_std=-1.0)])),
        (v, "member 1: clip \\(1.0, -1.0\\) is not an interval", *call([_sm(), _sm(clip=(1.0, -1.0))])),
        (v, "noise_clip must have one entry per member, 2", *call([_sm(), _sm()], noise_clip=[0.5])),
        (v, "members 0 and 1 disagree in the batch", *call([_sm(), _sm(B=7)])), (v, "start at the same address", *call((lambda c: [_sm(counter=c), _sm(counter=c)])(torch.zeros(1, dtype=torch.int64)))),
    ]
    _refused(eng, "smooth_target_action_group", eng.smooth_target_action_group, cases)


# ------------------------------------------------------------------------------------------------- what reaches the library
def _one_call(eng, name):
    """the one call of the recording library that is no workspace-size query"""
    (n, args), = [c for c in eng._L.calls if not c[0].endswith("_workspace")]
    assert n == name and args[0] == "H" and args[-1] is None
    return args


def test_what_reaches_the_library_for_three_td_members():
    import torch
    from helpers import recording_engine
    from rl_ptg_amd import _lib
    eng = recording_engine(4)
    B, K = 6, 2
    wide = [[torch.zeros(B, K) for _ in range(3)] for _ in range(3)]          # per member: q, next_q, grad_q as the strided columns of [B][K]
    ws = [torch.zeros(64, dtype=torch.uint8) for _ in range(3)]
    alpha_dev = torch.zeros(1, dtype=torch.float64)
    cols = lambda w: [w[:, k] for k in range(K)]
    members = [_td(q=cols(wide[i][0]), next_q=cols(wide[i][1]), rewards=torch.zeros(B, dtype=torch.float64), gamma=0.9 + 0.01 * i, ent_coef=alpha_dev if i == 1 else 0.1 * (i + 1),
                   want_target=True, out=(torch.zeros(8, dtype=torch.float64), cols(wide[i][2]), torch.zeros(B)), workspace=ws[i]) for i in range(3)]
    res = eng.td_loss_group("sac", members)
    args = _one_call(eng, "ptg_td_loss_group")
    arr = args[1]
    assert isinstance(arr, C.Array) and len(arr) == 3 and args[2] == 3
    for i, (d, m) in enumerate(zip(arr, members)):
        assert (d.kind, d.flags, d.n_actions, d.n_critics, d.q_dtype, d.rew_dtype, d.done_dtype, d.act_kind, d.batch) == (
            _lib.TD_CRITICS, _lib.TD_ENTROPY, 0, K, _lib.OUT_F32, _lib.OUT_F64, _lib.OUT_F32, _lib.ACT_I32, B)
        for k in range(K):
            assert (d.q_dev[k], d.q_s_n[k], d.next_q_dev[k], d.next_s_n[k], d.grad_q_dev[k], d.g_s_n[k]) == (
                wide[i][0].data_ptr() + 4 * k, K, wide[i][1].data_ptr() + 4 * k, K, wide[i][2].data_ptr() + 4 * k, K)
        assert (d.act_dev, d.rew_dev, d.done_dev, d.next_logp_dev) == (None, m["rewards"].data_ptr(), m["dones"].data_ptr(), m["next_log_prob"].data_ptr())
        assert (d.alpha_dev, d.alpha) == ((alpha_dev.data_ptr(), 0.0) if i == 1 else (None, 0.1 * (i + 1)))
        assert (d.gamma, d.scale) == (0.9 + 0.01 * i, 0.5)
        assert (d.stats_dev, d.y_dev, d.ws_dev) == (m["out"][0].data_ptr(), m["out"][2].data_ptr(), ws[i].data_ptr())
        assert res[i].stats is m["out"][0] and res[i].target is m["out"][2]
    # a group of one hands the library the bytes the single call hands it
    eng1, eng2 = recording_engine(4), recording_engine(4)
    eng1.td_loss_group("sac", members[1:2])
    single = dict(members[1])
    eng2.td_loss("sac", single.pop("q"), single.pop("next_q"), single.pop("rewards"), single.pop("dones"), single.pop("gamma"), **single)
    assert bytes(_one_call(eng1, "ptg_td_loss_group")[1][0]) == bytes(_one_call(eng2, "ptg_td_loss")[1]._obj) == bytes(arr[1])
    # DQN members, the scalars as one list
    eng3 = recording_engine(4)
    eng3.td_loss_group("dqn", [{k: x for k, x in _dqn().items() if k != "gamma"} for _ in range(2)], gamma=[0.9, 0.8])
    arr = _one_call(eng3, "ptg_td_loss_group")[1]
    assert [(d.kind, d.n_actions, d.act_kind, d.gamma, d.scale, d.q_s_n[0]) for d in arr] == [(_lib.TD_DQN, 5, _lib.ACT_I64, 0.9, 1.0, 5), (_lib.TD_DQN, 5, _lib.ACT_I64, 0.8, 1.0, 5)]


def test_what_reaches_the_library_for_three_actor_loss_members():
    import torch
    from helpers import recording_engine
    from rl_ptg_amd import _lib
    eng = recording_engine(4)
    B, K = 6, 2
    la = [torch.zeros(1, dtype=torch.float64) for _ in range(3)]
    ws = [torch.zeros(64, dtype=torch.uint8) for _ in range(3)]
    members = [_al(ent_coef=None, log_ent_coef=la[i], target_entropy=-1.0 - i, out=(torch.zeros(8, dtype=torch.float64), [torch.zeros(B), torch.zeros(B)], torch.zeros(B),
                                                                                     torch.zeros(1, dtype=torch.float64)), workspace=ws[i]) for i in range(3)]
    res = eng.actor_loss_group("sac", members)
    arr = _one_call(eng, "ptg_actor_loss_group")[1]
    assert isinstance(arr, C.Array) and len(arr) == 3
    for i, (d, m) in enumerate(zip(arr, members)):
        assert (d.kind, d.flags, d.n_critics, d.n_quantiles, d.q_dtype, d.batch) == (_lib.AL_MIN, _lib.AL_ENTROPY | _lib.AL_LOG_ALPHA | _lib.AL_ENT_COEF, K, 1, _lib.OUT_F32, B)
        assert [(d.q_dev[k], d.q_s_n[k], d.grad_q_dev[k], d.g_s_n[k]) for k in range(K)] == [(m["q"][k].data_ptr(), 1, m["out"][1][k].data_ptr(), 1) for k in range(K)]
        assert (d.logp_dev, d.alpha_dev, d.alpha, d.target_entropy) == (m["log_prob"].data_ptr(), la[i].data_ptr(), 0.0, -1.0 - i)
        assert (d.stats_dev, d.grad_logp_dev, d.grad_log_alpha_dev, d.ws_dev) == (m["out"][0].data_ptr(), m["out"][2].data_ptr(), m["out"][3].data_ptr(), ws[i].data_ptr())
        assert res[i].grad_log_ent_coef is m["out"][3]
    eng1, eng2 = recording_engine(4), recording_engine(4)
    eng1.actor_loss_group("sac", members[2:])
    eng2.actor_loss("sac", **members[2])
    assert bytes(_one_call(eng1, "ptg_actor_loss_group")[1][0]) == bytes(_one_call(eng2, "ptg_actor_loss")[1]._obj) == bytes(arr[2])
    # the other kinds, the scalars as lists
    eng3 = recording_engine(4)
    eng3.actor_loss_group("ent_coef", [dict(log_prob=torch.zeros(B), log_ent_coef=la[i]) for i in range(2)], target_entropy=[-1.0, -2.0])
    eng3.actor_loss_group("td3", [dict(q=torch.zeros(B, 1)) for _ in range(2)])
    eng3.actor_loss_group("tqc", [dict(q=torch.zeros(B, 2, 25), log_prob=torch.zeros(B)) for _ in range(2)], ent_coef=[0.1, 0.2])
    a, b, c = [args[1] for n, args in eng3._L.calls if n == "ptg_actor_loss_group"]
    assert [(d.kind, d.flags, d.n_critics, d.target_entropy) for d in a] == [(_lib.AL_ALPHA_ONLY, _lib.AL_LOG_ALPHA | _lib.AL_ENT_COEF, 0, -1.0), (_lib.AL_ALPHA_ONLY, 6, 0, -2.0)]
    assert [(d.kind, d.flags, d.n_critics, d.n_quantiles) for d in b] == [(_lib.AL_MEAN, 0, 1, 1)] * 2
    assert [(d.kind, d.flags, d.n_critics, d.n_quantiles, d.alpha, d.q_s_n[1]) for d in c] == [(_lib.AL_MEAN, _lib.AL_ENTROPY, 2, 25, 0.1, 50), (_lib.AL_MEAN, _lib.AL_ENTROPY, 2, 25, 0.2, 50)]


def test_what_reaches_the_library_for_three_rsample_members_forward_backward_and_smoothing():
    import torch
    from helpers import recording_engine
    from rl_ptg_amd import _lib
    eng = recording_engine(4)
    B = 6
    members = [_rs(with_out=True, seed=2 ** 64 - 1 - i) for i in range(3)]
    res = eng.rsample_group(members)
    arr = _one_call(eng, "ptg_rsample_group")[1]
    assert isinstance(arr, C.Array) and len(arr) == 3
    for i, (d, m) in enumerate(zip(arr, members)):
        assert (d.kind, d.flags, d.q_dtype, d.batch) == (_lib.RS_SQUASH, 0, _lib.OUT_F32, B)
        assert (d.mean_dev, d.mean_s_n, d.log_std_dev, d.log_std_s_n) == (m["mean"].data_ptr(), 2, m["mean"].data_ptr() + 4, 2)
        assert (d.seed, d.counter_dev) == (2 ** 64 - 1 - i, m["counter"].data_ptr())
        assert (d.act_dev, d.logp_dev, d.noise_dev) == tuple(t.data_ptr() for t in m["out"])
        assert res[i].noise is m["out"][2]
    eng1, eng2 = recording_engine(4), recording_engine(4)
    eng1.rsample_group(members[:1])
    eng2.rsample(**members[0])
    assert bytes(_one_call(eng1, "ptg_rsample_group")[1][0]) == bytes(_one_call(eng2, "ptg_rsample")[1]._obj) == bytes(arr[0])
    det = recording_engine(4)
    det.rsample_group([_rs(counter=None), _rs(counter=None)], seed=[3, 4], deterministic=True)
    assert [(d.flags, d.seed, d.counter_dev) for d in _one_call(det, "ptg_rsample_group")[1]] == [(_lib.RS_DETERMINISTIC, 3, None), (_lib.RS_DETERMINISTIC, 4, None)]
    # the backward: grad_actions alone in member 0, grad_log_prob alone in member 1, both in member 2
    eng = recording_engine(4)
    gl = torch.zeros(B, 1)
    members = [_bw(with_out=True), _bw(with_out=True, grad_actions=None, grad_log_prob=gl), _bw(with_out=True, grad_log_prob=gl)]
    res = eng.rsample_backward_group(members)
    arr = _one_call(eng, "ptg_rsample_backward_group")[1]
    for i, (d, m) in enumerate(zip(arr, members)):
        assert (d.kind, d.flags, d.batch, d.noise_dev) == (_lib.RS_SQUASH, 0, B, m["noise"].data_ptr())
        assert (d.grad_act_dev, d.grad_logp_dev) == (None if m["grad_actions"] is None else m["grad_actions"].data_ptr(), None if m["grad_log_prob"] is None else gl.data_ptr())
        assert (d.grad_mean_dev, d.gm_s_n, d.grad_log_std_dev, d.gl_s_n) == (m["out"][0].data_ptr(), 2, m["out"][0].data_ptr() + 4, 2)
        assert res[i].grad_mean is m["out"][0]
    eng1, eng2 = recording_engine(4), recording_engine(4)
    eng1.rsample_backward_group(members[1:2])
    eng2.rsample_backward(**members[1])
    assert bytes(_one_call(eng1, "ptg_rsample_backward_group")[1][0]) == bytes(_one_call(eng2, "ptg_rsample_backward")[1]._obj) == bytes(arr[1])
    # the smoothing goes through ptg_rsample_group too
    eng = recording_engine(4)
    outs = [torch.zeros(B, 1) for _ in range(3)]
    members = [dict(mean=torch.zeros(B, 1), counter=torch.zeros(1, dtype=torch.int64), clip=(-1.0 + 0.1 * i, 1.0), out=outs[i]) for i in range(3)]
    res = eng.smooth_target_action_group(members, noise_std=[0.1, 0.2, 0.3], noise_clip=0.5, seed=[7, 8, 9])
    arr = _one_call(eng, "ptg_rsample_group")[1]
    assert [(d.kind, d.noise_std, d.noise_clip, d.clip_lo, d.clip_hi, d.seed, d.act_dev, d.logp_dev) for d in arr] == [
        (_lib.RS_SMOOTH, [0.1, 0.2, 0.3][i], 0.5, -1.0 + 0.1 * i, 1.0, 7 + i, outs[i].data_ptr(), None) for i in range(3)]
    assert all(r is o for r, o in zip(res, outs))
    eng1, eng2 = recording_engine(4), recording_engine(4)
    eng1.smooth_target_action_group(members[:1], noise_std=0.1, noise_clip=0.5, seed=7)
    eng2.smooth_target_action(members[0]["mean"], members[0]["counter"], 0.1, 0.5, clip=members[0]["clip"], seed=7, out=outs[0])
    assert bytes(_one_call(eng1, "ptg_rsample_group")[1][0]) == bytes(_one_call(eng2, "ptg_rsample")[1]._obj) == bytes(arr[0])


def test_the_autograd_front_ends_make_one_grouped_library_call_each():
    import torch
    from helpers import recording_engine
    from rl_ptg_amd import (dqn_loss_group, ent_coef_loss_group, sac_actor_loss_group, sac_critic_loss_group, squashed_rsample_group, td3_actor_loss_group,
                            td3_critic_loss_group, tqc_actor_loss_group)
    eng = recording_engine(4)
    B, G = 6, 3
    req = lambda *s: torch.zeros(*s, requires_grad=True)
    names = lambda: [n for n, _ in eng._L.calls if not n.endswith("_workspace")]
    q = [[req(B), req(B)] for _ in range(G)]
    strip = lambda m, *ks: {k: x for k, x in m.items() if k not in ks}
    losses, stats = sac_critic_loss_group(eng, [strip(_td(q=q[i]), "gamma", "ent_coef") for i in range(G)], gamma=[0.9, 0.8, 0.7], ent_coef=0.2)
    assert len(losses) == len(stats) == G and all(x.requires_grad and x.dim() == 0 for x in losses)
    torch.autograd.backward(losses[:2])                      # member 2 is left out: its Q tensors keep no gradient
    assert all(t.grad is not None and t.grad.shape == (B,) for t in q[0] + q[1]) and all(t.grad is None for t in q[2])
    td3_critic_loss_group(eng, [strip(_td(), "gamma", "ent_coef", "next_log_prob") for _ in range(G)], gamma=0.9)
    dqn_loss_group(eng, [strip(_dqn(q=req(B, 5)), "gamma") for _ in range(G)], gamma=0.9)
    assert names() == ["ptg_td_loss_group"] * 3
    eng._L.calls.clear()
    ml = [req(B, 2) for _ in range(G)]
    pairs = squashed_rsample_group(eng, [dict(mean=x[:, :1], log_std=x[:, 1:], counter=torch.zeros(1, dtype=torch.int64)) for x in ml], seed=[1, 2, 3])
    assert len(pairs) == G and all(a.shape == (B, 1) and lp.shape == (B, 1) and a.requires_grad for a, lp in pairs)
    torch.autograd.backward([pairs[0][0].sum(), pairs[2][1].sum()])      # member 0 through its actions, member 2 through its log-probs, member 1 not at all
    assert names() == ["ptg_rsample_group", "ptg_rsample_backward_group"]
    bw = eng._L.calls[-1][1]
    assert bw[2] == 2 and [(d.grad_act_dev is not None, d.grad_logp_dev is not None) for d in bw[1]] == [(True, False), (False, True)]
    assert ml[0].grad is not None and ml[2].grad is not None and ml[1].grad is None
    eng._L.calls.clear()
    la = [torch.zeros(1, dtype=torch.float64, requires_grad=True) for _ in range(G)]
    els, el_stats = ent_coef_loss_group(eng, [dict(log_prob=torch.zeros(B), log_ent_coef=la[i]) for i in range(G)], target_entropy=[-1.0, -2.0, -3.0])
    torch.autograd.backward(els)
    assert all(x.grad is not None and x.grad.shape == (1,) for x in la) and all(e.dtype == torch.float64 for e in els)
    qa, lp = [[req(B), req(B)] for _ in range(G)], [req(B) for _ in range(G)]
    al, _ = sac_actor_loss_group(eng, [dict(q=qa[i], log_prob=lp[i], ent_coef=el_stats[i][4:5]) for i in range(G)])
    torch.autograd.backward(al)
    assert all(t.grad is not None for ts in qa for t in ts) and all(t.grad is not None for t in lp)
    tqc_actor_loss_group(eng, [dict(quantiles=req(B, 2, 25), log_prob=req(B)) for _ in range(G)], ent_coef=[0.1, 0.2, 0.3])
    q1 = [req(B, 1) for _ in range(G)]
    tl, _ = td3_actor_loss_group(eng, [dict(q1=x) for x in q1])
    torch.autograd.backward(tl)
    assert all(x.grad is not None and x.grad.shape == (B, 1) for x in q1)
    assert names() == ["ptg_actor_loss_group"] * 4
