"""ptg_policy_loss_group / ptg_optim_step_group without a device: the header's declarations and the exported symbols, what the library
refuses on a NULL handle, every Python-level refusal of HipEngine.policy_loss_group / optim_step_group (the single op's words behind
"member i:", nothing touched), the descriptor arrays an accepted three-member call hands the library, a group of one against the single
op (the same descriptor bytes), and DeviceOptimizerGroup's refusals.  The arithmetic has no test here: a grouped call is defined as the
single calls, which tests/test_train_group.py compares bit for bit on the device."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- the ABI, without a device
def test_the_header_declares_both_entries_and_the_library_exports_them():
    from rl_ptg_amd import _lib
    _lib.build()
    L = _lib.lib()
    assert all(hasattr(L, n) and n in _lib.EXPORTS for n in ("ptg_policy_loss_group", "ptg_optim_step_group"))
    assert L.ptg_abi_version() == 13
    hdr = open(os.path.join(ROOT, "include", "ptg_env.h")).read()
    assert "#define PTG_ABI_VERSION 13" in hdr and "#define PTG_TRAIN_GROUP_MAX 8" in hdr and _lib.TRAIN_GROUP_MAX == 8
    assert "int ptg_policy_loss_group(ptg_env* env, const ptg_loss* members, int32_t n_members, void* stream);" in hdr
    assert "int ptg_optim_step_group(ptg_env* env, const ptg_optim* members, int32_t n_members, void* stream);" in hdr
    # eight members by value in the launch arguments: the header states the sizes; the descriptors themselves are no larger than the limit either
    assert "8 x 208 = 1 664 bytes" in hdr and "8 x 136 = 1 088 bytes" in hdr
    assert 8 * C.sizeof(_lib.PtgLoss) <= 4096 and 8 * C.sizeof(_lib.PtgOptim) <= 4096


def test_a_null_handle_without_a_device():
    """no handle exists without a device: array and counts are refused with a handle in tests/test_train_group.py"""
    from rl_ptg_amd import _lib
    L = _lib.lib()
    lo, op = (_lib.PtgLoss * 9)(), (_lib.PtgOptim * 9)()
    for n in (0, 1, 8, 9, -1):
        assert L.ptg_policy_loss_group(None, lo, n, None) == _lib.E_INVALID
        assert L.ptg_optim_step_group(None, op, n, None) == _lib.E_INVALID
    assert L.ptg_policy_loss_group(None, None, 1, None) == _lib.E_INVALID and L.ptg_optim_step_group(None, None, 1, None) == _lib.E_INVALID


# ------------------------------------------------------------------------------------------------- the loss: Python refusals
def _member(B=6, A=5, dt=None, with_out=False, **over):
    import torch
    dt = dt or torch.float32
    m = dict(head_input=torch.zeros(B, A, dtype=dt), values=torch.zeros(B, dtype=dt), actions=torch.zeros(B, dtype=torch.int64),
             old_log_prob=torch.zeros(B, dtype=dt), advantages=torch.zeros(B, dtype=dt), returns=torch.zeros(B, dtype=dt))
    if with_out:
        m["out"] = (torch.zeros(8, dtype=torch.float64), torch.zeros(B, A, dtype=dt), torch.zeros(B, dtype=dt), None)
    m.update(over)
    return m


def test_policy_loss_group_refusals_touch_nothing():
    import torch
    from helpers import host_engine
    eng = host_engine(4)
    t, v = TypeError, ValueError
    M = lambda *ms: list(ms)
    g3 = lambda **over2: M(_member(), _member(), _member(**over2))
    shared = _member(with_out=True)
    cases = [
        # the container and the member count: 0 and 9
        (t, "members must be a list of dicts", dict(members=_member())), (t, "members must be a list of dicts", dict(members=[_member(), 3])),
        (v, "1 to 8 members, got 0", dict(members=[])), (v, "1 to 8 members, got 9", dict(members=[_member() for _ in range(9)])),
        (t, "member 1: a member names policy_loss's arguments; missing \\['returns'\\]", dict(members=M(_member(), {k: x for k, x in _member().items() if k != "returns"}))),
        (t, "member 0: .*unknown \\['gamma'\\]", dict(members=M(_member(gamma=0.9)))),
        (v, "kind must be", dict(kind="trpo", members=M(_member()))),
        # a bad tensor in member 2, named as such, in the single op's words
        (t, "member 2: values must be of torch.float32", dict(members=g3(values=torch.zeros(6, dtype=torch.float64)))),
        (t, "member 2: actions must be of torch.int32 or torch.int64", dict(members=g3(actions=torch.zeros(6)))),
        (v, "member 2: advantages must be \\[6\\]", dict(members=g3(advantages=torch.zeros(7)))),
        (v, "member 2: head_input .* needs unit column stride", dict(members=g3(head_input=torch.zeros(5, 6).t()))),
        (v, "member 2: returns lives on meta", dict(members=g3(returns=torch.zeros(6, device="meta")))),
        (v, "member 2: PPO needs a clip_range", dict(members=g3(clip_range=-0.1))),
        (v, "member 2: clip_range_vf needs old_values", dict(members=g3(clip_range_vf=0.2))),
        (v, "member 1: out.grad_values must be", dict(members=M(_member(), _member(out=(torch.zeros(8, dtype=torch.float64), torch.zeros(6, 5), torch.zeros(7), None))))),
        # a TypeError of member 0 comes before a ValueError of member 1: member by member, each in check()'s fixed order
        (t, "member 0: head_input", dict(members=M(_member(head_input=torch.zeros(6, 5).long()), _member(advantages=torch.zeros(7))))),
        # each field the members must agree in
        (v, "members 0 and 1 disagree in the batch: 6 and 7", dict(members=M(_member(), _member(B=7)))),
        (v, "members 0 and 2 disagree in the number of actions: 5 and 2", dict(members=M(_member(), _member(), _member(A=2)))),
        (v, "members 0 and 1 disagree in the dtype: torch.float32 and torch.float64", dict(members=M(_member(), _member(dt=torch.float64)))),
        (v, "members 0 and 1 disagree in the actions' dtype", dict(members=M(_member(), _member(actions=torch.zeros(6, dtype=torch.int32))))),
        (v, "members 0 and 1 disagree in normalize_advantage: True and False", dict(members=M(_member(), _member(normalize_advantage=False)))),
        (v, "members 0 and 1 disagree in clip_range_vf given or not", dict(members=M(_member(), _member(clip_range_vf=0.2, old_values=torch.zeros(6))))),
        (v, "members 0 and 1 disagree in the head: categorical and gaussian",
         dict(members=M(_member(), _member(head_input=torch.zeros(6), actions=torch.zeros(6), log_std=torch.zeros(1))))),
        # shared outputs: one stats tensor, one gradient tensor
        (v, "start at the same address", dict(members=M(shared, _member(out=(shared["out"][0], torch.zeros(6, 5), torch.zeros(6), None))))),
        (v, "start at the same address", dict(members=M(shared, _member(out=(torch.zeros(8, dtype=torch.float64), shared["out"][1], torch.zeros(6), None))))),
    ]
    for k, (exc, text, kw) in enumerate(cases):
        kw = dict(dict(kind="ppo", clip_range=0.2), **kw)
        with pytest.raises(exc, match=text) as e:
            eng.policy_loss_group(kw.pop("kind"), kw.pop("members"), **kw)
        assert type(e.value) is exc and str(e.value).startswith("policy_loss_group: "), (k, str(e.value))
        assert eng._L is None, k
    # the autograd wrappers: the scalars' lists
    from rl_ptg_amd import a2c_loss_group, ppo_loss_group
    for exc, text, fn in [(v, "clip_range must have one entry per member, 2", lambda: ppo_loss_group(eng, [_member(), _member()], clip_range=[0.1, 0.2, 0.3])),
                          (t, "member 0 names \\['clip_range'\\]", lambda: ppo_loss_group(eng, [_member(clip_range=0.1)], clip_range=0.2)),
                          (t, "members must be a non-empty list", lambda: a2c_loss_group(eng, [])),
                          (t, "member 1 needs the tensors \\['values'\\]", lambda: a2c_loss_group(eng, [_member(), _member(values=None)]))]:
        with pytest.raises(exc, match=text):
            fn()
        assert eng._L is None


def test_what_reaches_the_library_for_three_loss_members():
    """the descriptor array: three members in order, each member's own pointers, strides and scalars; the fields the launches share
    equal; nothing allocated when out= and workspace= are given (the recording library sees one size query per member and the call)"""
    import torch
    from helpers import recording_engine
    from rl_ptg_amd import _lib
    eng = recording_engine(4)
    B, A = 6, 5
    ac = [torch.zeros(B, A + 1) for _ in range(3)]                       # strided [B][A + 1] actor-critic outputs
    gr = [torch.zeros(B, A + 1) for _ in range(3)]
    ws = [torch.zeros(120, dtype=torch.uint8) for _ in range(3)]
    members = [_member(head_input=ac[i][:, :A], values=ac[i][:, A], old_values=torch.zeros(B), clip_range=0.1 * (i + 1), clip_range_vf=0.5 + i, ent_coef=0.01 * i,
                       vf_coef=0.25 * (i + 1), out=(torch.zeros(8, dtype=torch.float64), gr[i][:, :A], gr[i][:, A], None), workspace=ws[i]) for i in range(3)]
    res = eng.policy_loss_group("ppo", members)
    sizes = [c for c in eng._L.calls if c[0] == "ptg_policy_loss_workspace"]
    (name, args), = [c for c in eng._L.calls if c[0] != "ptg_policy_loss_workspace"]
    assert name == "ptg_policy_loss_group" and args[0] == "H" and args[2] == 3 and args[3] is None and all(a == (B,) for _, a in sizes)
    arr = args[1]
    assert isinstance(arr, C.Array) and len(arr) == 3
    for i, (d, m) in enumerate(zip(arr, members)):
        assert (d.kind, d.head, d.flags, d.n_actions, d.in_dtype, d.act_kind, d.batch) == (_lib.LOSS_PPO, _lib.HEAD_CATEGORICAL, _lib.LOSS_NORM_ADV | _lib.LOSS_CLIP_VF,
                                                                                          A, _lib.OUT_F32, _lib.ACT_I64, B)
        assert (d.in_dev, d.in_s_n, d.val_dev, d.val_s_n) == (ac[i].data_ptr(), A + 1, ac[i].data_ptr() + 4 * A, A + 1)
        assert (d.act_dev, d.old_logp_dev, d.adv_dev, d.ret_dev, d.old_val_dev, d.log_std_dev) == (
            m["actions"].data_ptr(), m["old_log_prob"].data_ptr(), m["advantages"].data_ptr(), m["returns"].data_ptr(), m["old_values"].data_ptr(), None)
        assert (d.clip_range, d.clip_range_vf, d.ent_coef, d.vf_coef) == (0.1 * (i + 1), 0.5 + i, 0.01 * i, 0.25 * (i + 1))
        assert (d.stats_dev, d.grad_in_dev, d.g_s_n, d.grad_val_dev, d.gv_s_n, d.grad_log_std_dev, d.ws_dev) == (
            m["out"][0].data_ptr(), gr[i].data_ptr(), A + 1, gr[i].data_ptr() + 4 * A, A + 1, None, ws[i].data_ptr())
        assert res[i].stats is m["out"][0] and res[i].grad_log_std is None
    # a group of one hands the library the bytes the single call hands it
    eng1, eng2 = recording_engine(4), recording_engine(4)
    eng1.policy_loss_group("ppo", members[:1])
    eng2.policy_loss("ppo", **members[0])
    d1 = [a for n, a in eng1._L.calls if n == "ptg_policy_loss_group"][0][1][0]
    d2 = [a for n, a in eng2._L.calls if n == "ptg_policy_loss"][0][1]._obj
    assert bytes(d1) == bytes(d2)


# ------------------------------------------------------------------------------------------------- the optimiser
def _plans(eng, kinds=("adam", "adam", "adam"), dt=None, targets=False, n=(5, 1024, 1025)):
    import torch
    dt = dt or torch.float32
    mk = lambda: [torch.zeros(k, dtype=dt) for k in n]
    return [eng.optim_plan(mk(), mk(), kind, targets=mk() if targets else None) for kind in kinds]


def _recording_optim_engine():
    from helpers import CpuTorch, host_engine
    from test_optim_host import _Lib
    return host_engine(4, _h="H", _L=_Lib(), _torch=CpuTorch(), _stream=lambda: None)


def test_optim_step_group_refusals_touch_the_library_with_no_step():
    import torch
    rec = _recording_optim_engine()
    plans = _plans(rec)
    t, v = TypeError, ValueError
    lr64 = torch.zeros(1, dtype=torch.float64)
    cases = [
        (t, "plans must be a list", dict(plans=plans[0])),
        (v, "1 to 8 members, got 0", dict(plans=[])), (v, "1 to 8 members, got 9", dict(plans=_plans(rec, ("adam",) * 9))),
        (t, "member 2: plan must be an OptimPlan", dict(plans=plans[:2] + ["plan"])),
        (v, "lrs must have one entry per member, 3", dict(lrs=[1e-3, 1e-3])), (v, "eps must have one entry per member", dict(eps=[1e-8] * 4)),
        (t, "member 2: a tensor lr must be of torch.float64", dict(lrs=[1e-3, lr64, torch.zeros(1)])),
        (v, "member 1: lr must be finite", dict(lrs=[1e-3, -1.0, 1e-3])),
        (v, "member 2: betas must be in", dict(betas=[(0.9, 0.999), (0.9, 0.999), (1.0, 0.999)])),
        (v, "member 0: eps must be", dict(eps=[-1.0, 1e-8, 1e-8])),
        (v, "member 1: max_grad_norm must be", dict(max_grad_norm=[0.5, -0.5, 0.5])),
        (v, "member 0: tau given, but the plan has no targets", dict(tau=0.5)),
        (v, "member 1: a 'polyak' plan", dict(plans=[plans[0], rec.polyak_update([torch.zeros(3)], [torch.zeros(3)], 1.0), plans[2]])),
        # what the members must agree in
        (v, "members 0 and 1 disagree in the plan's kind: adam and rmsprop", dict(plans=_plans(rec, ("adam", "rmsprop")))),
        (v, "members 0 and 2 disagree in the dtype", dict(plans=plans[:2] + _plans(rec, ("adam",), dt=torch.float64))),
        (v, "members 0 and 1 disagree in clipping", dict(plans=plans[:2], max_grad_norm=[0.5, None])),
        (v, "members 0 and 1 disagree in having targets", dict(plans=[plans[0]] + _plans(rec, ("adam",), targets=True), tau=[None, 0.5])),
        # one plan twice: shared state, norm and scratch
        (v, "a plan is given twice", dict(plans=[plans[0], plans[1], plans[0]])),
    ]
    before = len(rec._L.calls)
    for k, (exc, text, kw) in enumerate(cases):
        kw = dict(dict(plans=plans, lrs=1e-3), **kw)
        with pytest.raises(exc, match=text) as e:
            rec.optim_step_group(kw.pop("plans"), kw.pop("lrs"), **kw)
        assert type(e.value) is exc and str(e.value).startswith("optim_step_group: "), (k, str(e.value))
    assert [n for n, _ in rec._L.calls[before:] if n != "ptg_optim_step"] == []      # the one Polyak call of the cases' setup aside, nothing reached the library
    assert not any(n == "ptg_optim_step_group" for n, _ in rec._L.calls)
    # two plans over one state (a rebuilt plan takes its predecessor's state over): the state pointer is shared
    twin = rec.optim_plan(plans[0].params, plans[0].grads, "adam", state=plans[0])
    with pytest.raises(ValueError, match="start at the same address"):
        rec.optim_step_group([plans[0], twin], 1e-3)


def test_what_reaches_the_library_for_three_optimiser_members():
    import torch
    from rl_ptg_amd import _lib
    eng = _recording_optim_engine()
    plans = [_plans(eng, ("adam",), n=n, targets=True)[0] for n in ((5,), (1024, 1025), (2049, 1, 3, 1023))]
    assert [p.n_chunks for p in plans] == [1, 3, 6]
    lr_dev = torch.zeros(1, dtype=torch.float64)
    eng.optim_step_group(plans, [3e-4, lr_dev, 1e-3], betas=[(0.9, 0.999), (0.8, 0.95), (0.7, 0.9)], eps=[1e-8, 1e-5, 1e-6], max_grad_norm=[0.5, 1e6, 10.0],
                         tau=[0.005, 0.01, 1.0], zero_grad=True)
    (name, args), = eng._L.calls
    assert name == "ptg_optim_step_group" and args[0] == "H" and args[2] == 3 and args[3] is None
    arr = args[1]
    assert isinstance(arr, C.Array) and len(arr) == 3
    for i, (d, p) in enumerate(zip(arr, plans)):
        assert (d.kind, d.flags, d.dtype) == (_lib.OPTIM_ADAM, _lib.OPTIM_CLIP | _lib.OPTIM_TARGETS | _lib.OPTIM_ZERO_GRAD, _lib.OUT_F32)
        assert (d.n_tensors, d.n_chunks) == (len(p.params), p.n_chunks)
        assert (d.tensors_dev, d.chunks_dev, d.state_dev, d.norm_dev, d.ws_dev) == (p.tensors_dev.data_ptr(), p.chunks_dev.data_ptr(), p.state.data_ptr(),
                                                                                   p.norm.data_ptr(), p.workspace.data_ptr())
    assert [(d.lr_dev, d.lr) for d in arr] == [(None, 3e-4), (lr_dev.data_ptr(), 0.0), (None, 1e-3)]
    assert [(d.beta1, d.beta2, d.eps, d.max_norm, d.tau) for d in arr] == [(0.9, 0.999, 1e-8, 0.5, 0.005), (0.8, 0.95, 1e-5, 1e6, 0.01), (0.7, 0.9, 1e-6, 10.0, 1.0)]
    # a group of one hands the library the bytes the single call hands it
    eng.optim_step_group(plans[1:2], lr_dev, betas=(0.8, 0.95), eps=1e-5, max_grad_norm=1e6, tau=0.01, zero_grad=True)
    eng.optim_step(plans[1], lr_dev, betas=(0.8, 0.95), eps=1e-5, max_grad_norm=1e6, tau=0.01, zero_grad=True)
    assert bytes(eng._L.calls[1][1][1][0]) == bytes(eng._L.calls[2][1][1]._obj) == bytes(arr[1])


def test_device_optimizer_group_refusals_and_its_one_call():
    import torch
    from rl_ptg_amd import DeviceOptimizer, DeviceOptimizerGroup
    eng = _recording_optim_engine()
    P = lambda dt=torch.float32: [torch.zeros(3, 4, dtype=dt, requires_grad=True), torch.zeros(1030, dtype=dt, requires_grad=True)]
    adam = lambda **kw: DeviceOptimizer(eng, P(kw.pop("dt", torch.float32)), **dict(dict(kind="adam", lr=1e-3, max_grad_norm=0.5, zero_grad=True), **kw))
    a = adam()
    for exc, text, opts in [
            (ValueError, "an empty list", []), (ValueError, "1 to 8 optimizers, got 9", [adam() for _ in range(9)]),
            (TypeError, r"optimizers\[1\] must be a DeviceOptimizer", [adam(), torch.optim.SGD(P(), lr=0.1)]),
            (ValueError, "optimizers 0 and 1 disagree in kind: adam and rmsprop", [adam(), adam(kind="rmsprop")]),
            (ValueError, "optimizers 0 and 2 disagree in clipping", [adam(), adam(), adam(max_grad_norm=None)]),
            (ValueError, "optimizers 0 and 1 disagree in zero_grad", [adam(), adam(zero_grad=False)]),
            (ValueError, "optimizers 0 and 1 disagree in having targets", [adam(), adam(targets=P(), tau=0.5)]),
            (ValueError, "optimizers 0 and 1 disagree in the parameters' dtype", [adam(), adam(dt=torch.float64)]),
            (ValueError, "given twice", [a, a])]:
        with pytest.raises(exc, match=text):
            DeviceOptimizerGroup(eng, opts)
    assert eng._L.calls == []
    opts = [adam(lr=1e-3 * (i + 1), eps=1e-5 * (i + 1), max_grad_norm=0.5 + i) for i in range(3)]
    grp = DeviceOptimizerGroup(eng, opts)
    assert grp.grad_norms == [None, None, None]
    with pytest.raises(ValueError, match="parameter 0 has no gradient"):
        grp.step()
    for o in opts:
        for p in o.params:
            p.grad = torch.ones_like(p)
    grp.step()
    grp.step()                                               # nothing moved: the same plans
    assert [n for n, _ in eng._L.calls] == ["ptg_optim_step_group"] * 2 and eng._L.calls[0][1][2] == 3
    d = eng._L.calls[1][1][1]
    assert [(x.lr, x.eps, x.max_norm) for x in d] == [(1e-3 * (i + 1), 1e-5 * (i + 1), 0.5 + i) for i in range(3)]
    assert [x.ws_dev for x in d] == [o.plan.workspace.data_ptr() for o in opts] and [g.data_ptr() for g in grp.grad_norms] == [o.plan.norm.data_ptr() for o in opts]
    # a moved .grad in member 1 rebuilds that member's plan alone and keeps its state; the member stays usable alone
    first = [o.plan for o in opts]
    opts[1].params[0].grad = torch.ones_like(opts[1].params[0])
    grp.step()
    assert opts[0].plan is first[0] and opts[2].plan is first[2] and opts[1].plan is not first[1] and opts[1].plan.state is first[1].state
    opts[1].step()
    assert [n for n, _ in eng._L.calls][2:] == ["ptg_optim_step_group", "ptg_optim_step"]
    assert sorted(opts[1].state_dict()["state"]) == [0, 1]   # checkpoints stay the members' own
