"""The NumPy restatement of ptg_optim_step (tests/optim_restatement.py) pinned against torch.optim.Adam, torch.optim.RMSprop,
clip_grad_norm_ and SB3's polyak_update in float64 on the CPU and by hand, and the parts of the call that need no device: the exported
symbols, the ABI version, the structs' sizes, the workspace size, the Python argument checks, the checkpoint layout.

Bound: 1e-12 * max(1, |ref|) per element.  What differs from torch is a few ulp each: the running products beta^t against torch's
beta ** t, m = beta1 * m + (1 - beta1) * g against torch's lerp, and the order of the norm's sum (math.fsum here)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import optim_restatement as orr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(7, 5), (5,), (1,), (3, 4, 2), (65,)]


def _err(got, ref):
    """max |got - ref| in units of 1e-12 * max(1, |ref|), per element"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(ref).all()
    return float((np.abs(got - ref) / (1e-12 * np.maximum(1.0, np.abs(ref)))).max())


def _arrays(seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=s) * scale for s in SHAPES]


def _sb3_polyak(params, targets, tau):
    """stable_baselines3/common/utils.py polyak_update, its two lines typed out"""
    import torch
    with torch.no_grad():
        for param, target_param in zip(params, targets):
            target_param.data.mul_(1 - tau)
            torch.add(target_param.data, param.data, alpha=tau, out=target_param.data)


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
@pytest.mark.parametrize("lr", [5e-5, 1e-2])
@pytest.mark.parametrize("max_norm", [None, 0.5, 1e6])
@pytest.mark.parametrize("tau", [0.005, 1.0])
def test_restatement_against_torch_five_steps(kind, lr, max_norm, tau):
    """five consecutive steps of clip_grad_norm_ + optimizer.step() + polyak_update in float64; clipping off (None), active (0.5:
    the total norm of these gradients is some 10) and inactive (1e6: the coefficient is exactly 1)"""
    import torch
    p0, q0 = _arrays(1), _arrays(2)
    tp = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in p0]
    tq = [torch.tensor(a, dtype=torch.float64) for a in q0]
    opt = torch.optim.Adam(tp, lr=lr, eps=1e-5) if kind == "adam" else torch.optim.RMSprop(tp, lr=lr, alpha=0.99, eps=1e-5)
    params, targets = [a.copy() for a in p0], [a.copy() for a in q0]
    s1, s2, st = [np.zeros_like(a) for a in p0], [np.zeros_like(a) for a in p0], orr.new_state()
    worst = 0.0
    for k in range(5):
        grads = _arrays(10 + k)
        for p, g in zip(tp, grads):
            p.grad = torch.tensor(g, dtype=torch.float64)
        ref_total = None if max_norm is None else float(torch.nn.utils.clip_grad_norm_(tp, max_norm))
        opt.step()
        _sb3_polyak(tp, tq, tau)
        r = orr.step(kind, params, grads, s1, s2, st, lr, eps=1e-5, alpha=0.99, max_norm=max_norm, targets=targets, tau=tau)
        params, s1, targets = r["params"], r["state1"], r["targets"]
        if kind == "adam":
            s2 = r["state2"]
        if max_norm is not None:
            worst = max(worst, abs(r["total"] - ref_total) / (1e-12 * max(1.0, abs(ref_total))))
            assert (r["coef"] == 1.0) == (max_norm == 1e6) and r["coef"] <= 1.0
        else:
            assert r["coef"] == 1.0 and r["total"] is None
        for i, p in enumerate(tp):
            ts = opt.state[p]
            worst = max(worst, _err(params[i], p.detach().numpy()), _err(targets[i], tq[i].numpy()))
            if kind == "adam":
                worst = max(worst, _err(s1[i], ts["exp_avg"].numpy()), _err(s2[i], ts["exp_avg_sq"].numpy()))
                assert float(ts["step"]) == st["t"] == k + 1
            else:
                worst = max(worst, _err(s1[i], ts["square_avg"].numpy()))
        assert worst <= 1.0, (k, worst)
    print(f"{kind} lr={lr} max_norm={max_norm} tau={tau}: max error / bound {worst:.5f}")


def test_two_elements_by_hand():
    """p = (1, -2), g = (3, 4): total 5.  Clip 2.5 -> coef = 2.5 / 5.000001, g' = g * coef.  Adam step 1 with beta = (0.9, 0.999): m = 0.1 g',
    v = 0.001 g'^2, step_size = lr / 0.1, bc2 = sqrt(0.001) -> p - lr * g' / (|g'| + eps * ...) ~ p - lr * sign(g) for a tiny eps"""
    p, g = [np.array([1.0, -2.0])], [np.array([3.0, 4.0])]
    z = [np.zeros(2)]
    r = orr.step("adam", p, g, z, z, orr.new_state(), lr=0.5, eps=0.0, max_norm=2.5)
    assert r["total"] == 5.0 and r["coef"] == 2.5 / 5.000001
    gp = g[0] * r["coef"]
    assert np.allclose(r["state1"][0], 0.1 * gp, rtol=1e-15, atol=0) and np.allclose(r["state2"][0], 0.001 * gp * gp, rtol=1e-15, atol=0)
    assert np.allclose(r["params"][0], [0.5, -2.5], rtol=0, atol=2e-15)          # six roundings of 2^-53 on magnitudes <= 2.5
    # unclipped (total 5 <= 10): the gradient itself, bit for bit
    r = orr.step("adam", p, g, z, z, orr.new_state(), lr=0.5, eps=0.0, max_norm=10.0)
    assert r["coef"] == 1.0 and np.allclose(r["state1"][0], [0.3, 0.4], rtol=1e-15, atol=0)
    # RMSprop, alpha 0.75, eps 1: s = 0.25 g^2 = (2.25, 4); p - 0.5 * g / (sqrt(s) + 1) = 1 - 1.5 / 2.5, -2 - 2 / 3
    r = orr.step("rmsprop", p, g, z, None, orr.new_state(), lr=0.5, eps=1.0, alpha=0.75)
    assert np.array_equal(r["state1"][0], [2.25, 4.0]) and np.allclose(r["params"][0], [0.4, -2.0 - 2.0 / 3.0], rtol=0, atol=1e-15)
    # Polyak: tau 0.25 of p onto q = (8, 8); tau = 1 is a copy
    q = [np.array([8.0, 8.0])]
    assert np.array_equal(orr.polyak(p, q, 0.25)[0], [6.25, 5.5]) and np.array_equal(orr.polyak(p, q, 1.0)[0], p[0])
    # a zero gradient: total 0, coefficient 1, nothing moves (v = 0, g = 0: 0 / (0 + eps))
    r = orr.step("adam", p, z, z, z, orr.new_state(), lr=0.5, eps=1e-8, max_norm=0.5, zero_grad=True)
    assert r["total"] == 0.0 and r["coef"] == 1.0 and np.array_equal(r["params"][0], p[0]) and np.array_equal(r["state2"][0], [0.0, 0.0])


def test_second_step_by_hand_the_running_products():
    st = orr.new_state()
    p, g, z = [np.array([0.0])], [np.array([1.0])], [np.zeros(1)]
    r = orr.step("adam", p, g, z, z, st, lr=0.1, eps=0.0)
    r = orr.step("adam", r["params"], g, r["state1"], r["state2"], st, lr=0.1, eps=0.0)
    assert st == {"t": 2.0, "p1": 0.9 * 0.9, "p2": 0.999 * 0.999}
    assert abs(r["params"][0][0] + 0.2) < 1e-15                # a constant gradient: bias-corrected m / sqrt(v) = 1, two steps of lr


def test_float32_rounds_once():
    """float32 tensors: float64 arithmetic, one rounding on the store; the moments entering the parameter update are the unrounded ones"""
    rng = np.random.default_rng(3)
    p, g = [rng.normal(size=33).astype(np.float32)], [rng.normal(size=33).astype(np.float32)]
    z = [np.zeros(33, np.float32)]
    r32 = orr.step("adam", p, g, z, z, orr.new_state(), lr=1e-2, max_norm=0.5)
    r64 = orr.step("adam", [p[0].astype(np.float64)], [g[0].astype(np.float64)], [z[0].astype(np.float64)], [z[0].astype(np.float64)], orr.new_state(),
                   lr=1e-2, max_norm=0.5)
    assert r32["params"][0].dtype == np.float32 and r32["total"] == r64["total"]
    for k in ("params", "state1", "state2"):
        assert np.array_equal(r32[k][0], r64[k][0].astype(np.float32)), k


# ------------------------------------------------------------------------------------------------- the ABI, without a device
def test_the_library_exports_the_three_symbols_at_abi_13():
    from rl_ptg_amd import _lib
    _lib.build()
    L = _lib.lib()
    for name in ("ptg_optim_step", "ptg_optim_workspace", "ptg_optim_chunk"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    assert L.ptg_abi_version() == 13
    assert (_lib.OPTIM_ADAM, _lib.OPTIM_RMSPROP, _lib.OPTIM_POLYAK, _lib.OPTIM_CLIP, _lib.OPTIM_TARGETS, _lib.OPTIM_ZERO_GRAD) == (0, 1, 2, 1, 2, 4)
    hdr = open(os.path.join(ROOT, "include", "ptg_env.h")).read()
    assert "PTG_OPTIM_ADAM = 0, PTG_OPTIM_RMSPROP = 1, PTG_OPTIM_POLYAK = 2" in hdr and "PTG_OPTIM_CLIP = 1, PTG_OPTIM_TARGETS = 2, PTG_OPTIM_ZERO_GRAD = 4" in hdr
    C_ = L.ptg_optim_chunk()
    assert C_ == 1024 and C_ % 256 == 0 and 300000 // C_ >= 256       # PPO's 0.3 M elements still cover the 256 CUs


def test_struct_sizes_and_offsets_match_the_c_compiler(tmp_path):
    import subprocess
    from rl_ptg_amd import _lib
    src = tmp_path / "sz.c"
    fields = ["dtype", "n_tensors", "chunks_dev", "state_dev", "lr_dev", "norm_dev", "ws_dev", "lr", "tau", "max_norm"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu %%zu", sizeof(ptg_optim), sizeof(ptg_optim_tensor), '
                   'sizeof(ptg_optim_span), offsetof(ptg_optim_tensor, numel), offsetof(ptg_optim_span, offset));\n%s\nreturn 0;}\n'
                   % (os.path.join(ROOT, "include", "ptg_env.h"), "\n".join('printf(" %%zu", offsetof(ptg_optim, %s));' % f for f in fields)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S, T, P = _lib.PtgOptim, _lib.PtgOptimTensor, _lib.PtgOptimSpan
    assert got == [C.sizeof(S), C.sizeof(T), C.sizeof(P), T.numel.offset, P.offset.offset] + [getattr(S, f).offset for f in fields]
    assert C.sizeof(T) == 48 and C.sizeof(P) == 16


def test_the_workspace_size_and_the_null_handle():
    from rl_ptg_amd import _lib
    L = _lib.lib()
    assert L.ptg_optim_workspace(0) < 0 and L.ptg_optim_workspace(-7) < 0 and L.ptg_optim_workspace(2 ** 31) < 0 and L.ptg_optim_workspace(2 ** 40) < 0
    assert L.ptg_optim_workspace(1) == 32 + 8 and L.ptg_optim_workspace(300) == 32 + 2400 and L.ptg_optim_workspace(2 ** 31 - 1) == 32 + 8 * (2 ** 31 - 1)
    assert L.ptg_optim_step(None, C.byref(_lib.PtgOptim()), None) == _lib.E_INVALID


# ------------------------------------------------------------------------------------------------- the Python layer, without a device
class _Lib:
    """stands in for the loaded library: records (name, args), answers the two size questions as the library does"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            if name == "ptg_optim_chunk":
                return 1024
            if name == "ptg_optim_workspace":
                return 32 + 8 * args[0] if 1 <= args[0] < 2 ** 31 else -1
            self.calls.append((name, args))
            return 0
        return f


def _recording_engine():
    from helpers import CpuTorch, host_engine
    return host_engine(4, _h="H", _L=_Lib(), _torch=CpuTorch(), _stream=lambda: None)


def _lists(torch, dt=None, n=(5, 1024, 1025, 2055)):
    dt = dt or torch.float32
    mk = lambda: [torch.zeros(k, dtype=dt) for k in n]
    return mk(), mk(), mk()


def test_what_reaches_the_library():
    import torch
    from rl_ptg_amd import _lib
    eng = _recording_engine()
    params, grads, targets = _lists(torch)
    plan = eng.optim_plan(params, grads, "adam", targets=targets)
    assert eng._L.calls == [] and plan.n_chunks == 1 + 1 + 2 + 3
    tab = plan.tensors_dev.numpy()
    assert tab.shape == (4, 6) and tab.dtype == np.int64
    for k in range(4):
        assert tab[k].tolist() == [params[k].data_ptr(), grads[k].data_ptr(), plan.state1[k].data_ptr(), plan.state2[k].data_ptr(), targets[k].data_ptr(), params[k].numel()]
    assert plan.chunks_dev.numpy().tolist() == [[0, 0], [1, 0], [2, 0], [2, 1024], [3, 0], [3, 1024], [3, 2048]]
    assert plan.state.tolist() == [0.0, 1.0, 1.0, 0.0] and plan.state.dtype == torch.float64 and plan.norm.shape == (1,)
    assert plan.workspace.numel() == 32 + 8 * 7 and all(s.dtype == torch.float32 and not s.any() for s in plan.state1 + plan.state2)
    lr = torch.zeros(1, dtype=torch.float64)
    eng.optim_step(plan, lr, betas=(0.8, 0.95), eps=1e-5, max_grad_norm=0.5, tau=0.005, zero_grad=True)
    eng.optim_step(plan, 3e-4, tau=1.0)
    (n0, a0), (n1, a1) = eng._L.calls
    assert n0 == n1 == "ptg_optim_step" and a0[0] == "H" and a0[2] is None
    d0, d1 = a0[1]._obj, a1[1]._obj
    assert (d0.kind, d0.flags, d0.dtype, d0.n_tensors, d0.n_chunks) == (_lib.OPTIM_ADAM, 7, _lib.OUT_F32, 4, 7)
    assert (d0.tensors_dev, d0.chunks_dev, d0.state_dev, d0.lr_dev, d0.norm_dev, d0.ws_dev) == (
        plan.tensors_dev.data_ptr(), plan.chunks_dev.data_ptr(), plan.state.data_ptr(), lr.data_ptr(), plan.norm.data_ptr(), plan.workspace.data_ptr())
    assert (d0.beta1, d0.beta2, d0.eps, d0.tau, d0.max_norm) == (0.8, 0.95, 1e-5, 0.005, 0.5)
    assert (d1.flags, d1.lr_dev, d1.lr, d1.beta1, d1.beta2, d1.eps, d1.alpha, d1.tau) == (_lib.OPTIM_TARGETS, None, 3e-4, 0.9, 0.999, 1e-8, 0.99, 1.0)
    # RMSprop in float64 without targets: one state tensor; the standalone Polyak call: one library call, the plan reused
    eng = _recording_engine()
    params, grads, targets = _lists(torch, torch.float64)
    plan = eng.optim_plan(params, grads, "rmsprop")
    assert plan.state2 == [] and plan.tensors_dev.numpy()[:, 3].tolist() == [0] * 4 and plan.tensors_dev.numpy()[:, 4].tolist() == [0] * 4
    eng.optim_step(plan, 7e-4, eps=1e-5, alpha=0.9)
    d = eng._L.calls[0][1][1]._obj
    assert (d.kind, d.flags, d.dtype, d.alpha, d.eps, d.lr) == (_lib.OPTIM_RMSPROP, 0, _lib.OUT_F64, 0.9, 1e-5, 7e-4)
    pp = eng.polyak_update(params, targets, 1.0)
    assert eng.polyak_update(params, targets, 0.5, plan=pp) is pp and len(eng._L.calls) == 3
    d = eng._L.calls[2][1][1]._obj
    assert (d.kind, d.flags, d.tau, d.state_dev, d.n_chunks) == (_lib.OPTIM_POLYAK, 0, 0.5, None, 7)
    assert pp.tensors_dev.numpy()[:, 1:4].tolist() == [[0, 0, 0]] * 4 and pp.tensors_dev.numpy()[:, 4].tolist() == [t.data_ptr() for t in targets]


def test_python_refusals_need_no_device():
    """every refusal comes before any allocation or library call (the shell has no library: an accepted call would die on None);
    TypeError for what a value is, ValueError for shapes, strides, devices and relations"""
    import torch
    from helpers import CpuTorch, host_engine
    from rl_ptg_amd import DeviceOptimizer
    eng = host_engine(4, _torch=CpuTorch())
    other = torch.device("meta")
    P = lambda: [torch.zeros(3, 4), torch.zeros(7)]
    params, grads, targets = P(), P(), P()
    plan_of = lambda **kw: eng.optim_plan(kw.pop("params", params), kw.pop("grads", grads), kw.pop("kind", "adam"), **kw)
    rec = _recording_engine()
    good = rec.optim_plan(params, grads, "adam", targets=targets)
    bare = rec.optim_plan(params, grads, "rmsprop")
    step = lambda plan=good, lr=1e-3, **kw: eng.optim_step(plan, lr, **dict(dict(tau=0.005) if plan is good else {}, **kw))
    refused = [
        (TypeError, lambda: plan_of(params=[params[0], params[1].double()])),                     # mixed dtypes
        (TypeError, lambda: plan_of(grads=[grads[0].double(), grads[1]])),
        (TypeError, lambda: plan_of(targets=[targets[0], targets[1].double()])),
        (TypeError, lambda: plan_of(params=[params[0].half(), params[1].half()], grads=[grads[0].half(), grads[1].half()])),
        (TypeError, lambda: plan_of(params=[params[0].numpy(), params[1]])),
        (TypeError, lambda: plan_of(params=[params[0].long(), params[1].long()])),
        (ValueError, lambda: plan_of(kind="sgd")),
        (ValueError, lambda: plan_of(params=[])),
        (ValueError, lambda: plan_of(params=[torch.zeros(4, 3).t(), params[1]])),                 # not contiguous
        (ValueError, lambda: plan_of(grads=[torch.zeros(4, 3).t(), grads[1]])),
        (ValueError, lambda: plan_of(params=[params[0].to(other), params[1]])),                   # wrong device
        (ValueError, lambda: plan_of(targets=[targets[0], targets[1].to(other)])),
        (ValueError, lambda: plan_of(grads=[grads[0], torch.zeros(8)])),                          # shape mismatch
        (ValueError, lambda: plan_of(grads=[torch.zeros(4, 3), grads[1]])),
        (ValueError, lambda: plan_of(targets=[torch.zeros(12), targets[1]])),
        (ValueError, lambda: plan_of(grads=grads[:1])),
        (ValueError, lambda: plan_of(grads=[grads[0], None])),                                    # a parameter without a gradient
        (ValueError, lambda: plan_of(grads=None)),
        (ValueError, lambda: plan_of(kind="polyak")),                                             # polyak takes no gradients ...
        (ValueError, lambda: plan_of(kind="polyak", grads=None)),                                 # ... and needs targets
        (ValueError, lambda: plan_of(params=[params[0], torch.zeros(0)], grads=[grads[0], torch.zeros(0)])),
        (TypeError, lambda: step(plan="plan")),
        (TypeError, lambda: step(lr=torch.zeros(1))),                                             # an lr tensor that is not float64
        (TypeError, lambda: step(lr=torch.zeros(2, dtype=torch.float64))),
        (ValueError, lambda: step(lr=torch.zeros(1, dtype=torch.float64, device=other))),
        (ValueError, lambda: step(lr=-1e-3)), (ValueError, lambda: step(lr=float("nan"))),
        (ValueError, lambda: step(tau=None)),                                                     # targets without tau
        (ValueError, lambda: step(tau=1.5)), (ValueError, lambda: step(tau=-0.1)), (ValueError, lambda: step(tau=float("nan"))),
        (ValueError, lambda: step(plan=bare, tau=0.5)),                                           # tau without targets
        (ValueError, lambda: step(max_grad_norm=-0.5)), (ValueError, lambda: step(max_grad_norm=float("nan"))),
        (ValueError, lambda: step(betas=(1.0, 0.999))), (ValueError, lambda: step(eps=-1.0)), (ValueError, lambda: step(plan=bare, alpha=-0.1)),
        (ValueError, lambda: eng.polyak_update(params, targets, 1.5)),
        (ValueError, lambda: eng.polyak_update(params, targets[:1], 0.5)),
        (TypeError, lambda: eng.polyak_update(params, targets, 0.5, plan=good)),                   # an optimiser's plan
        (TypeError, lambda: eng.polyak_update(params, [targets[0], targets[1].double()], 0.5)),
        (ValueError, lambda: DeviceOptimizer(eng, params, kind="sgd")),
        (ValueError, lambda: DeviceOptimizer(eng, [])),
        (ValueError, lambda: DeviceOptimizer(eng, params, targets=targets)),                       # targets without tau
        (ValueError, lambda: DeviceOptimizer(eng, params, tau=0.5)),
        (ValueError, lambda: DeviceOptimizer(eng, params, targets=targets, tau=2.0)),
        (ValueError, lambda: DeviceOptimizer(eng, params, max_grad_norm=-1.0)),
        (TypeError, lambda: DeviceOptimizer(eng, params, lr=torch.zeros(1))),
        (ValueError, lambda: DeviceOptimizer(eng, params).step()),                                 # .grad is None
    ]
    for k, (exc, fn) in enumerate(refused):
        with pytest.raises(exc):
            fn()
        assert eng._L is None, k


def test_state_dict_round_trip_and_a_torch_adam_checkpoint():
    """torch.optim's layout both ways: a torch.optim.Adam state loads here (moments copied, the device state becomes {t, beta1^t,
    beta2^t}), what state_dict() gives loads into a fresh torch.optim.Adam, and a round trip through a second DeviceOptimizer is exact"""
    import torch
    from rl_ptg_amd import DeviceOptimizer
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.ReLU(), torch.nn.Linear(8, 2)).double()
    ref = torch.optim.Adam(net.parameters(), lr=3e-4, betas=(0.8, 0.95), eps=1e-5)
    for _ in range(3):
        ref.zero_grad()
        net(torch.randn(5, 4, dtype=torch.float64)).square().sum().backward()
        ref.step()
    sd = ref.state_dict()
    eng = _recording_engine()
    opt = DeviceOptimizer(eng, net.parameters(), kind="adam", lr=1.0)
    assert opt.state_dict()["state"] == {} and opt.grad_norm is None
    opt.load_state_dict(sd)
    assert (opt.lr, opt.betas, opt.eps) == (3e-4, (0.8, 0.95), 1e-5)
    assert opt.plan.state.tolist() == [3.0, 0.8 ** 3.0, 0.95 ** 3.0, 0.0]
    for k, p in enumerate(net.parameters()):
        assert torch.equal(opt.plan.state1[k], sd["state"][k]["exp_avg"]) and torch.equal(opt.plan.state2[k], sd["state"][k]["exp_avg_sq"])
    out = opt.state_dict()
    assert sorted(out["state"]) == [0, 1, 2, 3] and out["param_groups"][0]["params"] == [0, 1, 2, 3] and out["param_groups"][0]["betas"] == (0.8, 0.95)
    for k in range(4):
        assert float(out["state"][k]["step"]) == 3.0 and sorted(out["state"][k]) == ["exp_avg", "exp_avg_sq", "step"]
        assert torch.equal(out["state"][k]["exp_avg"], sd["state"][k]["exp_avg"]) and torch.equal(out["state"][k]["exp_avg_sq"], sd["state"][k]["exp_avg_sq"])
    back = torch.optim.Adam(net.parameters(), lr=3e-4, betas=(0.8, 0.95), eps=1e-5)
    merged = back.state_dict()
    merged["state"] = out["state"]
    back.load_state_dict(merged)                                                                  # torch accepts the layout
    assert float(back.state[next(iter(net.parameters()))]["step"]) == 3.0
    twin = DeviceOptimizer(_recording_engine(), net.parameters(), kind="adam", lr=1.0)
    twin.load_state_dict(out)
    assert twin.plan.state.tolist() == opt.plan.state.tolist() and all(torch.equal(a, b) for a, b in zip(twin.plan.state2, opt.plan.state2))
    opt.step()                                                                                    # gradients in place since the load: one call
    assert [n for n, _ in eng._L.calls] == ["ptg_optim_step"] and opt.step() is None
    # RMSprop: square_avg
    net2 = torch.nn.Linear(3, 2)
    ref2 = torch.optim.RMSprop(net2.parameters(), lr=7e-4, alpha=0.9, eps=1e-5)
    net2(torch.randn(4, 3)).sum().backward()
    ref2.step()
    opt2 = DeviceOptimizer(_recording_engine(), net2.parameters(), kind="rmsprop", lr=1.0)
    opt2.load_state_dict(ref2.state_dict())
    assert (opt2.lr, opt2.alpha, opt2.eps) == (7e-4, 0.9, 1e-5) and opt2.plan.state.tolist()[0] == 1.0
    out2 = opt2.state_dict()
    assert sorted(out2["state"][0]) == ["square_avg", "step"] and torch.equal(out2["state"][1]["square_avg"], ref2.state_dict()["state"][1]["square_avg"])
    with pytest.raises(ValueError):
        opt2.load_state_dict(sd)                                                                  # four parameters into two


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_a_moved_gradient_rebuilds_the_tables_and_keeps_the_state(kind):
    import torch
    from rl_ptg_amd import DeviceOptimizer
    eng = _recording_engine()
    w = torch.zeros(5, requires_grad=True)
    w.grad = torch.ones(5)
    opt = DeviceOptimizer(eng, [w], kind=kind, lr=1e-3, zero_grad=True)
    opt.step()
    first = opt.plan
    opt.step()
    assert opt.plan is first                                                                      # nothing moved: the same tables
    opt.zero_grad(set_to_none=True)
    with pytest.raises(ValueError):
        opt.step()
    w.grad = torch.ones(5)
    opt.step()
    assert opt.plan is not first and opt.plan.state is first.state and opt.plan.state1[0] is first.state1[0]
    assert opt.plan.tensors_dev.numpy()[0, 1] == w.grad.data_ptr() and len(eng._L.calls) == 3
