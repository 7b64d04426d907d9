"""The NumPy restatement of ptg_rsample / ptg_rsample_backward / ptg_actor_loss (tests/actor_restatement.py) pinned against torch CPU
autograd of SB3's own lines (typed out in float64: neither stable_baselines3 nor sb3_contrib is needed) and by hand, the inputs of
the GPU tests vetted for the conditioning their bounds rest on, and the parts of the calls that need no device: the exported symbols,
the structs' layout, the workspace size, the Python argument checks and what reaches the library.
Bounds: 1e-12 * max(1, |ref|); for gradients scaled by 1 / n, n * gradient within 1e-12 * max(1, max |n * ref|)."""
import ctypes as C
import os

import numpy as np
import pytest

import actor_restatement as at
from rl_ptg_amd._lib import PtgAl, PtgRs  # noqa: F401  (the descriptors the restatement speaks for: without them nothing here applies)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_BS = [1, 2, 65, 257, 290, 470]
_worst = {}


def _close(got, ref, scale_by=1.0):
    """max |got - ref| * scale_by in units of 1e-12 * max(1, max |ref * scale_by|)"""
    got, ref = np.asarray(got, np.float64) * scale_by, np.asarray(ref, np.float64) * scale_by
    assert got.shape == ref.shape and np.isfinite(ref).all()
    return float(np.abs(got - ref).max() / (1e-12 * max(1.0, float(np.abs(ref).max()))))


def _stat(got, ref):
    return abs(got - ref) / (1e-12 * max(1.0, abs(ref)))


# ------------------------------------------------------------------------------------------------- rsample and its backward
@pytest.mark.parametrize("B", HOST_BS)
def test_rsample_restatement_against_torch_autograd(B):
    """forward and backward at the drawn z, at z = 0 (the deterministic call) and with either incoming gradient alone; the planted
    rows (log_std exactly -20 and 2, one spacing outside each) are rows 0 .. 3.
    One comparison is left out, for torch's sake: d / d mean on the two rows at the lower clamp edge when z != 0.  There autograd adds
    +t and -t with t = gl * z / sigma = gl * z * 4.9e8 (the paths through the sample and through Normal's loc) around the tanh term, which
    loses that term's low bits to ulp(t) ~ 1e-7; the closed form has no such pair.  The same rows ARE compared at z = 0, where t = 0."""
    worst = 0.0
    for dt in at.DTYPES:
        for z in (at.draw(at.SEED, 0, B), np.zeros(B)):
            mean, ls = at.rs_case(B, dt, z)
            ga, gl = at.grads_case(B, dt)
            f = at.rsample(mean, ls, z)
            assert not f["bad"].any()
            rows = slice(2, None) if z.any() else slice(None)
            for a, l in ((ga, gl), (ga, None), (None, gl)):
                act, logp, gm, gs = at.sb3_action_log_prob(mean, ls, z, a, l)
                b = at.rsample_backward(mean, ls, z, a, l)
                e = [_close(f["act"], act), _close(f["logp"], logp), _close(b["grad_log_std"], gs)]
                if len(gm[rows]):
                    e.append(_close(b["grad_mean"][rows], gm[rows]))
                worst = max(worst, *e)
                assert max(e) <= 1.0, (B, dt, e)
    print(f"rsample B={B}: max error / tolerance {worst:.4f}")


def test_the_clamp_edges_are_what_they_say():
    """log_std exactly at an edge passes its gradient (torch's clamp is inclusive), one spacing outside it does not and the value is the
    edge's; a NaN stays; an infinite log_std clamps and is legal"""
    for dt in at.DTYPES:
        z = at.draw(at.SEED, 3, 8)
        mean, ls = at.rs_case(8, dt, z)
        assert ls[0] == -20 and ls[1] < -20 and ls[2] == 2 and ls[3] > 2 and float(ls[1]) == float(np.nextafter(dt(-20), dt(-30)))
        c, ok = at.clamp_log_std(ls.astype(np.float64))
        assert c[:4].tolist() == [-20.0, -20.0, 2.0, 2.0] and ok[:4].tolist() == [True, False, True, False] and ok[4:].all()
        ga, gl = at.grads_case(8, dt)
        b = at.rsample_backward(mean, ls, z, ga, gl)
        assert b["grad_log_std"][1] == 0.0 and b["grad_log_std"][3] == 0.0 and b["grad_log_std"][0] != 0.0 and b["grad_log_std"][2] != 0.0
        _, _, gm, gs = at.sb3_action_log_prob(mean, ls, z, ga, gl)
        assert gs[1] == 0.0 and gs[3] == 0.0 and gs[0] != 0.0 and gs[2] != 0.0
    l = np.array([np.nan, np.inf, -np.inf, 0.5])
    c, ok = at.clamp_log_std(l)
    assert np.isnan(c[0]) and c[1:].tolist() == [2.0, -20.0, 0.5] and ok.tolist() == [False, False, False, True]
    f = at.rsample(np.zeros(4), l, np.ones(4))
    assert f["bad"].tolist() == [True, False, False, False] and np.isnan(f["act"][0]) and np.isfinite(f["logp"][1:]).all()
    b = at.rsample_backward(np.array([0.0, np.inf, 0.0, 0.0, 0.0]), np.zeros(5), np.array([1.0, 1.0, np.nan, 1.0, 1.0]),
                            np.array([1.0, 1.0, 1.0, np.inf, 1.0]), np.ones(5))
    assert b["bad"].tolist() == [False, True, True, True, False] and np.isnan(b["grad_mean"][1:4]).all() and np.isfinite(b["grad_mean"][[0, 4]]).all()


def test_the_inputs_of_the_gpu_tests_are_well_conditioned():
    """what the GPU bounds rest on: at every (B, dtype, counter) the GPU sweep draws, every unplanted row has |g| < 4, so 1 - tanh(g)^2 +
    1e-6 > 1.3e-3 and a last-place difference between two tanh implementations moves its log by less than 1e-12 (DESIGN.md section 12's
    argument); the planted rows sit at g = 0.3; every incoming gradient is at most 4 in magnitude; |z| <= 6.66"""
    worst = 0.0
    for B in at.BS + [at.B_BIG]:
        for dt in at.DTYPES:
            for c in range(4):
                z = at.draw(at.SEED, c, B)
                mean, ls = at.rs_case(B, dt, z)
                g = at.rsample(mean, ls, z)["g"]
                assert np.abs(g[at.N_PLANTED_RS:]).max(initial=0.0) < 4.0 and np.abs(z).max() <= 6.66
                assert np.abs(g[2:at.N_PLANTED_RS] - 0.3).max(initial=0.0) < 1e-4
                worst = max(worst, float(np.abs(g).max()))
            ga, gl = at.grads_case(B, dt)
            assert np.abs(ga).max() <= 4.0 and np.abs(gl).max() <= 4.0
    print(f"largest |g| over the GPU tests' inputs: {worst:.3f}")
    assert 1.0 - np.tanh(4.0) ** 2 + 1e-6 > 1.3e-3


def test_smooth_restatement_against_torch():
    import torch
    for B in HOST_BS:
        z = at.draw(at.SEED, 1, B)
        mean = np.random.default_rng(B).uniform(-1.2, 1.2, B)
        t = torch.from_numpy
        noise = (t(z) * 0.2).clamp(-0.5, 0.5)                # normal_(0, target_policy_noise) is target_policy_noise * z
        want = (t(mean) + noise).clamp(-1, 1).numpy()
        got = at.smooth(mean, z, 0.2, 0.5)
        assert np.array_equal(got["act"], want) and (np.abs(want) == 1.0).any() == (B > 2)
    assert at.smooth([0.0, np.nan, np.inf], [9.0, 0.0, 0.0], 1.0, 0.5)["act"].tolist()[0] == 0.5


def test_one_row_by_hand():
    """B = 1, mean 0, log_std 0 (sigma 1), z = 0: g = 0, a = 0, logp = -0.5 log 2 pi - log(1 + 1e-6); d = 1, q = 0, so grad_mean = ga and
    grad_log_std = -gl.  SAC with alpha 0.5, lp = -2, critics (3, 1): m = 1, term = -1 - 1 = -2; the gradient goes to critic 1.  TQC
    with one row of K = 2, Q = 2 quantiles (1, 3), (5, 7): m = (2 + 6) / 2 = 4.  The entropy coefficient: log alpha = ln 2, lp = -2,
    H_t = -1: S / B = -3, loss = 3 ln 2, gradient 3"""
    f = at.rsample([0.0], [0.0], [0.0])
    assert f["act"][0] == 0.0 and f["logp"][0] == -0.9189385332046727 - np.log(1.0 + 1e-6)
    b = at.rsample_backward([0.0], [0.0], [0.0], [0.75], [0.5])
    assert b["grad_mean"][0] == 0.75 and b["grad_log_std"][0] == -0.5
    r = at.actor_loss("min", [np.array([3.0]), np.array([1.0])], [-2.0], alpha=0.5)
    assert np.array_equal(r["stats"], [-2.0, 0.0, -2.0, 1.0, 0.5, 0.0, 0.0, 0.0])
    assert r["grad_q"][0][0] == 0.0 and r["grad_q"][1][0] == -1.0 and r["grad_lp"][0] == 0.5
    r = at.actor_loss("mean", [np.array([[1.0, 3.0]]), np.array([[5.0, 7.0]])], [-2.0], alpha=0.5)
    assert np.array_equal(r["stats"], [-5.0, 0.0, -2.0, 4.0, 0.5, 0.0, 0.0, 0.0]) and np.array_equal(r["grad_q"][1], [[-0.25, -0.25]])
    r = at.actor_loss("mean", [np.array([[1.5]])])                                  # TD3
    assert np.array_equal(r["stats"], [-1.5, 0.0, 0.0, 1.5, 0.0, 0.0, 0.0, 0.0]) and r["grad_q"][0][0, 0] == -1.0
    r = at.actor_loss("alpha_only", None, [-2.0], alpha=2.0, log_alpha=np.log(2.0), target_entropy=-1.0)
    assert np.array_equal(r["stats"], [0.0, 3.0 * np.log(2.0), -2.0, 0.0, 2.0, 3.0, 0.0, 0.0]) and r["grad_la"] == 3.0 and r["grad_q"] is None


# ------------------------------------------------------------------------------------------------- the losses
@pytest.mark.parametrize("B", HOST_BS)
@pytest.mark.parametrize("K", [1, 2, 4])
def test_sac_and_td3_restatement_against_torch_autograd(B, K):
    alpha, log_alpha = 0.3172, -1.3125
    c = at.al_case(B, K, 1, np.float64)
    q = at.al_flat(c)
    loss, gq, glp = at.sb3_actor_lines("sac", q, c["lp"], alpha)
    r = at.actor_loss("min", q, c["lp"], alpha=alpha, log_alpha=log_alpha, target_entropy=at.H_T)
    el, gla, _ = at.sb3_ent_coef_lines(c["lp"], log_alpha, at.H_T)
    assert not r["bad"].any()
    e = [_stat(r["stats"][0], loss), _stat(r["stats"][1], el), _stat(r["stats"][5], gla), _stat(r["stats"][2], c["lp"].mean()),
         _stat(r["stats"][3], np.min(np.stack(q), axis=0).mean()), _close(r["grad_lp"], glp, B)] + [_close(g, w, B) for g, w in zip(r["grad_q"], gq)]
    assert r["stats"][4] == alpha and r["grad_la"] == r["stats"][5]
    assert r["grad_q"][0][0] == -1.0 / B and all(g[0] == 0.0 for g in r["grad_q"][1:])              # equal critics: the first index wins
    if B > 1:
        assert r["grad_q"][K - 1][1] == -1.0 / B
    loss3, gq3, _ = at.sb3_actor_lines("td3", q[:1])
    r3 = at.actor_loss("mean", [c["q"][0]])
    e += [_stat(r3["stats"][0], loss3), _close(r3["grad_q"][0][:, 0], gq3[0], B)]
    assert r3["stats"][1] == 0.0 and r3["stats"][2] == 0.0 and r3["stats"][4] == 0.0 and r3["grad_la"] is None
    print(f"sac / td3 B={B} K={K}: max error / tolerance {max(e):.4f}")
    assert max(e) <= 1.0, e


@pytest.mark.parametrize("B", HOST_BS)
@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("Q", [1, 25, 30, 64])
def test_tqc_restatement_against_torch_autograd(B, K, Q):
    alpha = 0.00047                                          # the reference's
    c = at.al_case(B, K, Q, np.float64)
    loss, gq, glp = at.sb3_actor_lines("tqc", c["q"], c["lp"], alpha)
    r = at.actor_loss("mean", c["q"], c["lp"], alpha=alpha)
    n = B * K * Q
    e = [_stat(r["stats"][0], loss), _stat(r["stats"][3], np.stack(c["q"], axis=1).mean()), _close(r["grad_lp"], glp, B)] + \
        [_close(g, w, n) for g, w in zip(r["grad_q"], gq)]
    assert not r["bad"].any() and r["stats"][1] == 0.0 and r["stats"][5] == 0.0
    _worst["tqc"] = max(_worst.get("tqc", 0.0), *e)
    print(f"tqc B={B} K={K} Q={Q}: max error / tolerance {max(e):.4f} (so far {_worst['tqc']:.4f})")
    assert max(e) <= 1.0, e


@pytest.mark.parametrize("B", HOST_BS)
def test_ent_coef_restatement_against_torch_autograd(B):
    c = at.al_case(B, 1, 1, np.float64)
    for log_alpha in (-1.3125, 0.5, -7.66):
        el, gla, alpha = at.sb3_ent_coef_lines(c["lp"], log_alpha, at.H_T)
        r = at.actor_loss("alpha_only", None, c["lp"], alpha=alpha, log_alpha=log_alpha, target_entropy=at.H_T)
        e = [_stat(r["stats"][1], el), _stat(r["stats"][5], gla), _stat(r["stats"][2], c["lp"].mean())]
        assert r["stats"][0] == 0.0 and r["stats"][3] == 0.0 and r["stats"][4] == alpha and max(e) <= 1.0, e


def test_bad_rows_of_the_restatement():
    """a NaN critic wins the minimum (torch.min's rule) and makes the row bad; a +Inf beside a smaller value is legal; a -Inf minimum,
    a non-finite log-prob, any non-finite quantile and a non-finite alpha are bad"""
    import torch
    c = at.al_case(16, 2, 1, np.float64)
    q = at.al_flat(c)
    q[1][3] = np.nan; q[0][4] = np.nan; q[0][5] = np.inf; q[1][6] = -np.inf; c["lp"][7] = np.inf
    r = at.actor_loss("min", q, c["lp"], alpha=0.2)
    assert np.nonzero(r["bad"])[0].tolist() == [3, 4, 6, 7] and np.isnan(r["stats"][[0, 1, 2, 3, 5]]).all() and r["stats"][4] == 0.2
    assert np.isnan(r["grad_q"][0][[3, 4, 6, 7]]).all() and np.isnan(r["grad_lp"][[3, 4, 6, 7]]).all() and r["grad_q"][1][5] == -1.0 / 16
    assert torch.isnan(torch.min(torch.tensor([1.0, float("nan")])))          # the rule the restatement follows
    c = at.al_case(16, 2, 30, np.float64)
    c["q"][1][2, 29] = np.inf; c["q"][0][9, 0] = np.nan
    r = at.actor_loss("mean", c["q"], c["lp"], alpha=0.2)
    assert np.nonzero(r["bad"])[0].tolist() == [2, 9] and np.isnan(r["grad_q"][0][2]).all() and np.isfinite(r["grad_q"][0][3]).all()
    for a, la in ((np.nan, None), (np.inf, 800.0), (0.0, -np.inf)):
        r = at.actor_loss("min", q[:1], c["lp"], alpha=a, log_alpha=la, target_entropy=-1.0 if la is not None else None)
        assert r["bad"].all()


# ------------------------------------------------------------------------------------------------- the ABI, without a device
def test_the_library_exports_the_symbols_and_the_abi_stays_13():
    from rl_ptg_amd import _lib
    _lib.build()
    L = _lib.lib()
    names = ("ptg_rsample", "ptg_rsample_backward", "ptg_actor_loss", "ptg_actor_loss_workspace")
    assert all(hasattr(L, n) and n in _lib.EXPORTS for n in names)
    assert L.ptg_abi_version() == 13
    assert (_lib.RS_SQUASH, _lib.RS_SMOOTH, _lib.RS_DETERMINISTIC) == (0, 1, 1)
    assert (_lib.AL_MIN, _lib.AL_MEAN, _lib.AL_ALPHA_ONLY, _lib.AL_ENTROPY, _lib.AL_LOG_ALPHA, _lib.AL_ENT_COEF) == (0, 1, 2, 1, 2, 4)
    hdr = open(os.path.join(ROOT, "include", "ptg_env.h")).read()
    assert "PTG_RS_SQUASH = 0, PTG_RS_SMOOTH = 1" in hdr and "PTG_RS_DETERMINISTIC = 1" in hdr
    assert "PTG_AL_MIN = 0, PTG_AL_MEAN = 1, PTG_AL_ALPHA_ONLY = 2" in hdr and "PTG_AL_ENTROPY = 1, PTG_AL_LOG_ALPHA = 2, PTG_AL_ENT_COEF = 4" in hdr


def test_the_struct_layouts_match_the_c_compiler(tmp_path):
    import subprocess
    from rl_ptg_amd import _lib
    fields = {"ptg_rs": ["batch", "mean_dev", "log_std_s_n", "seed", "counter_dev", "noise_std", "clip_hi", "act_dev", "noise_dev", "grad_act_dev",
                         "grad_mean_dev", "gm_s_n", "grad_log_std_dev", "gl_s_n"],
              "ptg_al": ["n_quantiles", "q_dtype", "batch", "q_dev", "q_s_n", "logp_dev", "alpha_dev", "alpha", "target_entropy", "stats_dev", "grad_q_dev",
                         "g_s_n", "grad_logp_dev", "grad_log_alpha_dev", "ws_dev"]}
    body = "\n".join('printf("%%zu", sizeof(%s));\n%s\nprintf("\\n");' % (s, "\n".join('printf(" %%zu", offsetof(%s, %s));' % (s, f) for f in fs))
                     for s, fs in fields.items())
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){%s return 0;}\n' % (os.path.join(ROOT, "include", "ptg_env.h"), body))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().strip().split("\n")
    for line, (s, fs), S in zip(lines, fields.items(), (_lib.PtgRs, _lib.PtgAl)):
        assert [int(x) for x in line.split()] == [C.sizeof(S)] + [getattr(S, f).offset for f in fs], s


def test_the_workspace_size_and_the_null_handle():
    from rl_ptg_amd import _lib
    L = _lib.lib()
    W = L.ptg_actor_loss_workspace
    assert W(0) < 0 and W(-5) < 0 and W(1) == W(256) == 64 and W(257) == 128 and W(at.B_BIG) == 258 * 64
    assert W(2 ** 31) == 2 ** 23 * 64 and W(2 ** 31 + 1) < 0 and W(2 ** 40) < 0
    assert L.ptg_actor_loss(None, C.byref(_lib.PtgAl()), None) == _lib.E_INVALID
    assert L.ptg_rsample(None, C.byref(_lib.PtgRs()), None) == _lib.E_INVALID and L.ptg_rsample_backward(None, C.byref(_lib.PtgRs()), None) == _lib.E_INVALID


# ------------------------------------------------------------------------------------------------- the Python argument checks
def test_python_argument_checks_need_no_device():
    import torch
    from helpers import host_engine
    eng = host_engine(4)
    B = 6
    col, col1, cnt = torch.zeros(B), torch.zeros(B, 1), torch.zeros(1, dtype=torch.int64)
    z = torch.zeros(B, dtype=torch.float64)
    a64 = torch.zeros(1, dtype=torch.float64)
    quant = torch.zeros(B, 2, 30)
    other = torch.device("meta")
    rs = lambda **kw: eng.rsample(**{**dict(mean=col, log_std=col, counter=cnt), **kw})
    bw = lambda **kw: eng.rsample_backward(**{**dict(mean=col, log_std=col, noise=z, grad_actions=col, grad_log_prob=col), **kw})
    sm = lambda **kw: eng.smooth_target_action(**{**dict(mean=col, counter=cnt, noise_std=0.2, noise_clip=0.5), **kw})
    sac = lambda **kw: eng.actor_loss(**{**dict(kind="sac", q=[col, col1], log_prob=col, ent_coef=0.2), **kw})
    tqc = lambda **kw: eng.actor_loss(**{**dict(kind="tqc", q=quant, log_prob=col, log_ent_coef=a64), **kw})
    td3 = lambda **kw: eng.actor_loss(**{**dict(kind="td3", q=col1), **kw})
    ec = lambda **kw: eng.actor_loss(**{**dict(kind="ent_coef", log_prob=col, log_ent_coef=a64, target_entropy=-1.0), **kw})
    stats = torch.zeros(8, dtype=torch.float64)
    refused = [
        # rsample: what the tensors are, then shape, strides, device; then the counter; then out
        (TypeError, lambda: rs(mean=col.numpy())), (TypeError, lambda: rs(mean=col.half())), (TypeError, lambda: rs(mean=torch.zeros(B, 3, dtype=torch.int32))),
        (TypeError, lambda: rs(log_std=col.double())), (TypeError, lambda: rs(log_std=None)), (TypeError, lambda: rs(log_std=torch.zeros(B + 1, dtype=torch.float64))),
        (ValueError, lambda: rs(mean=torch.zeros(B, 2))), (ValueError, lambda: rs(log_std=torch.zeros(B + 1))), (ValueError, lambda: rs(mean=torch.zeros(1).expand(B))),
        (ValueError, lambda: rs(mean=torch.zeros(B, device=other))), (ValueError, lambda: rs(mean=col[:0], log_std=col[:0])),
        (ValueError, lambda: rs(counter=None)), (TypeError, lambda: rs(counter=torch.zeros(1, dtype=torch.int32))), (TypeError, lambda: rs(counter=torch.zeros(2, dtype=torch.int64))),
        (ValueError, lambda: rs(out=(col, col))), (ValueError, lambda: rs(out=[col, col, z])), (ValueError, lambda: rs(out=(col.double(), None, None))),
        (ValueError, lambda: rs(out=(None, col, z))), (ValueError, lambda: rs(out=(torch.zeros(2 * B)[::2], None, None))), (ValueError, lambda: rs(out=(col, col, z.float()))),
        (ValueError, lambda: rs(out=(col, torch.zeros(B + 1), z))),
        # rsample_backward
        (TypeError, lambda: bw(noise=z.float())), (TypeError, lambda: bw(noise=None)), (ValueError, lambda: bw(noise=torch.zeros(B + 1, dtype=torch.float64))),
        (TypeError, lambda: bw(grad_actions=col.double())), (ValueError, lambda: bw(grad_log_prob=torch.zeros(2 * B)[::2])), (ValueError, lambda: bw(grad_actions=None, grad_log_prob=None)),
        (TypeError, lambda: bw(mean=col.long())), (ValueError, lambda: bw(out=(col,))), (ValueError, lambda: bw(out=(col, col.double()))), (ValueError, lambda: bw(out=(col, torch.zeros(B + 1)))),
        # smooth_target_action
        (TypeError, lambda: sm(mean=[0.0] * B)), (ValueError, lambda: sm(counter=None)), (ValueError, lambda: sm(noise_std=-0.1)), (ValueError, lambda: sm(noise_std=float("inf"))),
        (ValueError, lambda: sm(noise_std=float("nan"))), (ValueError, lambda: sm(noise_clip=-1.0)), (ValueError, lambda: sm(noise_clip=float("nan"))), (ValueError, lambda: sm(clip=(1.0, -1.0))),
        (ValueError, lambda: sm(out=col.double())), (ValueError, lambda: sm(out=torch.zeros(B + 1))),
        # actor_loss: the kind, q, log_prob, the relations, the coefficients, out and workspace
        (ValueError, lambda: sac(kind="dqn")), (TypeError, lambda: sac(q=col)), (TypeError, lambda: sac(q=None)), (ValueError, lambda: sac(q=[])), (ValueError, lambda: sac(q=[col] * 5)),
        (TypeError, lambda: sac(q=[col, col.double()])), (TypeError, lambda: sac(q=[col.half()])), (ValueError, lambda: sac(q=[col, torch.zeros(B + 1)])), (ValueError, lambda: sac(q=[torch.zeros(B, 2)])),
        (ValueError, lambda: sac(q=[torch.zeros(B, device=other)])), (TypeError, lambda: sac(log_prob=col.double())), (ValueError, lambda: sac(log_prob=None)),
        (ValueError, lambda: sac(log_prob=torch.zeros(B + 1))), (ValueError, lambda: sac(log_prob=torch.zeros(2 * B)[::2])),
        (ValueError, lambda: sac(ent_coef=None)), (ValueError, lambda: sac(log_ent_coef=a64)), (ValueError, lambda: sac(target_entropy=-1.0)),
        (ValueError, lambda: sac(ent_coef=None, log_ent_coef=a64, target_entropy=float("nan"))), (TypeError, lambda: sac(ent_coef=torch.zeros(1))),
        (TypeError, lambda: sac(ent_coef=None, log_ent_coef=0.5)), (TypeError, lambda: sac(ent_coef=torch.zeros(2, dtype=torch.float64))),
        (TypeError, lambda: tqc(q=quant.half())), (ValueError, lambda: tqc(q=torch.zeros(B, 5, 30))), (ValueError, lambda: tqc(q=torch.zeros(B, 2, 65))), (ValueError, lambda: tqc(q=torch.zeros(B, 30, 2).transpose(1, 2))),
        (ValueError, lambda: tqc(q=[torch.zeros(B, 30), torch.zeros(B, 29)])), (ValueError, lambda: tqc(log_prob=torch.zeros(B - 1))),
        (ValueError, lambda: td3(log_prob=col)), (ValueError, lambda: td3(ent_coef=0.2)), (ValueError, lambda: td3(q=[col, col])), (TypeError, lambda: td3(q=col.long())), (TypeError, lambda: td3(q=None)),
        (ValueError, lambda: ec(q=[col])), (ValueError, lambda: ec(target_entropy=None)), (ValueError, lambda: ec(log_ent_coef=None)), (ValueError, lambda: ec(log_ent_coef=None, ent_coef=0.2)),
        (ValueError, lambda: ec(log_prob=None)), (TypeError, lambda: ec(log_prob=col.long())), (ValueError, lambda: ec(target_entropy=float("inf"))),
        (ValueError, lambda: sac(out=(stats, [col], None))), (ValueError, lambda: sac(out=[stats, [col, col1], None, None])), (ValueError, lambda: sac(out=(stats.float(), [torch.zeros(B), col1.clone()], None, None))),
        (ValueError, lambda: sac(out=(stats, [torch.zeros(B), torch.zeros(B).double()], None, None))), (ValueError, lambda: sac(out=(stats, [torch.zeros(B), torch.zeros(B)], None, a64))),
        (ValueError, lambda: sac(out=(stats, [col, torch.zeros(B)], None, None))),                               # an input given as an output
        (ValueError, lambda: sac(out=(stats, [torch.zeros(B), torch.zeros(B)], torch.zeros(B + 1), None))), (ValueError, lambda: td3(out=(stats, torch.zeros(B, 1), torch.zeros(B), None))),
        (ValueError, lambda: tqc(out=(stats, [torch.zeros(B, 30)] * 2, None, None))), (ValueError, lambda: tqc(out=(stats, torch.zeros(B, 2, 29), None, None))),
        (ValueError, lambda: ec(out=(stats, [col], None, None))), (ValueError, lambda: ec(out=(stats, None, torch.zeros(B), None))), (ValueError, lambda: ec(out=(stats, None, None, torch.zeros(1)))),
        (ValueError, lambda: td3(out=(stats, torch.zeros(B, 1), None, None), workspace=torch.zeros(4096))),
    ]
    for k, (exc, fn) in enumerate(refused):
        with pytest.raises(exc):
            fn()
        assert eng._L is None, k


def test_a_refusal_reaches_nothing_and_a_good_call_reaches_the_library_once():
    import torch
    from helpers import recording_engine
    from rl_ptg_amd import _lib
    eng = recording_engine(4)
    B = 300
    wide = torch.zeros(B, 2, dtype=torch.float64)
    mean, ls = wide[:, 0], wide[:, 1:]                       # [B] with stride 2 and [B, 1] with row stride 2
    cnt = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(TypeError):
        eng.rsample(mean, ls.float(), cnt)
    with pytest.raises(ValueError):
        eng.rsample(mean, ls, None)
    with pytest.raises(ValueError):
        eng.smooth_target_action(mean, cnt, -1.0, 0.5)
    with pytest.raises(ValueError):
        eng.actor_loss("sac", [mean], mean.contiguous(), ent_coef=0.1, workspace=torch.zeros(10))
    assert eng._L.calls == []
    res = eng.rsample(mean, ls, cnt, seed=2 ** 64 + 5)
    assert [c[0] for c in eng._L.calls] == ["ptg_rsample"]
    d = eng._L.calls[0][1][1]._obj
    assert (d.kind, d.flags, d.q_dtype, d.batch, d.mean_dev, d.mean_s_n, d.log_std_dev, d.log_std_s_n, d.seed, d.counter_dev) == \
        (_lib.RS_SQUASH, 0, _lib.OUT_F64, B, mean.data_ptr(), 2, ls.data_ptr(), 2, 5, cnt.data_ptr())
    assert (d.act_dev, d.logp_dev, d.noise_dev) == (res.actions.data_ptr(), res.log_prob.data_ptr(), res.noise.data_ptr())
    assert res.actions.shape == (B,) and res.actions.dtype == torch.float64 and res.noise.dtype == torch.float64 and d.grad_mean_dev is None
    eng._L.calls.clear()
    res = eng.rsample(mean, ls, None, deterministic=True, out=(torch.zeros(B, 1, dtype=torch.float64), None, None))
    d = eng._L.calls[0][1][1]._obj
    assert (d.flags, d.counter_dev, d.logp_dev, d.noise_dev) == (_lib.RS_DETERMINISTIC, None, None, None) and res.log_prob is None
    eng._L.calls.clear()
    g = eng.rsample_backward(mean, ls, torch.zeros(B, dtype=torch.float64), None, torch.zeros(B, 1, dtype=torch.float64), out=(wide[:, 0], wide[:, 1]))
    assert [c[0] for c in eng._L.calls] == ["ptg_rsample_backward"]
    d = eng._L.calls[0][1][1]._obj
    assert (d.kind, d.grad_act_dev, d.grad_mean_dev, d.gm_s_n, d.grad_log_std_dev, d.gl_s_n) == (_lib.RS_SQUASH, None, wide.data_ptr(), 2, wide[:, 1].data_ptr(), 2)
    assert d.grad_logp_dev is not None and d.noise_dev is not None and g.grad_mean.data_ptr() == wide.data_ptr()
    eng._L.calls.clear()
    a = eng.smooth_target_action(ls.float().contiguous(), cnt, 0.2, 0.5, clip=(-0.5, 0.75), seed=9)
    d = eng._L.calls[0][1][1]._obj
    assert eng._L.calls[0][0] == "ptg_rsample" and a.shape == (B, 1) and a.dtype == torch.float32
    assert (d.kind, d.q_dtype, d.noise_std, d.noise_clip, d.clip_lo, d.clip_hi, d.seed, d.log_std_dev, d.logp_dev) == (_lib.RS_SMOOTH, _lib.OUT_F32, 0.2, 0.5, -0.5, 0.75, 9, None, None)
    # the losses
    lp = torch.zeros(B, 1)
    a64 = torch.zeros(1, dtype=torch.float64)
    both = torch.zeros(B, 2)
    eng._L.calls.clear()
    r = eng.actor_loss("sac", [both[:, 0], both[:, 1]], lp, log_ent_coef=a64, target_entropy=-1.0)
    assert [c[0] for c in eng._L.calls] == ["ptg_actor_loss_workspace", "ptg_actor_loss"] and eng._L.calls[0][1] == (B,)
    d = eng._L.calls[1][1][1]._obj
    assert (d.kind, d.flags, d.n_critics, d.n_quantiles, d.q_dtype, d.batch) == (_lib.AL_MIN, 7, 2, 1, _lib.OUT_F32, B)
    assert list(d.q_dev)[:3] == [both.data_ptr(), both[:, 1].data_ptr(), None] and list(d.q_s_n)[:2] == [2, 2] and list(d.g_s_n)[:2] == [1, 1]
    assert (d.logp_dev, d.alpha_dev, d.alpha, d.target_entropy) == (lp.data_ptr(), a64.data_ptr(), 0.0, -1.0)
    assert (d.grad_logp_dev, d.grad_log_alpha_dev, d.stats_dev) == (r.grad_log_prob.data_ptr(), r.grad_log_ent_coef.data_ptr(), r.stats.data_ptr())
    assert r.grad_log_prob.shape == (B, 1) and [g.shape for g in r.grad_q] == [(B,), (B,)] and r.grad_log_ent_coef.dtype == torch.float64
    eng._L.calls.clear()
    quant = torch.zeros(B, 2, 31)[:, :, :30]
    r = eng.actor_loss("tqc", quant, lp, ent_coef=0.00047)
    d = eng._L.calls[1][1][1]._obj
    assert (d.kind, d.flags, d.n_critics, d.n_quantiles, d.alpha, d.alpha_dev) == (_lib.AL_MEAN, _lib.AL_ENTROPY, 2, 30, 0.00047, None)
    assert list(d.q_dev)[:2] == [quant.data_ptr(), quant[:, 1].data_ptr()] and list(d.q_s_n)[:2] == [62, 62] and list(d.g_s_n)[:2] == [60, 60]
    assert r.grad_q.shape == (B, 2, 30) and r.grad_log_ent_coef is None and d.grad_log_alpha_dev is None
    eng._L.calls.clear()
    r = eng.actor_loss("td3", both[:, 1:])
    d = eng._L.calls[1][1][1]._obj
    assert (d.kind, d.flags, d.n_critics, d.n_quantiles, d.logp_dev, d.grad_logp_dev) == (_lib.AL_MEAN, 0, 1, 1, None, None)
    assert d.q_s_n[0] == 2 and r.grad_q.shape == (B, 1) and r.grad_log_prob is None
    eng._L.calls.clear()
    ws = torch.zeros(4096, dtype=torch.uint8)
    out = (torch.zeros(8, dtype=torch.float64), None, None, a64.clone())
    r = eng.actor_loss("ent_coef", log_prob=lp.double(), log_ent_coef=a64, target_entropy=-1.0, out=out, workspace=ws)
    d = eng._L.calls[1][1][1]._obj
    assert (d.kind, d.flags, d.n_critics, d.q_dtype, d.ws_dev, d.grad_log_alpha_dev) == (_lib.AL_ALPHA_ONLY, 6, 0, _lib.OUT_F64, ws.data_ptr(), out[3].data_ptr())
    assert r.stats is out[0] and r.grad_q is None and r.grad_log_prob is None
