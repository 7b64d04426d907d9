"""The NumPy restatement of ptg_quantile_loss (tests/quantile_loss_restatement.py) pinned against torch CPU autograd of sb3_contrib's
own lines (typed out in float64, cum_prob in float64: neither stable_baselines3 nor sb3_contrib is needed) and by hand, the planted
rows of the GPU tests vetted, and the parts of the call that need no device: the exported symbols, the struct's layout, the workspace
size, the Python argument checks and what reaches the library.
Bounds: statistics within 1e-12 * max(1, |ref|); n * gradient within 1e-12 * max(1, max |n * ref|); y equal to the last bit.
Measured here: the largest error is 0.0066 of its tolerance, at (K, Q, d) = (4, 64, 0) and B = 290."""
import ctypes as C
import os

import numpy as np
import pytest

import quantile_loss_restatement as qr
from rl_ptg_amd.train_ops import QuantileLoss             # needs no device and no library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_BS = [1, 2, 5, 65, 290]


def _close(got, ref, scale_by=1.0):
    """max |got - ref| * scale_by in units of 1e-12 * max(1, max |ref * scale_by|)"""
    got, ref = np.asarray(got, np.float64) * scale_by, np.asarray(ref, np.float64) * scale_by
    assert got.shape == ref.shape and np.isfinite(ref).all()
    return float(np.abs(got - ref).max() / (1e-12 * max(1.0, float(np.abs(ref).max()))))


def _stat(got, ref):
    return abs(got - ref) / (1e-12 * max(1.0, abs(ref)))


def _against_torch(c, drop, alpha):
    """-> the largest error in units of its tolerance; y and stats[4] must be exact"""
    B, K, Q = c["quantiles"].shape
    M = K * (Q - drop)
    n = float(B * K * Q * M)
    loss, grad, y = qr.sb3_tqc_lines(c, qr.GAMMA, alpha, drop)
    got = qr.quantile_loss(c["quantiles"], c["next_quantiles"], c["rewards"], c["dones"], c["next_log_prob"], qr.GAMMA, drop, alpha)
    assert not got["bad"].any() and got["y"].shape == (B, M)
    assert np.array_equal(got["y"].view(np.int64), y.view(np.int64))                    # the targets: equal to the last bit
    dl = y[:, None, None, :] - qr.stack(c["quantiles"])[:, :, :, None]
    e = [_stat(got["stats"][0], loss), _stat(got["stats"][1], qr.stack(c["quantiles"]).mean()), _stat(got["stats"][2], y.mean()),
         _stat(got["stats"][3], np.abs(dl).mean()), _close(got["grad"], grad, n)]
    assert got["stats"][4] == (np.abs(dl) > 1).sum() / n and got["stats"][5] == alpha and (got["stats"][6:] == 0).all()
    return max(e), e


@pytest.mark.parametrize("B", HOST_BS)
@pytest.mark.parametrize("shape", qr.SHAPES, ids=lambda s: "K%d-Q%d-d%d" % s)
def test_restatement_against_torch_autograd(B, shape):
    """every shape at the reference's gamma = 0.9639 and alpha = 0.00047, the planted rows included (a NaN and a +Inf among the dropped
    tops from B = 65 on); the reference's own shape also with alpha = 0.2"""
    K, Q, drop = shape
    c = qr.case(B, K, Q, drop, np.float64, rdt=np.float64, ddt=np.float64)
    worst, e = _against_torch(c, drop, qr.ALPHA)
    assert worst <= 1.0, e
    if shape == (2, 30, 2):
        w2, e = _against_torch(c, drop, 0.2)
        assert w2 <= 1.0, e
        worst = max(worst, w2)
    print(f"quantile loss B={B} K={K} Q={Q} d={drop}: max error / tolerance {worst:.4f}")


def test_one_row_by_hand():
    """B = 1, K = 1, Q = 2, d = 0, gamma 0.5, alpha 0.5: next quantiles (2, 1) sort to (1, 2); lp = -1 gives t = (1.5, 2.5) and, with
    r = 0.25, y = (1, 1.5).  tau = (0.25, 0.75).  theta = 1: delta = (0, 0.5), w = 0.25 twice, h = (0, 0.125), c = (0, 0.5): acc = 0.125,
    ls = 0.03125.  theta = 3: delta = (-2, -1.5), w = |0.75 - 1| = 0.25 twice, h = (1.5, 1), c = (-1, -1): acc = -0.5, ls = 0.625.  n = 4"""
    r = qr.quantile_loss([[[1.0, 3.0]]], [[[2.0, 1.0]]], [0.25], [0.0], [-1.0], 0.5, 0, 0.5)
    assert np.array_equal(r["y"], [[1.0, 1.5]]) and np.array_equal(r["grad"], [[[-0.03125, 0.125]]])
    assert np.array_equal(r["stats"], [0.1640625, 2.0, 1.25, 1.0, 0.5, 0.5, 0.0, 0.0])
    assert r["count"] == dict(loss=4.0, q=2.0, y=2.0, abs_delta=4.0) and not r["bad"].any()
    r = qr.quantile_loss([[[1.0, 3.0]]], [[[2.0, 1.0]]], [0.25], [0.0], [-1.0], 0.5, 1, 0.5)      # d = 1: only the lower one is kept
    assert np.array_equal(r["y"], [[1.0]]) and np.array_equal(r["grad"], [[[0.0, 0.125]]]) and r["stats"][0] == 0.1875


def test_the_planted_rows_are_what_they_say():
    """every case of tests/test_quantile_loss.py: delta exactly 0, -1, +1 and one spacing either side of |delta| = 1, on both branches of
    the Huber term; equal next quantiles across the critics; a NaN and a +Inf that the sort drops"""
    for dt in qr.DTYPES:
        eps, eps_lo = float(np.spacing(dt(1.5))), float(np.spacing(dt(0.5)))
        for K, Q, drop in qr.GPU_SHAPES:
            for B in (9, 290):
                c = qr.case(B, K, Q, drop, dt)
                r = qr.quantile_loss(c["quantiles"], c["next_quantiles"], c["rewards"], c["dones"], c["next_log_prob"], qr.GAMMA, drop, qr.ALPHA)
                M = K * (Q - drop)
                assert not r["bad"].any() and (r["y"][:6] == 0.5).all() and r["y"].shape == (B, M)
                dl = 0.5 - c["quantiles"][:6, 0, 0].astype(np.float64)
                assert dl.tolist() == [0.0, -1.0, 1.0, -1.0 - eps, -1.0 + eps, 1.0 + eps_lo]
                n, tau0 = float(B * K * Q * M), 0.5 / Q
                g = r["grad"][:6, 0, 0] * n / M                  # all M targets of the row are equal: M times one pair's w * c
                want = [0.0, (1 - tau0), -tau0, (1 - tau0), (1 - tau0) * (1.0 - eps), -tau0]
                assert np.allclose(g, want, rtol=1e-13, atol=0)
                assert c["dones"][6] == 0 and all(np.array_equal(c["next_quantiles"][6, k], c["next_quantiles"][6, 0]) for k in range(K))
                if K > 1:
                    s6 = np.sort(c["next_quantiles"][6].reshape(-1).astype(np.float64))
                    assert s6[0] == s6[K - 1] and np.array_equal(r["y"][6], c["rewards"][6].astype(np.float64)
                                                                  + ((1.0 - 0.0) * qr.GAMMA) * (s6[:M] - qr.ALPHA * float(c["next_log_prob"][6])))
                if drop > 0:
                    assert np.isnan(c["next_quantiles"][8]).sum() == 1 and np.isfinite(r["y"][8]).all() and np.isfinite(r["grad"][8]).all()
                    if B > 9:
                        assert np.isinf(c["next_quantiles"][9]).sum() == 1 and np.isfinite(r["y"][9]).all()
    import torch
    x = torch.tensor([1.0, float("nan"), float("inf"), -1.0, 1.0])
    assert torch.sort(x)[1].tolist()[:2] == [3, 0] and torch.isnan(torch.sort(x)[0][4]) and torch.sort(x)[0][3] == float("inf")
    assert np.isnan(np.sort(x.numpy())[4])                       # the order the restatement follows: a NaN ranks above +Inf


def test_bad_rows_of_the_restatement():
    c = qr.case(16, 2, 30, 2, np.float64)
    c["quantiles"][10, 1, 7] = np.nan
    c["rewards"][11] = np.inf
    c["next_quantiles"][12, 0, 3] = -np.inf                      # the lowest: it is kept
    c["next_quantiles"][13, 1, 5] = np.nan; c["next_quantiles"][13, 0, 5] = np.inf       # two tops of four dropped: legal
    c["next_quantiles"][14, :, 0] = np.nan; c["next_quantiles"][14, :, 1] = np.inf; c["next_quantiles"][14, 0, 2] = np.inf      # five: one is kept
    c["dones"][14] = 0.0
    run = lambda drop, alpha: qr.quantile_loss(c["quantiles"], c["next_quantiles"], c["rewards"], c["dones"], c["next_log_prob"], 0.96, drop, alpha)
    r = run(2, 0.2)
    assert np.nonzero(r["bad"])[0].tolist() == [10, 11, 12, 14] and np.isnan(r["stats"][:5]).all() and r["stats"][5] == 0.2
    assert np.isnan(r["grad"][[10, 11, 12, 14]]).all() and np.isfinite(r["grad"][~r["bad"]]).all() and (r["y"][11] == np.inf).all()
    assert np.isfinite(r["y"][13]).all() and r["y"][14, -1] == np.inf
    r = run(0, 0.2)                                              # nothing dropped: the planted NaN (row 8) and +Inf (row 9, 13) are kept
    assert np.nonzero(r["bad"])[0].tolist() == [8, 9, 10, 11, 12, 13, 14]
    r = run(2, np.nan)
    assert r["bad"].all() and np.isnan(r["stats"][:6]).all()


# ------------------------------------------------------------------------------------------------- the ABI, without a device
def test_the_library_exports_both_symbols_and_the_abi_stays_13():
    from rl_ptg_amd import _lib
    _lib.build()
    L = _lib.lib()
    assert hasattr(L, "ptg_quantile_loss") and hasattr(L, "ptg_quantile_loss_workspace")
    assert "ptg_quantile_loss" in _lib.EXPORTS and "ptg_quantile_loss_workspace" in _lib.EXPORTS
    assert L.ptg_abi_version() == 13
    assert (_lib.QL_LOG_ALPHA, _lib.QL_MAX_QUANTILES, _lib.TD_MAX_CRITICS) == (1, 64, 4)
    hdr = open(os.path.join(ROOT, "include", "ptg_env.h")).read()
    assert "PTG_QL_LOG_ALPHA = 1" in hdr and "#define PTG_QL_MAX_QUANTILES 64" in hdr and "left free for the quantile" not in hdr


def test_ptg_ql_layout_matches_the_c_compiler(tmp_path):
    import subprocess
    from rl_ptg_amd import _lib
    fields = ["flags", "n_critics", "n_quantiles", "n_drop", "q_dtype", "rew_dtype", "done_dtype", "batch", "cur_dev", "cur_s_n", "next_dev", "next_s_n",
              "grad_dev", "g_s_n", "rew_dev", "done_dev", "next_logp_dev", "alpha_dev", "gamma", "alpha", "stats_dev", "y_dev", "ws_dev"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu", sizeof(ptg_ql));\n%s\nprintf("\\n");return 0;}\n'
                   % (os.path.join(ROOT, "include", "ptg_env.h"), "\n".join('printf(" %%zu", offsetof(ptg_ql, %s));' % f for f in fields)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S = _lib.PtgQl
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]


def test_the_workspace_size_and_the_null_handle():
    from rl_ptg_amd import _lib
    L = _lib.lib()
    assert L.ptg_quantile_loss_workspace(0) < 0 and L.ptg_quantile_loss_workspace(-5) < 0
    assert L.ptg_quantile_loss_workspace(1) == L.ptg_quantile_loss_workspace(4) == 64
    assert L.ptg_quantile_loss_workspace(5) == 128 and L.ptg_quantile_loss_workspace(290) == 73 * 64 and L.ptg_quantile_loss_workspace(1029) == 258 * 64
    assert L.ptg_quantile_loss_workspace(2 ** 31) == 2 ** 29 * 64 and L.ptg_quantile_loss_workspace(2 ** 31 + 1) < 0 and L.ptg_quantile_loss_workspace(2 ** 40) < 0
    assert L.ptg_quantile_loss(None, C.byref(_lib.PtgQl()), None) == _lib.E_INVALID


# ------------------------------------------------------------------------------------------------- the Python argument checks
def test_python_argument_checks_need_no_device():
    import torch
    from helpers import host_engine
    eng = host_engine(4)
    B, K, Q = 6, 2, 5
    q, col = torch.zeros(B, K, Q), torch.zeros(B)
    ql = [torch.zeros(B, Q), torch.zeros(B, Q)]
    a64 = torch.zeros(1, dtype=torch.float64)
    other = torch.device("meta")

    def run(**kw):
        a = dict(quantiles=q, next_quantiles=q, rewards=col, dones=col, next_log_prob=col, gamma=0.96, top_quantiles_to_drop_per_net=2, ent_coef=0.2)
        a.update(kw)
        pos = [a.pop(k) for k in ("quantiles", "next_quantiles", "rewards", "dones", "next_log_prob", "gamma", "top_quantiles_to_drop_per_net")]
        return eng.quantile_loss(*pos, **a)

    lst = lambda **kw: run(**dict(dict(quantiles=ql, next_quantiles=ql), **kw))
    out = (torch.zeros(8, dtype=torch.float64), torch.zeros(B, K, Q), None)
    outl = (torch.zeros(8, dtype=torch.float64), [torch.zeros(B, Q), torch.zeros(B, Q)], torch.zeros(B, K * (Q - 2)))
    refused = [
        # the quantiles: what they are, then their shape, strides and device
        (TypeError, lambda: run(quantiles=q.numpy())), (TypeError, lambda: run(quantiles=q.half())), (TypeError, lambda: run(quantiles=q.long())), (TypeError, lambda: run(quantiles=None)),
        (TypeError, lambda: run(quantiles=torch.zeros(B, 9, Q, dtype=torch.int32))),                 # dtype and K both wrong: the TypeError comes first
        (ValueError, lambda: run(quantiles=torch.zeros(B, Q))), (ValueError, lambda: run(quantiles=torch.zeros(B, 5, Q), next_quantiles=torch.zeros(B, 5, Q))),
        (ValueError, lambda: run(quantiles=torch.zeros(B, K, 65), next_quantiles=torch.zeros(B, K, 65))), (ValueError, lambda: run(quantiles=torch.zeros(B, 0, Q), next_quantiles=torch.zeros(B, 0, Q))),
        (ValueError, lambda: run(quantiles=torch.zeros(B, Q, K).transpose(1, 2))), (ValueError, lambda: run(quantiles=torch.zeros(1, K, Q).expand(B, K, Q))),
        (ValueError, lambda: run(quantiles=torch.zeros(B, K, Q, device=other))),
        (ValueError, lambda: run(quantiles=q[:0], next_quantiles=q[:0], rewards=col[:0], dones=col[:0], next_log_prob=col[:0])),
        (TypeError, lambda: run(next_quantiles=q.double())), (TypeError, lambda: run(next_quantiles=None)), (ValueError, lambda: run(next_quantiles=torch.zeros(B, K, Q + 1))),
        (ValueError, lambda: run(next_quantiles=torch.zeros(B + 1, K, Q))), (ValueError, lambda: run(next_quantiles=torch.zeros(B, K + 1, Q))), (ValueError, lambda: run(next_quantiles=ql[:1])),
        (TypeError, lambda: run(next_quantiles=torch.zeros(B + 1, K, Q, dtype=torch.float64))),
        # the lists
        (ValueError, lambda: lst(quantiles=[])), (ValueError, lambda: lst(quantiles=ql * 3)), (ValueError, lambda: lst(next_quantiles=ql * 2)), (TypeError, lambda: lst(quantiles=[ql[0], None])),
        (TypeError, lambda: lst(quantiles=[ql[0], ql[1].double()])), (TypeError, lambda: lst(quantiles=[ql[0].half(), ql[1]])), (ValueError, lambda: lst(quantiles=[ql[0], torch.zeros(B, Q + 1)])),
        (ValueError, lambda: lst(quantiles=[ql[0], torch.zeros(B + 1, Q)])), (ValueError, lambda: lst(quantiles=[ql[0], torch.zeros(Q, B).t()])), (ValueError, lambda: lst(quantiles=[ql[0], torch.zeros(B)])),
        (TypeError, lambda: lst(next_quantiles=[ql[0], ql[1].double()])), (ValueError, lambda: lst(next_quantiles=[ql[0], torch.zeros(B, Q, device=other)])),
        # rewards, dones, next_log_prob
        (TypeError, lambda: run(rewards=col.half())), (TypeError, lambda: run(rewards=None)), (TypeError, lambda: run(dones=col.bool())), (ValueError, lambda: run(rewards=torch.zeros(B + 1))),
        (ValueError, lambda: run(rewards=torch.zeros(2 * B)[::2])), (ValueError, lambda: run(dones=torch.zeros(B, 2))), (ValueError, lambda: run(dones=torch.zeros(B, device=other))),
        (TypeError, lambda: run(next_log_prob=col.double())), (TypeError, lambda: run(next_log_prob=None)), (ValueError, lambda: run(next_log_prob=torch.zeros(B + 1))),
        (ValueError, lambda: run(next_log_prob=torch.zeros(2 * B)[::2])),
        # the scalars and the coefficients
        (TypeError, lambda: run(top_quantiles_to_drop_per_net=2.0)), (TypeError, lambda: run(top_quantiles_to_drop_per_net=True)), (TypeError, lambda: run(top_quantiles_to_drop_per_net=None)),
        (ValueError, lambda: run(top_quantiles_to_drop_per_net=-1)), (ValueError, lambda: run(top_quantiles_to_drop_per_net=Q)),
        (ValueError, lambda: run(gamma=float("nan"))), (ValueError, lambda: run(gamma=float("inf"))),
        (ValueError, lambda: run(ent_coef=None)), (ValueError, lambda: run(log_ent_coef=a64)), (TypeError, lambda: run(ent_coef=torch.zeros(1))),
        (TypeError, lambda: run(ent_coef=torch.zeros(2, dtype=torch.float64))), (TypeError, lambda: run(ent_coef=None, log_ent_coef=0.0)), (TypeError, lambda: run(ent_coef=None, log_ent_coef=torch.zeros(1))),
        (ValueError, lambda: run(ent_coef=torch.zeros(1, dtype=torch.float64, device=other))),
        # out and workspace: ValueError throughout, their dtypes are set by the inputs
        (ValueError, lambda: run(out=out[:2])), (ValueError, lambda: run(out=list(out))), (ValueError, lambda: run(out=(out[0].float(), out[1], None))), (ValueError, lambda: run(out=(out[0][:7], out[1], None))),
        (ValueError, lambda: run(out=(out[0], out[1].double(), None))), (ValueError, lambda: run(out=(out[0], out[1][:, :, :4], None))), (ValueError, lambda: run(out=(out[0], outl[1], None))),
        (ValueError, lambda: lst(out=(outl[0], out[1], None))), (ValueError, lambda: run(out=(out[0], None, None))), (ValueError, lambda: run(out=out, want_target=True)),
        (ValueError, lambda: run(out=(out[0], out[1], torch.zeros(B, K * Q)))), (ValueError, lambda: run(out=(out[0], out[1], torch.zeros(B, K * (Q - 2), dtype=torch.float64)))),
        (ValueError, lambda: lst(out=(outl[0], outl[1][:1], None))), (ValueError, lambda: lst(out=(outl[0], [outl[1][0], torch.zeros(B, Q + 1)], None))),
        (ValueError, lambda: lst(out=(outl[0], [outl[1][0], outl[1][0]], None))), (ValueError, lambda: lst(out=(outl[0], [outl[1][0], ql[1]], None))),      # a tensor given twice
        (ValueError, lambda: run(out=(out[0], q, None))),
        (ValueError, lambda: run(out=out, workspace=torch.zeros(4096))), (ValueError, lambda: run(out=out, workspace=torch.zeros(4096, dtype=torch.uint8, device=other))),
        (ValueError, lambda: run(out=out, workspace=torch.zeros(8192, dtype=torch.uint8)[::2])),
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
    B, K, Q, drop = 290, 2, 30, 2
    M = K * (Q - drop)
    q, nq = torch.zeros(B, K, Q, dtype=torch.float64), torch.zeros(B, K, Q, dtype=torch.float64)
    rew, done, lp = torch.zeros(B, 1, dtype=torch.float64), torch.zeros(B, 1), torch.zeros(B, dtype=torch.float64)
    with pytest.raises(ValueError):
        eng.quantile_loss(q, nq, rew, done, lp, float("nan"), drop, ent_coef=0.1)
    with pytest.raises(TypeError):
        eng.quantile_loss(q, nq, rew, done.bool(), lp, 0.96, drop, ent_coef=0.1)
    with pytest.raises(ValueError):
        eng.quantile_loss(q, nq, rew, done, lp, 0.96, drop, ent_coef=0.1, workspace=torch.zeros(10))
    assert eng._L.calls == []
    # SB3's stacked [B, K, Q] tensors, [B, 1] columns of a replay sample, float64 rewards beside float32 dones, the targets asked for
    res = eng.quantile_loss(q, nq, rew, done, lp, qr.GAMMA, drop, ent_coef=qr.ALPHA, want_target=True)
    assert isinstance(res, QuantileLoss)
    assert [c[0] for c in eng._L.calls] == ["ptg_quantile_loss_workspace", "ptg_quantile_loss"] and eng._L.calls[0][1] == (B,)
    h, ref, stream = eng._L.calls[1][1]
    d = ref._obj
    assert h == "H" and stream is None
    assert (d.flags, d.n_critics, d.n_quantiles, d.n_drop, d.q_dtype, d.rew_dtype, d.done_dtype, d.batch) == (0, K, Q, drop, _lib.OUT_F64, _lib.OUT_F64, _lib.OUT_F32, B)
    assert list(d.cur_dev) == [q.data_ptr(), q.data_ptr() + 8 * Q, None, None] and list(d.cur_s_n)[:2] == [K * Q, K * Q]
    assert list(d.next_dev)[:3] == [nq.data_ptr(), nq.data_ptr() + 8 * Q, None] and list(d.next_s_n)[:2] == [K * Q, K * Q]
    assert list(d.grad_dev)[:3] == [res.grad_quantiles.data_ptr(), res.grad_quantiles.data_ptr() + 8 * Q, None] and list(d.g_s_n)[:2] == [K * Q, K * Q]
    assert (d.rew_dev, d.done_dev, d.next_logp_dev, d.alpha_dev) == (rew.data_ptr(), done.data_ptr(), lp.data_ptr(), None)
    assert (d.gamma, d.alpha) == (qr.GAMMA, qr.ALPHA) and (d.stats_dev, d.y_dev) == (res.stats.data_ptr(), res.target.data_ptr())
    assert res.grad_quantiles.shape == (B, K, Q) and res.grad_quantiles.dtype == torch.float64 and res.target.shape == (B, M) and res.stats.shape == (8,)
    # a list of K [B, Q] tensors, one of them a column slice of a wider tensor (row stride Q + 1), preallocated outputs
    eng._L.calls.clear()
    wide = torch.zeros(B, Q + 1)
    qs, nqs = [wide[:, :Q], torch.zeros(B, Q)], [torch.zeros(B, Q), torch.zeros(B, Q)]
    gw = torch.zeros(B, Q + 1)
    out = (torch.zeros(8, dtype=torch.float64), [torch.zeros(B, Q), gw[:, :Q]], None)
    ws = torch.zeros(8192, dtype=torch.uint8)
    a64 = torch.zeros(1, dtype=torch.float64)
    res = eng.quantile_loss(qs, nqs, rew.float(), done, lp.float(), 0.99, 0, log_ent_coef=a64, out=out, workspace=ws)
    assert [c[0] for c in eng._L.calls] == ["ptg_quantile_loss_workspace", "ptg_quantile_loss"]      # the size query of the workspace check
    d = eng._L.calls[1][1][1]._obj
    assert (d.flags, d.n_critics, d.n_quantiles, d.n_drop, d.q_dtype, d.rew_dtype, d.batch) == (_lib.QL_LOG_ALPHA, 2, Q, 0, _lib.OUT_F32, _lib.OUT_F32, B)
    assert list(d.cur_dev)[:3] == [qs[0].data_ptr(), qs[1].data_ptr(), None] and list(d.cur_s_n)[:2] == [Q + 1, Q] and list(d.next_s_n)[:2] == [Q, Q]
    assert list(d.grad_dev)[:2] == [out[1][0].data_ptr(), gw.data_ptr()] and list(d.g_s_n)[:2] == [Q, Q + 1]
    assert d.ws_dev == ws.data_ptr() and d.y_dev is None and (d.alpha, d.alpha_dev) == (0.0, a64.data_ptr())
    assert res.stats is out[0] and res.grad_quantiles is out[1] and res.target is None
    # a device alpha; one row (any stride is lifted to Q)
    eng._L.calls.clear()
    res = eng.quantile_loss(q[:1], nq[:1], rew[:1], done[:1], lp[:1], 0.9, 29, ent_coef=a64)
    d = eng._L.calls[1][1][1]._obj
    assert (d.flags, d.batch, d.n_drop, d.alpha, d.alpha_dev) == (0, 1, 29, 0.0, a64.data_ptr()) and res.target is None
