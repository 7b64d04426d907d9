"""The NumPy restatement of ptg_policy_loss (tests/policy_loss_restatement.py) pinned against torch CPU autograd of SB3's own lines
and by hand, the inputs of the GPU tests vetted (no PPO ratio near a clip edge, where the gradient jumps), and the parts of the call
that need no device: the exported symbols, the ABI version, the struct's size, the workspace size, the Python argument checks."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import policy_loss_restatement as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN2 = math.log(2.0)


def _close(got, ref, scale_by=1.0):
    """max |got - ref| * scale_by in units of 1e-12 * max(1, max |ref * scale_by|)"""
    got, ref = np.asarray(got, np.float64) * scale_by, np.asarray(ref, np.float64) * scale_by
    assert got.shape == ref.shape and np.isfinite(ref).all()
    return float(np.abs(got - ref).max() / (1e-12 * max(1.0, float(np.abs(ref).max()))))


@pytest.mark.parametrize("B", [2, 65, 203])
@pytest.mark.parametrize("A", [2, 5, 32])
def test_restatement_against_torch_autograd_categorical(B, A):
    """both kinds x value clipping on / off x normalisation on / off; statistics within 1e-12 * max(1, |ref|), B * gradient within
    1e-12 * max(1, max |B * ref|)"""
    c = pr.case(B, A, np.float64)
    worst = 0.0
    for kind in ("ppo", "a2c"):
        for cvf in (None, pr.CLIP_VF):
            for norm in (False, True):
                kw = dict(clip_range=pr.CLIP, clip_range_vf=cvf, ent_coef=pr.ENT_COEF, vf_coef=pr.VF_COEF, normalize_advantage=norm)
                ref = pr.torch_reference(kind, c, **kw)
                got = pr.policy_loss(kind, c["logits"], c["values"], c["actions"], c["old_log_prob"], c["advantages"], c["returns"],
                                     old_values=c["old_values"], **kw)
                assert not got["bad"].any() and not got["oob"].any()
                e = [max(abs(got["stats"][k] - ref["stats"][k]) / (1e-12 * max(1.0, abs(ref["stats"][k]))) for k in range(5)),
                     _close(got["grad_input"], ref["grad_input"], B), _close(got["grad_values"], ref["grad_values"], B)]
                assert got["stats"][5] == ref["stats"][5]                          # clip_fraction: a count over B
                worst = max(worst, *e)
                assert max(e) <= 1.0, (kind, cvf, norm, e)
    print(f"B={B} A={A}: max error / tolerance {worst:.4f}")


@pytest.mark.parametrize("B", [2, 65, 203])
def test_restatement_against_torch_autograd_gaussian(B):
    c = pr.gaussian_case(B, np.float64)
    for kind in ("ppo", "a2c"):
        for cvf in (None, pr.CLIP_VF):
            for norm in (False, True):
                kw = dict(clip_range=pr.CLIP, clip_range_vf=cvf, ent_coef=pr.ENT_COEF, vf_coef=pr.VF_COEF, normalize_advantage=norm)
                ref = pr.torch_reference(kind, c, **kw)
                got = pr.policy_loss(kind, c["mean"], c["values"], c["actions"], c["old_log_prob"], c["advantages"], c["returns"],
                                     old_values=c["old_values"], log_std=c["log_std"], **kw)
                e = [max(abs(got["stats"][k] - ref["stats"][k]) / (1e-12 * max(1.0, abs(ref["stats"][k]))) for k in range(5)),
                     _close(got["grad_input"], ref["grad_input"], B), _close(got["grad_values"], ref["grad_values"], B),
                     _close([got["grad_log_std"]], ref["grad_log_std"])]
                assert got["stats"][5] == ref["stats"][5] and max(e) <= 1.0, (kind, cvf, norm, e)


def test_two_rows_by_hand():
    """logits (0, 0) twice: lp = -ln 2, H = ln 2, p = 1/2.  A2C, advantages (1, -3) as they are, values (0.5, 2), returns (1, 1),
    ent_coef 0.5, vf_coef 0.25"""
    x, act = np.zeros((2, 2)), np.array([0, 1])
    adv, v, ret = np.array([1.0, -3.0]), np.array([0.5, 2.0]), np.array([1.0, 1.0])
    r = pr.policy_loss("a2c", x, v, act, None, adv, ret, ent_coef=0.5, vf_coef=0.25)
    assert np.allclose(r["stats"][:6], [-1.5 * LN2 + 0.15625, -LN2, 0.625, -LN2, 0.0, 0.0], rtol=0, atol=1e-15)
    assert r["stats"][6] == 0.0 and r["stats"][7] == 1.0
    assert np.allclose(r["grad_input"], [[-0.25, 0.25], [-0.75, 0.75]], rtol=0, atol=1e-16)
    assert np.array_equal(r["grad_values"], [-0.125, 0.25])
    assert r["abs_mean"]["policy_loss"] == 2 * LN2 and r["abs_mean"]["value_loss"] == 0.625 and r["margin"] == np.inf
    # PPO, eps 0.2: row 0 has ratio 1.5 and advantage 1 -- clipped, surrogate 1.2, no gradient; row 1 has ratio exactly 1
    old = np.array([-LN2 - math.log(1.5), -LN2])
    r = pr.policy_loss("ppo", x, v, act, old, adv, ret, clip_range=0.2, ent_coef=0.0, vf_coef=0.25, normalize_advantage=False)
    assert abs(r["stats"][1] - 0.9) < 1e-15 and r["stats"][5] == 0.5 and abs(r["stats"][4] - (0.5 - math.log(1.5)) / 2) < 1e-15
    assert np.array_equal(r["grad_input"][0], [0.0, 0.0]) and np.allclose(r["grad_input"][1], [-0.75, 0.75], rtol=0, atol=1e-16)
    assert r["ratio"][1] == 1.0 and abs(r["margin"] - 0.2) < 1e-15
    # normalised: mean -1, unbiased std sqrt(8) -> advantages +-(2 / (sqrt(8) + 1e-8))
    r = pr.policy_loss("a2c", x, v, act, None, adv, ret, normalize_advantage=True)
    assert r["stats"][6] == -1.0 and r["stats"][7] == math.sqrt(8.0)
    ah = 2.0 / (math.sqrt(8.0) + 1e-8)
    assert np.allclose(r["grad_input"], [[-ah / 4, ah / 4], [-ah / 4, ah / 4]], rtol=0, atol=1e-16)


def test_a_batch_of_one_is_not_normalised():
    """SB3 skips the normalisation for one row (its std would be NaN): the advantage is used as it is"""
    c = pr.case(1, 5, np.float64)
    args = (c["logits"], c["values"], c["actions"], c["old_log_prob"], c["advantages"], c["returns"])
    a = pr.policy_loss("ppo", *args, clip_range=0.2, normalize_advantage=True)
    b = pr.policy_loss("ppo", *args, clip_range=0.2, normalize_advantage=False)
    assert np.isfinite(a["stats"]).all() and np.array_equal(a["stats"], b["stats"]) and np.array_equal(a["grad_input"], b["grad_input"])
    assert a["stats"][6] == 0.0 and a["stats"][7] == 1.0
    ref = pr.torch_reference("ppo", c, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True)
    assert _close(a["grad_input"], ref["grad_input"]) <= 1.0 and abs(a["stats"][0] - ref["stats"][0]) <= 1e-12


def test_bad_rows_of_the_restatement():
    c = pr.case(16, 5, np.float64)
    c["logits"][5, 2] = np.nan; c["logits"][6] = -np.inf; c["values"][7] = np.inf; c["actions"][8] = 5; c["actions"][9] = -1
    c["logits"][10, c["actions"][10]] = -np.inf                                      # an action of probability 0
    c["old_log_prob"][11] = -1e30; c["advantages"][11] = 0.0                         # a ratio that overflows: 0 * Inf
    c["old_log_prob"][12] = -1e30
    r = pr.policy_loss("ppo", c["logits"], c["values"], c["actions"], c["old_log_prob"], c["advantages"], c["returns"], clip_range=0.2,
                       normalize_advantage=False)
    assert np.nonzero(r["bad"])[0].tolist() == [5, 6, 7, 10, 11, 12] and np.nonzero(r["oob"])[0].tolist() == [8, 9]
    assert np.isnan(r["stats"][:6]).all() and np.isnan(r["grad_input"][[5, 6, 7, 10, 11, 12]]).all() and np.isnan(r["grad_values"][[5, 6, 7, 10, 11, 12]]).all()
    good = [k for k in range(16) if k not in (5, 6, 7, 8, 9, 10, 11, 12)]
    assert np.isfinite(r["grad_input"][good]).all() and np.isfinite(r["grad_values"][good]).all()


def test_the_gpu_inputs_keep_every_ratio_away_from_the_clip_edges():
    """every case tests/test_policy_loss.py runs PPO on: no ratio within 1e-9 of 1 - eps or 1 + eps, where the gradient jumps and a
    last-place difference in exp could move a row; the planted row 4 has ratio exactly 1; every planted row is what it says"""
    cases = [(B, A, dt) for B in pr.BS for A in pr.AS for dt in pr.DTYPES] + [(pr.B_BIG, 5, np.float32), (pr.B_BIG, 5, np.float64)]
    for B, A, dt in cases:
        c = pr.case(B, A, dt)
        for norm in (False, True):
            r = pr.policy_loss("ppo", c["logits"], c["values"], c["actions"], c["old_log_prob"], c["advantages"], c["returns"], clip_range=pr.CLIP,
                               clip_range_vf=pr.CLIP_VF, old_values=c["old_values"], ent_coef=pr.ENT_COEF, normalize_advantage=norm)
            assert r["margin"] >= 1e-9 and not r["bad"].any() and not r["oob"].any() and np.isfinite(r["stats"]).all(), (B, A, dt)
        if B > 4:
            assert 4 in pr.ratio_one_rows(c) and r["ratio"][4] == 1.0
        if B > 11:
            rt, adv = r["ratio"], c["advantages"]
            assert rt[5] > 1.2 and rt[6] > 1.2 and rt[7] < 0.8 and rt[8] < 0.8 and adv[5] > 0 > adv[6] and adv[7] > 0 > adv[8] and adv[3] == 0
            dv = c["values"].astype(np.float64) - c["old_values"].astype(np.float64)
            assert abs(dv[9]) < pr.CLIP_VF and dv[10] > pr.CLIP_VF and dv[11] < -pr.CLIP_VF
            assert np.isinf(c["logits"][1]).sum() == 1 and (c["logits"][0] == c["logits"][0, 0]).all()
    for B in (203, 4097):
        c = pr.gaussian_case(B, np.float32)
        r = pr.policy_loss("ppo", c["mean"], c["values"], c["actions"], c["old_log_prob"], c["advantages"], c["returns"], clip_range=pr.CLIP,
                           log_std=c["log_std"])
        assert r["margin"] >= 1e-9 and not r["bad"].any()


# ------------------------------------------------------------------------------------------------- the ABI, without a device
def test_the_library_exports_both_symbols_at_abi_13():
    from rl_ptg_amd import _lib
    _lib.build()
    L = _lib.lib()
    assert hasattr(L, "ptg_policy_loss") and hasattr(L, "ptg_policy_loss_workspace")
    assert "ptg_policy_loss" in _lib.EXPORTS and "ptg_policy_loss_workspace" in _lib.EXPORTS
    assert L.ptg_abi_version() == 13
    assert (_lib.LOSS_PPO, _lib.LOSS_A2C, _lib.LOSS_NORM_ADV, _lib.LOSS_CLIP_VF) == (0, 1, 1, 2)
    hdr = open(os.path.join(ROOT, "include", "ptg_env.h")).read()
    assert "PTG_LOSS_PPO = 0, PTG_LOSS_A2C = 1" in hdr and "PTG_LOSS_NORM_ADV = 1, PTG_LOSS_CLIP_VF = 2" in hdr


def test_ptg_loss_size_matches_the_c_compiler(tmp_path):
    import subprocess
    from rl_ptg_amd import _lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu %%zu\\n", sizeof(ptg_loss), offsetof(ptg_loss, batch), '
                   'offsetof(ptg_loss, clip_range), offsetof(ptg_loss, g_s_n), offsetof(ptg_loss, ws_dev));return 0;}\n' % os.path.join(ROOT, "include", "ptg_env.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S = _lib.PtgLoss
    assert got == [C.sizeof(S), S.batch.offset, S.clip_range.offset, S.g_s_n.offset, S.ws_dev.offset]


def test_the_workspace_size_and_the_null_handle():
    from rl_ptg_amd import _lib
    L = _lib.lib()
    assert L.ptg_policy_loss_workspace(0) < 0 and L.ptg_policy_loss_workspace(-5) < 0
    assert L.ptg_policy_loss_workspace(1) == L.ptg_policy_loss_workspace(256) == 32 + 88
    assert L.ptg_policy_loss_workspace(257) == 32 + 2 * 88 and L.ptg_policy_loss_workspace(20 * 65536) == 32 + 5120 * 88
    assert L.ptg_policy_loss_workspace(2 ** 40) < 0 and L.ptg_policy_loss_workspace(2 ** 31 + 1) < 0
    assert L.ptg_policy_loss_workspace(2 ** 31) == 32 + 2 ** 23 * 88      # the largest batch: 2^23 blocks, half of a launch's 2^32 threads
    assert L.ptg_policy_loss(None, C.byref(_lib.PtgLoss()), None) == _lib.E_INVALID


def test_python_argument_checks_need_no_device():
    import torch
    from helpers import host_engine
    eng = host_engine(4)
    B, A = 6, 5
    x, v, act = torch.zeros(B, A), torch.zeros(B), torch.zeros(B, dtype=torch.int64)
    col = torch.zeros(B)
    other = torch.device("meta")
    base = dict(kind="ppo", x=x, v=v, act=act, old=col, adv=col, ret=col)

    def call(**kw):
        a = dict(base)
        for k in list(kw):
            if k in a:
                a[k] = kw.pop(k)
        kw.setdefault("clip_range", 0.2)
        return eng.policy_loss(a["kind"], a["x"], a["v"], a["act"], a["old"], a["adv"], a["ret"], **kw)

    out = (torch.zeros(8, dtype=torch.float64), torch.zeros(B, A), torch.zeros(B), None)
    refused = [
        (ValueError, lambda: call(kind="dqn")), (TypeError, lambda: call(x=x.half())), (TypeError, lambda: call(x=x.numpy())),
        (ValueError, lambda: call(x=x[:, :1])), (ValueError, lambda: call(x=torch.zeros(B, 33))), (ValueError, lambda: call(x=torch.zeros(B))),
        (ValueError, lambda: call(x=torch.zeros(A, B).t())), (ValueError, lambda: call(x=torch.zeros(1, A).expand(B, A))),
        (ValueError, lambda: call(x=torch.zeros(B, A, device=other))),
        (TypeError, lambda: call(act=act.float())), (TypeError, lambda: call(act=act.short())), (ValueError, lambda: call(act=act[:5])),
        (ValueError, lambda: call(act=torch.zeros(2 * B, dtype=torch.int64)[::2])),
        (TypeError, lambda: call(v=v.double())), (ValueError, lambda: call(v=torch.zeros(B + 1))), (ValueError, lambda: call(v=torch.zeros(B, 2))),
        (TypeError, lambda: call(adv=col.double())), (ValueError, lambda: call(ret=torch.zeros(2 * B)[::2])), (ValueError, lambda: call(old=None)),
        (TypeError, lambda: call(old=col.double())), (ValueError, lambda: call(adv=torch.zeros(B, device=other))),
        (ValueError, lambda: call(clip_range=None)), (ValueError, lambda: call(clip_range=-0.1)), (ValueError, lambda: call(clip_range=float("nan"))),
        (ValueError, lambda: call(clip_range_vf=0.2)), (ValueError, lambda: call(clip_range_vf=-1.0, old_values=col)),
        (TypeError, lambda: call(clip_range_vf=0.2, old_values=col.double())),
        (TypeError, lambda: call(x=v, log_std=0.0)), (TypeError, lambda: call(x=v, act=col, log_std=torch.zeros(2))),
        (TypeError, lambda: call(x=v, act=act, log_std=torch.zeros(1))), (ValueError, lambda: call(x=x, act=col, log_std=torch.zeros(1))),
        (ValueError, lambda: call(out=out[:3])), (ValueError, lambda: call(out=list(out))),
        (ValueError, lambda: call(out=(out[0].float(), out[1], out[2], None))), (ValueError, lambda: call(out=(out[0], out[1][:, :4], out[2], None))),
        (ValueError, lambda: call(out=(out[0], out[1], out[2].double(), None))), (ValueError, lambda: call(out=(out[0], out[1], out[2], torch.zeros(1)))),
        (ValueError, lambda: call(out=(out[0], torch.zeros(A, B).t(), out[2], None))),
        (ValueError, lambda: call(out=out, workspace=torch.zeros(4096))), (ValueError, lambda: call(out=out, workspace=torch.zeros(4096, dtype=torch.uint8, device=other))),
    ]
    for k, (exc, fn) in enumerate(refused):
        with pytest.raises(exc):
            fn()
        assert eng._L is None, k
