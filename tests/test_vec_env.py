"""The SB3-facing surface (rl_ptg_amd/vec_env.py) against the reference's golden trajectories: dict observations in the
declared spaces, float32 rewards, bool dones, Monitor / DummyVecEnv info conventions, numpy-seeded noise streams."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-11, 1e-13


def _flat(obs, order):
    return np.concatenate([np.asarray(obs[k], dtype=np.float64).reshape(len(np.atleast_1d(obs["METH_STATUS"])), -1) for k in order], axis=1)


@pytest.mark.parametrize("case", ["real_bs2_op2_mod_disc_train", "synth_bs2_op2_term_penalty", "real_bs1_op1_raw_cont_evalval"])
def test_vec_env_matches_reference_stack(case):
    from rl_ptg_amd.vec_env import INFO_KEYS, PtGVecEnv
    tr, kw = H.kwargs_from_fixture(case)
    meta = tr["meta"]
    n = meta["n_envs"]
    env = PtGVecEnv(kw, n, train_or_eval=meta["train_or_eval"], seed=meta["seed"], noise="numpy", noise_tape_len=64)
    order = H_ORDER[kw["raw_modified"]]
    # the numpy generators reproduce the normal draws the reference env consumed
    L = min(64, tr["noise"].shape[1])
    for e in range(n):
        m = min(L, int(tr["noise_len"][e]))
        assert np.array_equal(env._tape[e, :m], tr["noise"][e, :m])
    assert list(env.observation_space.spaces) == sorted(order)
    obs = env.reset()
    assert obs["METH_STATUS"].dtype == np.int64 and obs["T_CAT"].dtype == np.float64 and obs["T_CAT"].shape == (n, 1)
    np.testing.assert_allclose(_flat(obs, order), tr["reset_obs"], rtol=RTOL, atol=ATOL)
    # DummyVecEnv.reset keeps each env's reset info: the reference returns _get_info() there (env/ptg_gym_env.py:504)
    assert len(env.reset_infos) == n
    for e in range(n):
        assert list(env.reset_infos[e]) == list(INFO_KEYS)
        for q, k in enumerate(INFO_KEYS):
            if k != "Meth_Action":
                assert float(env.reset_infos[e][k]) == tr["reset_info"][e, q], (e, k)
    K = tr["actions"].shape[0]
    n_post = 0
    ret = np.zeros(n)
    for t in range(K):
        a = tr["actions"][t]
        obs, rew, done, infos = env.step(a.reshape(n, 1) if kw["action_type"] == "continuous" else a)
        assert rew.dtype == np.float32 and done.dtype == bool and len(infos) == n
        assert np.array_equal(done, tr["done"][t].astype(bool))
        H.assert_rewards(rew, tr["f64s"][t, :, 0], "float32", err_msg=f"reward step {t}")
        ret += tr["f64s"][t, :, 0]
        flat = _flat(obs, order)
        for e in range(n):
            if done[e]:
                np.testing.assert_allclose(flat[e], tr["post_reset_obs"][n_post], rtol=RTOL, atol=ATOL)
                term = infos[e]["terminal_observation"]
                np.testing.assert_allclose(_flat({k: np.asarray([v]) for k, v in term.items()}, order)[0], tr["obs"][t, e], rtol=RTOL, atol=ATOL)
                assert infos[e]["TimeLimit.truncated"] is False
                assert infos[e]["episode"]["l"] == int(tr["ints"][t, e, 8])
                assert abs(infos[e]["episode"]["r"] - ret[e]) < 1e-5
                ret[e] = 0.0
                n_post += 1
            else:
                np.testing.assert_allclose(flat[e], tr["obs"][t, e], rtol=RTOL, atol=ATOL, err_msg=f"step {t} env {e}")
        if meta["train_or_eval"] == "eval":
            for e in range(n):
                for q, k in enumerate(INFO_KEYS):
                    v = infos[e][k]
                    if k == "Meth_Action":
                        assert v == ["standby", "cooldown", "startup", "partial_load", "full_load"][int(tr["infos"][t, e, q])]
                    else:
                        assert abs(float(v) - tr["infos"][t, e, q]) <= 1e-11 * max(1.0, abs(tr["infos"][t, e, q])), (t, e, k)
        elif not done.any():
            assert infos == [{} for _ in range(n)]
    assert n_post == len(tr["post_reset_at"])
    env.close()


H_ORDER = {
    "mod": ["Pot_Reward", "Part_Full", "METH_STATUS", "T_CAT", "H2_in_MolarFlow", "CH4_syn_MolarFlow", "H2_res_MolarFlow",
            "H2O_DE_MassFlow", "Elec_Heating", "Temp_hour_enc_sin", "Temp_hour_enc_cos"],
    "raw": ["Elec_Price", "Gas_Price", "EUA_Price", "METH_STATUS", "T_CAT", "H2_in_MolarFlow", "CH4_syn_MolarFlow",
            "H2_res_MolarFlow", "H2O_DE_MassFlow", "Elec_Heating", "Temp_hour_enc_sin", "Temp_hour_enc_cos"],
}


def test_single_env_adapter_eval_mode():
    """PTGEnv(dict_input, 'eval'): reset(seed) / step() like the reference env object (config #1 of BASELINE.json: 1 env, BS2/OP2)."""
    from rl_ptg_amd.vec_env import PTGEnv
    tr, kw = H.kwargs_from_fixture("real_bs2_op2_mod_disc_evalval")
    env = PTGEnv(kw, "eval")
    obs, info = env.reset(seed=tr["meta"]["seed"])
    order = H_ORDER["mod"]
    np.testing.assert_allclose(_flat({k: np.asarray([v]) for k, v in obs.items()}, order)[0], tr["reset_obs"][0], rtol=RTOL, atol=ATOL)
    assert list(info) == tr["meta"]["info_keys"]
    for q, k in enumerate(tr["meta"]["info_keys"]):
        if k != "Meth_Action":
            assert float(info[k]) == tr["reset_info"][0, q], k
    tot = 0.0
    for t in range(600):
        obs, r, term, trunc, info = env.step(int(tr["actions"][t, 0]))
        assert trunc is False and term is False and isinstance(r, float)
        np.testing.assert_allclose(_flat({k: np.asarray([v]) for k, v in obs.items()}, order)[0], tr["obs"][t, 0], rtol=RTOL, atol=ATOL)
        H.assert_rewards([r], tr["f64s"][t, :1, 0], "float32", err_msg=f"reward step {t}")
        assert info["step"] == t and abs(info["cum_reward"] - tr["f64s"][t, 0, 1]) < 1e-8
        tot += r
    env.close()


def test_vec_env_device_noise_and_tensor_path():
    """noise='device' (in-kernel RNG) with the float32 feature-major fast path: tensors stay on the GPU, shapes and basic sanity."""
    import torch
    from rl_ptg_amd.vec_env import PtGVecEnv
    from rl_ptg_amd.prep import synthetic_spec
    spec, _ = synthetic_spec(scenario=1, operation="OP1", eps_len_d=32)
    n = 4096
    env = PtGVecEnv(spec, n, seed=5, out_dtype="float32", obs_layout="feature", noise="device")
    obs = env.reset()
    assert obs["Pot_Reward"].shape == (n, 13) and obs["METH_STATUS"].shape == (n,)
    a = torch.randint(0, 5, (n,), dtype=torch.int32, device="cuda")
    for _ in range(20):
        o, r, d = env.step_tensors(a)
    env.engine.sync()
    assert o.shape == (35, n) and o.is_cuda and r.shape == (n,) and int(d.sum()) == 0
    assert torch.isfinite(o).all() and torch.isfinite(r).all()
    obs2, rew, done, infos = env.step(a.cpu().numpy())
    assert set(np.unique(obs2["METH_STATUS"])) <= {0, 1, 2, 3, 4}
    env.close()
