"""The headline workload (BASELINE.json configs[2]: N = 65 536, BS1/OP1, 32-day episodes) through one WHOLE episode and into the
next against the CPU oracle: 4 615 steps, the synchronised batch terminating on step index 4 602 (call 4 603).  The oracle follows a
256-env slice that straddles two workgroups (envs are independent).  Checked at every step: observations, rewards and done flags;
at the end of the episode: the terminating step of every env, the finished returns and lengths, cum_rew after 4 602 float64 adds of
the price-linear reward form (float32 path: its operand order is not the reference's), and the post-reset state.

The synthetic trace holds one 32-day episode in 38 days, so eps_ind is all zeros and every reset starts at offset 0 by construction;
the episode-plan mapping is covered by tests/test_mixed_scenarios.py."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

INT_FIELDS = ["meth_state", "i", "j", "hot_cold", "standby_tid", "startup_tid", "partial_tid", "full_tid", "k", "current_action"]
N, LO, M = 65536, 40960 + 128, 256       # the slice [LO, LO + M) straddles two 256-env workgroups
K, T_END = 4615, 4602
L = 1536                                 # noise draws per env: the tape never wraps (asserted), so tape and RNG modes coincide
SEED, ACT_SEED = 31, 3

_oracle_run = {}


def _spec():
    from rl_ptg_amd.prep import synthetic_spec
    return synthetic_spec(scenario=1, operation="OP1", eps_len_d=32)[0]


def _slice_tape(spec):
    """The first L draws of the slice's counter-RNG streams (ptg_fill_noise_tape on a 256-env twin at the global offset LO)."""
    from rl_ptg_amd.engine import HipEngine
    twin = HipEngine(spec.consts, spec.tables, spec.markets, M, device=0, out_dtype="float64", obs_layout="row")
    twin.set_global_env_offset(LO)
    twin.fill_noise_tape(seed=SEED, per_env_len=L)
    tape = twin.get_noise_tape(L)
    twin.close()
    return tape


def _actions():
    import torch
    from rl_ptg_amd.synthetic import sticky_actions_device
    return sticky_actions_device(K, N, seed=ACT_SEED, device=torch.device("cuda", 0))


def _reference(spec, a_host):
    """The oracle's 4 615 steps of the slice, computed once and shared by every variant."""
    if "run" not in _oracle_run:
        m = spec.markets[0]
        consts = dict(spec.consts, scenario=m["scenario"], rew_l_b=m["rew_l_b"], rew_u_b=m["rew_u_b"], r_0=m["r_0"])
        ora = H.po.OracleVecEnv(consts, spec.tables, dict(m, eps_ind=None), M)
        ora.set_noise_tape(_slice_tape(spec))
        ora.reset()
        obs = np.zeros((K, M, ora.obs_dim))
        rew = np.zeros((K, M))
        done = np.zeros((K, M), np.uint8)
        for t in range(K):
            obs[t], rew[t], done[t], _, _ = ora.step(a_host[t])
            if t == T_END - 1:
                cum_before = ora.state()[1][:, 1].copy()
            if t == T_END:
                post_ints = ora.state()[0].copy()
        ints, f64s = ora.state()
        ora.close()
        _oracle_run["run"] = dict(obs=obs, rew=rew, done=done, cum_before=cum_before, post_ints=post_ints, ints=ints, f64s=f64s)
    return _oracle_run["run"]


def _ints(eng):
    cols = [eng.get_state(f)[LO:LO + M] for f in INT_FIELDS]
    actd = eng.get_state("act_ep_d")[LO:LO + M]
    return np.stack(cols + [actd * 24, actd], axis=1)


@pytest.mark.parametrize("variant", ["f32_rng_chunks", "f64_tape_chunks", "f32_rng_term_heads_launch", "f32_rng_eager_tail"])
def test_headline_episode_vs_oracle(variant):
    """f32_rng_chunks: float32 rows with the in-kernel counter RNG (bench.py's instantiation), fused chunks of 500 steps;
    f64_tape_chunks: float64 rows on a device-filled tape; f32_rng_term_heads_launch: chunk boundaries put the terminating step
    first in a launch (102 + 9 x 500 steps before it); f32_rng_eager_tail: fused up to step 4 590, then ptg_step launches for steps
    4 590 .. 4 614 (hot kernel, the generic kernel on the terminating step, hot again behind it)."""
    from rl_ptg_amd.engine import HipEngine
    out_dtype = "float64" if variant.startswith("f64") else "float32"
    spec = _spec()
    eng = HipEngine(spec.consts, spec.tables, spec.markets, N, device=0, out_dtype=out_dtype, obs_layout="row")
    eng.set_episode_plan(spec.eps_ind, N, N)
    assert not np.any(spec.eps_ind)
    if "tape" in variant:
        eng.fill_noise_tape(seed=SEED, per_env_len=L)
    else:
        eng.set_noise_rng(SEED)
    eng.reset()
    acts = _actions()
    a_host = acts[:, LO:LO + M].cpu().numpy()
    ref = _reference(spec, a_host)
    rtol, atol = (H.RTOL64, H.ATOL64) if out_dtype == "float64" else (H.RTOL32, H.ATOL32)
    if variant == "f32_rng_term_heads_launch":
        bounds = [0, 102] + [102 + 500 * j for j in range(1, 10)] + [K]
        assert bounds[-2] == T_END
    elif variant == "f32_rng_eager_tail":
        bounds = list(range(0, 4590, 500)) + [4590]
    elif variant == "f64_tape_chunks":
        bounds = list(range(0, T_END, 500)) + [T_END, K]   # a cut before the terminating step: cum_rew read there
    else:
        bounds = list(range(0, K, 500)) + [K]
    obs, rew, done = [], [], []
    n_done = 0
    fin = []
    cum_before = None
    for t0, t1 in zip(bounds[:-1], bounds[1:]):
        o, r, d = eng.rollout(acts[t0:t1])                 # 500 float32 steps of observations: 4.6 GB on the device
        eng.sync()
        obs.append(o[:, LO:LO + M].cpu().numpy()); rew.append(r[:, LO:LO + M].cpu().numpy())
        done.append(d[:, LO:LO + M].cpu().numpy())
        n_done += int(d.sum())
        fin.append(eng.finished_episodes())
        del o, r, d
        if t1 == T_END:
            cum_before = eng.get_state("cum_rew")[LO:LO + M]
    if variant == "f32_rng_eager_tail":
        for t in range(4590, K):
            o, r, d = eng.step(acts[t])
            eng.sync()
            obs.append(o[LO:LO + M].cpu().numpy()[None]); rew.append(r[LO:LO + M].cpu().numpy()[None])
            done.append(d[LO:LO + M].cpu().numpy()[None])
            n_done += int(d.sum())
            fin.append(eng.finished_episodes())
            if t == T_END - 1:
                cum_before = eng.get_state("cum_rew")[LO:LO + M]
            if t == T_END:
                post = _ints(eng)
    obs, rew, done = np.concatenate(obs), np.concatenate(rew), np.concatenate(done)
    assert obs.shape[0] == K
    # every env of the batch terminated on step 4 602 and on no other step
    assert n_done == N
    assert np.all(done[T_END] == 1) and not np.any(np.delete(done, T_END, axis=0))
    assert np.array_equal(done, ref["done"])
    for t in range(K):
        H.assert_rewards(rew[t], ref["rew"][t], out_dtype, err_msg=f"reward step {t}")
        np.testing.assert_allclose(obs[t], ref["obs"][t], rtol=rtol, atol=atol, err_msg=f"obs step {t}")
    # float64 sums of 4 602 rewards that agree to a few ulp: within 1e-9 of the summed magnitudes
    abs_ep = np.abs(ref["rew"][:T_END + 1]).sum(axis=0)
    if cum_before is not None:
        assert np.all(np.abs(cum_before - ref["cum_before"]) <= 1e-9 * abs_ep)
    r_fin = np.concatenate([f[0] for f in fin]); l_fin = np.concatenate([f[1] for f in fin]); id_fin = np.concatenate([f[2] for f in fin])
    assert len(id_fin) == N and np.array_equal(np.sort(id_fin), np.arange(N)) and set(l_fin.tolist()) == {T_END + 1}
    sel = (id_fin >= LO) & (id_fin < LO + M)
    order = np.argsort(id_fin[sel])
    ret_ref = ref["rew"][:T_END + 1].sum(axis=0)
    assert np.all(np.abs(r_fin[sel][order] - ret_ref) <= 1e-9 * abs_ep)
    if variant == "f32_rng_eager_tail":
        assert np.array_equal(post, ref["post_ints"]) and np.all(post[:, 11] == 0) and np.all(post[:, 8] == 0)
    # 12 steps into the next episode: integer state, T_cat and cum_rew of the slice
    assert np.array_equal(_ints(eng), ref["ints"])
    assert np.array_equal(eng.get_state("T_cat")[LO:LO + M], ref["f64s"][:, 2])
    abs_new = np.abs(ref["rew"][T_END + 1:]).sum(axis=0)
    assert np.all(np.abs(eng.get_state("cum_rew")[LO:LO + M] - ref["f64s"][:, 1]) <= 1e-9 * abs_new)
    assert int(eng.get_state("noise_count")[LO:LO + M].max()) <= L
    eng.close()
