"""rl_ptg_amd: MI355X-native batched Power-to-Gas environment (HIP kernels behind a C ABI, SB3 VecEnv surface).

    from rl_ptg_amd import PtGVecEnv, PTGEnv, HipEngine, DeviceReplayBuffer, DeviceRolloutBuffer, SdeNoise, SquashedSdeNoise, DeviceOptimizer, DeviceOptimizerGroup, DeviceMLP, TrainMLP, DeviceMLPGroup, TrainMLPGroup, EnvConfig, Preprocessing, EnvSpec
"""
__version__ = "0.1.0"

_LAZY = {"PtGVecEnv": "vec_env", "PTGEnv": "vec_env", "HipEngine": "engine", "PtgError": "engine", "CategoricalAct": "engine", "EpsGreedyAct": "engine", "GaussianAct": "engine", "PolicyLoss": "engine", "ppo_loss": "loss", "a2c_loss": "loss", "ppo_loss_group": "loss", "a2c_loss_group": "loss", "dqn_loss": "loss", "td3_critic_loss": "loss", "sac_critic_loss": "loss", "TdLoss": "train_ops", "tqc_critic_loss": "loss", "QuantileLoss": "train_ops", "squashed_rsample": "loss", "sac_actor_loss": "loss", "tqc_actor_loss": "loss", "td3_actor_loss": "loss", "ent_coef_loss": "loss",
         "dqn_loss_group": "loss", "td3_critic_loss_group": "loss", "sac_critic_loss_group": "loss", "squashed_rsample_group": "loss", "sac_actor_loss_group": "loss", "tqc_actor_loss_group": "loss", "td3_actor_loss_group": "loss", "ent_coef_loss_group": "loss",
         "RSample": "train_ops", "RSampleGrad": "train_ops", "ActorLoss": "train_ops", "MlpOut": "train_ops", "DeviceMLP": "mlp", "TrainMLP": "mlp", "DeviceMLPGroup": "mlp", "TrainMLPGroup": "mlp", "DeviceOptimizer": "optim", "DeviceOptimizerGroup": "optim", "OptimPlan": "train_ops", "DeviceReplayBuffer": "replay", "ReplayStorage": "replay", "ReplaySamples": "replay", "DeviceRolloutBuffer": "rollout_buffer", "RolloutStorage": "rollout_buffer", "RolloutBufferSamples": "rollout_buffer", "EnvConfig": "config",
         "SdeNoise": "sde", "SquashedSdeNoise": "sde", "sde_squashed_rsample": "loss", "SdeRSample": "train_ops", "SdeRSampleGrad": "train_ops", "SdeAct": "train_ops", "SdePolicyLoss": "train_ops", "ppo_sde_loss": "loss", "a2c_sde_loss": "loss",
         "Preprocessing": "prep", "EnvSpec": "prep", "synthetic_spec": "prep", "load_op_tables": "tables", "load_data": "market", "import_market_data": "market"}


def __getattr__(name):
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module(f".{_LAZY[name]}", __name__), name)
    raise AttributeError(name)
