"""Resolved configs of the BASELINE.json workloads and the model presets.

PRESETS holds what the reference's load_config(...) resolves for each id (values taken
from config/environments/{CartPole-v1,LunarLander-v3,Acrobot-v1,ALE-Pong-v5,ALE-Breakout-v5}.yaml
through utils/config.py; tests/golden/configs.json, config_acrobot.json for Acrobot-v1:ppo and
config_mountaincar.json for the three MountainCar-v0 variants are the machine-generated records
the tests compare against).  The reference leaves MountainCar-v0's n_envs at "auto", the host's core
count (utils/config.py:482-485): the record keeps "auto" and the presets take 32; the same holds for
FrozenLake-v1's ppo / ppo_deterministic and Taxi-v3's ppo (config_toytext.json) and for Bandit-v0's ppo
(config_cartpole_bandit.json, which also records CartPole-v1:ppo_rewardshaped); config_pong_objects.json
records ALE-Pong-v5's objects_ppo / objects_deterministic_ppo (masked MLP policies).  MODEL_REGISTRY
mirrors utils/model_registry.py:17-76.
"""

MODEL_REGISTRY = {
    "mlp_tiny": {"policy": "mlp_actorcritic", "hidden_dims": (64,)},
    "mlp_small": {"policy": "mlp_actorcritic", "hidden_dims": (128, 128)},
    "mlp_medium": {"policy": "mlp_actorcritic", "hidden_dims": (256, 256)},
    "mlp_large": {"policy": "mlp_actorcritic", "hidden_dims": (512, 512)},
    "cnn_nature": {"policy": "cnn_actorcritic", "hidden_dims": (512,),
                   "channels": (32, 64, 64), "kernel_sizes": (8, 4, 3), "strides": (4, 2, 1)},
    "cnn_impala": {"policy": "cnn_actorcritic", "hidden_dims": (256,),
                   "channels": (16, 32, 32), "kernel_sizes": (8, 4, 3), "strides": (4, 2, 1)},
    "cnn_large": {"policy": "cnn_actorcritic", "hidden_dims": (1024,),
                  "channels": (32, 64, 128), "kernel_sizes": (8, 4, 3), "strides": (4, 2, 1)},
}

_COMMON = dict(algo_id="ppo", clip_range_vf=0.2, vf_coef=0.5, max_grad_norm=0.5, normalize_advantages="batch",
               seed=42, target_kl=None, optimizer="adam")

_MC_SHAPER = dict(id="MountainCarV0_RewardShaper", position_reward_scale=100.0, velocity_reward_scale=10.0,
                  height_reward_scale=50.0)
_MC_CURIOSITY = dict(id="MountainCarV0_StateCountBonus", position_bins=50, velocity_bins=50, bonus_scale=0.1,
                     bonus_type="count")

PRESETS = {
    "CartPole-v1:ppo": dict(
        _COMMON, env_id="CartPole-v1", project_id="CartPole-v1", n_envs=8, n_steps=32, batch_size=256, n_epochs=20,
        gamma=0.98, gae_lambda=0.8, clip_range=0.1, ent_coef=0.0, policy_lr=0.001, model_id="mlp_medium",
        max_env_steps=100000.0, obs_type="vector", accelerator="cpu",
        spec={"action_space": {"discrete": 2}, "observation_space": {"default": "state",
                                                                     "variants": {"state": {"shape": [4]}}}}),
    # the reward-shaped variant (config/environments/CartPole-v1.yaml:46-53, 83-87; record:
    # tests/golden/config_cartpole_bandit.json): CartPole-v1:ppo under CartPoleV1_RewardShaper
    "CartPole-v1:ppo_rewardshaped": dict(
        _COMMON, env_id="CartPole-v1", project_id="CartPole-v1_rewardshaped", n_envs=8, n_steps=32, batch_size=256,
        n_epochs=20, gamma=0.98, gae_lambda=0.8, clip_range=0.1, ent_coef=0.0, policy_lr=0.001,
        model_id="mlp_medium", max_env_steps=100000.0, obs_type="vector", accelerator="cpu",
        env_wrappers=[dict(id="CartPoleV1_RewardShaper", angle_reward_scale=1.0, position_reward_scale=0.25,
                           clip_potential=True)],
        spec={"action_space": {"discrete": 2}, "observation_space": {"default": "state",
                                                                     "variants": {"state": {"shape": [4]}}}}),
    # Bandit-v0 (config/environments/Bandit-v0.yaml:47-60; same record): the reference's stateless
    # Gaussian bandit, the one classic config with a scheduled policy_lr (0.04 -> 0, linear over the
    # whole budget).  n_envs resolves to "auto" there as for MountainCar-v0: 32 here.  The spec's
    # observation shape is the symbol n_arms: resolved_obs_dim() follows env_kwargs.
    "Bandit-v0:ppo": dict(
        _COMMON, env_id="Bandit-v0", project_id="Bandit-v0", n_envs=32, n_steps=64, batch_size=64, n_epochs=4,
        gamma=1.0, gae_lambda=1.0, clip_range=0.2, ent_coef=0.0, policy_lr=0.04, model_id="mlp_small",
        max_env_steps=20000, obs_type="vector", accelerator="cpu",
        env_kwargs={"n_arms": 10, "means": [0, 1, 2, 3, 4, 5, 6, 7, 8, 9], "stds": 1, "episode_length": 1},
        schedules={"policy_lr": {"schedule": "linear", "start_value": 0.04, "end_value": 0.0, "start": 0.0,
                                 "end": 1.0, "warmup": 0.0}},
        spec={"action_space": {"discrete": 10},
              "observation_space": {"default": "constant_zero",
                                    "variants": {"constant_zero": {"shape": ["n_arms"], "dtype": "float32"}}}}),
    # Bandit-v0's reinforce variant (config/environments/Bandit-v0.yaml:62-73; record:
    # tests/golden/config_reinforce.json): REINFORCEConfig's defaults (utils/config.py:806-816) under the
    # same env.  The yaml names no model_id — the reference asserts at utils/config.py:463 and cannot
    # start — so this preset takes its ppo sibling's mlp_small (the record keeps null); n_envs "auto"
    # -> 32, so N T = 32 x 64 = 2048 = batch_size: one optimizer step per rollout.
    "Bandit-v0:reinforce": dict(
        algo_id="reinforce", env_id="Bandit-v0", project_id="Bandit-v0", n_envs=32, n_steps=64, batch_size=2048,
        n_epochs=1, gamma=1.0, gae_lambda=1.0, ent_coef=0.01, max_grad_norm=0.5, policy_lr=0.04, model_id="mlp_small",
        max_env_steps=20000, obs_type="vector", accelerator="cpu", seed=42, optimizer="adam",
        returns_type="mc:rtg", policy_targets="returns", normalize_returns="off", normalize_advantages="off",
        env_kwargs={"n_arms": 10, "means": [0, 1, 2, 3, 4, 5, 6, 7, 8, 9], "stds": 1, "episode_length": 1},
        schedules={"policy_lr": {"schedule": "linear", "start_value": 0.04, "end_value": 0.0, "start": 0.0,
                                 "end": 1.0, "warmup": 0.0}},
        spec={"action_space": {"discrete": 10},
              "observation_space": {"default": "constant_zero",
                                    "variants": {"constant_zero": {"shape": ["n_arms"], "dtype": "float32"}}}}),
    "LunarLander-v3:ppo": dict(
        _COMMON, env_id="LunarLander-v3", project_id="LunarLander-v3", n_envs=8, n_steps=2048, batch_size=64,
        n_epochs=10, gamma=0.99, gae_lambda=0.95, clip_range=0.2, ent_coef=0.0, policy_lr=0.0003,
        model_id="mlp_small", max_env_steps=5000000.0, obs_type="vector",
        spec={"action_space": {"discrete": 4}, "observation_space": {"default": "state",
                                                                     "variants": {"state": {"shape": [8]}}}}),
    "Acrobot-v1:ppo": dict(
        _COMMON, env_id="Acrobot-v1", project_id="Acrobot-v1", n_envs=32, n_steps=2048, batch_size=64,
        n_epochs=10, gamma=0.99, gae_lambda=0.95, clip_range=0.2, ent_coef=0.0, policy_lr=0.0003,
        model_id="mlp_small", max_env_steps=1000000.0, obs_type="vector", accelerator="cpu",
        spec={"action_space": {"discrete": 3}, "observation_space": {"default": "state",
                                                                     "variants": {"state": {"shape": [6]}}}}),
    **{f"MountainCar-v0:{variant}": dict(
        _COMMON, env_id="MountainCar-v0", project_id=project, n_envs=32, n_steps=2048, batch_size=64,
        n_epochs=10, gamma=0.99, gae_lambda=0.95, clip_range=0.2, ent_coef=0.0, policy_lr=0.0003,
        model_id="mlp_medium", max_env_steps=None, obs_type="vector", accelerator="cpu", env_wrappers=wrappers,
        spec={"action_space": {"discrete": 3}, "observation_space": {"default": "state",
                                                                     "variants": {"state": {"shape": [2]}}}})
       for variant, project, wrappers in (
           # `ppo` is the curiosity env too (config/environments/MountainCar-v0.yaml:74-77)
           ("ppo", "MountainCar-v0_curiosity", [dict(_MC_CURIOSITY)]),
           ("ppo_rewardshaped", "MountainCar-v0_rewardshaped", [dict(_MC_SHAPER)]),
           ("ppo_curiosity", "MountainCar-v0_curiosity", [dict(_MC_CURIOSITY)]))},
    # FrozenLake-v1 / Taxi-v3 (config/environments/{FrozenLake-v1,Taxi-v3}.yaml; record:
    # tests/golden/config_toytext.json): Discrete observations through the reference's DiscreteEncoder,
    # mlp_tiny (one hidden layer of 64).  n_envs resolves to "auto" there as for MountainCar-v0: 32 here.
    # The spec names the state count (`n`), not a shape: resolved_obs_dim() follows the encoder.
    **{f"FrozenLake-v1:{variant}": dict(
        _COMMON, env_id="FrozenLake-v1", project_id=project, n_envs=32, n_steps=2048, batch_size=64,
        n_epochs=10, gamma=0.99, gae_lambda=0.95, clip_range=0.2, ent_coef=0.0, policy_lr=0.0003,
        model_id="mlp_tiny", max_env_steps=None, obs_type="vector", accelerator="cpu",
        env_kwargs={"is_slippery": slippery, "map_name": "4x4"},
        env_wrappers=[{"id": "DiscreteEncoder", "encoding": "array"}],
        spec={"action_space": {"discrete": 4},
              "observation_space": {"default": "grid_4x4", "variants": {"grid_4x4": {"n": 16, "dtype": "int64"},
                                                                        "grid_8x8": {"n": 64, "dtype": "int64"}}}})
       for variant, project, slippery in (("ppo", "FrozenLake-v1", True),
                                          ("ppo_deterministic", "FrozenLake-v1_deterministic", False))},
    "Taxi-v3:ppo": dict(
        _COMMON, env_id="Taxi-v3", project_id="Taxi-v3", n_envs=32, n_steps=1024, batch_size=64, n_epochs=20,
        gamma=0.99, gae_lambda=0.95, clip_range=0.2, ent_coef=0.01, policy_lr=0.01, model_id="mlp_tiny",
        max_env_steps=10000000.0, obs_type="vector", accelerator="cpu",
        env_wrappers=[{"id": "DiscreteEncoder", "encoding": "array"}],
        spec={"action_space": {"discrete": 6},
              "observation_space": {"default": "encoded_state",
                                    "variants": {"encoded_state": {"n": 500, "dtype": "int64"}}}}),
    "ALE-Pong-v5:rgb_ppo": dict(
        _COMMON, env_id="ALE/Pong-v5", project_id="ALE-Pong-v5_rgb", n_envs=32, n_steps=256, batch_size=1024,
        n_epochs=15, gamma=0.99, gae_lambda=0.95, clip_range=0.2, ent_coef=0.01, policy_lr=0.0003,
        model_id="cnn_nature", max_env_steps=5000000.0, obs_type="rgb", frame_stack=4,
        spec={"action_space": {"discrete": 18, "valid": [0, 3, 4]}}),
    # Pong on extracted objects (config/environments/ALE-Pong-v5.yaml:180-242; record:
    # tests/golden/config_pong_objects.json): 12 features from the host's PongV5_FeatureExtractor, the full
    # 18-action space masked down to NOOP / RIGHT / LEFT.  No device dynamics: env= / env_factory= as the
    # rgb configs.  batch_size 2048 and the mask both put these on the row-parallel update's masked entries.
    "ALE-Pong-v5:objects_ppo": dict(
        _COMMON, env_id="ALE/Pong-v5", project_id="ALE-Pong-v5_objects", n_envs=32, n_steps=1024, batch_size=2048,
        n_epochs=8, gamma=0.995, gae_lambda=0.96, clip_range=0.3, ent_coef=0.04, policy_lr=0.0055,
        model_id="mlp_small", max_env_steps=3500000, obs_type="objects", accelerator="cpu",
        env_wrappers=[{"id": "PongV5_FeatureExtractor", "action_ids": [0, 3, 4]}],
        schedules={"policy_lr": {"schedule": "linear", "start_value": 0.0055, "end_value": 0.00015, "start": 0.0,
                                 "end": 0.92, "warmup": 0.0},
                   "clip_range": {"schedule": "linear", "start_value": 0.3, "end_value": 0.08, "start": 0.5,
                                  "end": 0.85, "warmup": 0.0},
                   "ent_coef": {"schedule": "linear", "start_value": 0.04, "end_value": 0.0001, "start": 0.48,
                                "end": 0.65, "warmup": 0.0}},
        spec={"action_space": {"discrete": 18, "valid": [0, 3, 4]},
              "observation_space": {"default": "state", "variants": {"state": {"shape": [12], "dtype": "float32"}}}}),
    "ALE-Pong-v5:objects_deterministic_ppo": dict(
        _COMMON, env_id="ALE/Pong-v5", project_id="ALE-Pong-v5_objects_deterministic", n_envs=32, n_steps=1024,
        batch_size=2048, n_epochs=10, gamma=0.99, gae_lambda=0.95, clip_range=0.1, ent_coef=0.0, policy_lr=0.01,
        model_id="mlp_tiny", max_env_steps=1500000, obs_type="objects", accelerator="cpu",
        env_kwargs={"repeat_action_probability": 0.0},
        env_wrappers=[{"id": "PongV5_FeatureExtractor", "action_ids": [0, 3, 4]}],
        spec={"action_space": {"discrete": 18, "valid": [0, 3, 4]},
              "observation_space": {"default": "state", "variants": {"state": {"shape": [12], "dtype": "float32"}}}}),
    "ALE-Breakout-v5:rgb_ppo": dict(
        _COMMON, env_id="ALE/Breakout-v5", project_id="ALE-Breakout-v5_rgb", n_envs=32, n_steps=128,
        batch_size=1024, n_epochs=4, gamma=0.99, gae_lambda=0.95, clip_range=0.1, ent_coef=0.01,
        policy_lr=0.0003, model_id="cnn_nature", max_env_steps=None, obs_type="rgb", frame_stack=4,
        spec={"action_space": {"discrete": 18, "valid": [0, 1, 3, 4]}}),
}
