"""CPU: the Acrobot-v1 restatement (tests/acrobot_twin.py, the twin of csrc/gs_acrobot_env.h)
checked independently of the kernel, and the config / agent plumbing of the device Acrobot env."""
import json
import math
import os

import numpy as np
import pytest

import acrobot_twin as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _energy(y):
    """Total mechanical energy of the two-link pendulum of the "book" equations (m = l1 = I = 1,
    lc = 0.5, g = 9.8), angles from the downward vertical."""
    t1, t2, w1, w2 = y
    m1 = m2 = l1 = I1 = I2 = 1.0
    lc1 = lc2 = 0.5
    g = 9.8
    v2sq = l1 * l1 * w1 * w1 + lc2 * lc2 * (w1 + w2) ** 2 + 2.0 * l1 * lc2 * w1 * (w1 + w2) * math.cos(t2)
    return (0.5 * m1 * (lc1 * w1) ** 2 + 0.5 * I1 * w1 * w1 + 0.5 * m2 * v2sq + 0.5 * I2 * (w1 + w2) ** 2
            - m1 * g * lc1 * math.cos(t1) - m2 * g * (l1 * math.cos(t1) + lc2 * math.cos(t1 + t2)))


def test_equations_conserve_energy_without_torque():
    """A sign or index error in the restated derivative breaks energy conservation; the device-
    against-twin tests cannot see one (both restate the same text).  Torque 0, 0.2 s in 2000 RK4
    sub-steps of 1e-4 (truncation error ~ 1e-16 per step), 200 random states with every
    component in [-3, 3]: relative drift below 1e-10 (a correct restatement measures ~8e-14)."""
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(200):
        y = [float(v) for v in rng.uniform(-3.0, 3.0, 4)]
        e0 = _energy(y)
        for _ in range(2000):
            y = T.rk4(y, 0.0, 1e-4)
        worst = max(worst, abs(_energy(y) - e0) / max(abs(e0), 1.0))
    print("worst relative energy drift", worst)
    assert worst < 1e-10


def test_twin_known_answers():
    # hanging at rest with no torque: an equilibrium
    s, term, info = T.step_state([0.0, 0.0, 0.0, 0.0], 1)
    assert max(abs(v) for v in s) < 1e-15 and not term
    assert info == {"wrap1": 0, "wrap2": 0, "clamp1": False, "clamp2": False}
    # both links straight up: the tip is 2 above the pivot, beyond the line at 1
    assert T.height([math.pi, 0.0]) > 1.0
    s, term, _ = T.step_state([math.pi, 0.0, 0.0, 0.0], 1)
    assert term
    # reward 0 on the terminating step, -1 otherwise; the step after a done only resets
    tw = T.AcrobotTwin(2, seed=1, max_steps=50)
    tw.state[0] = [math.pi, 0.0, 0.0, 0.0]
    rew, done, trunc = tw.step([1, 1])
    assert rew.tolist() == [0.0, -1.0] and done.tolist() == [True, False] and not trunc.any()
    rew, done, trunc = tw.step([1, 1])
    assert rew.tolist() == [0.0, -1.0] and not done.any() and tw.infos[0] == "reset" and tw.steps == [0, 2]
    assert tw.state[0] == [T.reset_uniform(1, 0, 1, c) for c in range(4)]
    assert all(abs(v) <= 0.1 and v == float(np.float32(v)) for v in tw.state[0])


def test_wrap_is_bounded():
    """The wrap loops stop after WRAP_CAP turns: an infinite or huge angle returns instead of
    spinning, a NaN passes through, and an angle within the cap is wrapped exactly as before."""
    assert T.WRAP_CAP == 16
    for bad in (math.inf, -math.inf):
        x, n = T.wrap(bad)
        assert x == bad and n == T.WRAP_CAP
    x, n = T.wrap(1e9)
    assert n == T.WRAP_CAP and x == pytest.approx(1e9 - 32 * math.pi)
    assert math.isnan(T.wrap(math.nan)[0])
    x, n = T.wrap(3.0 + 6.0 * math.pi)
    assert n == 3 and x == pytest.approx(3.0, abs=1e-12)
    x, n = T.wrap(-3.0 - 4.0 * math.pi)
    assert n == 2 and x == pytest.approx(-3.0, abs=1e-12)
    # a whole step on a non-finite state returns
    s, term, _ = T.step_state([math.inf, 0.0, 0.0, 0.0], 2)
    assert len(s) == 4 and not term


def _fixture():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "config_acrobot.json")))["Acrobot-v1:ppo"]


def test_acrobot_config_names_the_device_env():
    from types import SimpleNamespace
    from gsamd import needs_host_env
    from gsamd.config import device_env_kind, from_reference_config, load_config
    from gsamd.presets import PRESETS
    full = _fixture()
    cfg = load_config("Acrobot-v1", "ppo")
    assert device_env_kind(cfg) == "acrobot"
    assert device_env_kind(from_reference_config(SimpleNamespace(**full))) == "acrobot"
    assert needs_host_env(SimpleNamespace(**full)) is False
    # the bundled preset is what the reference resolves from its YAML
    preset = PRESETS["Acrobot-v1:ppo"]
    for k, v in preset.items():
        if k == "spec":
            assert v["action_space"]["discrete"] == full["spec"]["action_space"]["discrete"] == 3
            assert (v["observation_space"]["variants"]["state"]["shape"]
                    == full["spec"]["observation_space"]["variants"]["state"]["shape"] == [6])
        else:
            assert full[k] == v, k
    assert (cfg.n_envs, cfg.n_steps, cfg.batch_size, cfg.n_epochs) == (32, 2048, 64, 10)
    assert tuple(cfg.hidden_dims) == tuple(full["_hidden_dims"]) == (128, 128)
    assert cfg.resolved_obs_dim() == 6 and cfg.resolved_n_actions() == 3
    # wrappers make it another env: the host VectorEnv is needed
    shaped = from_reference_config(SimpleNamespace(**dict(full, env_wrappers=[{"id": "X"}])))
    assert device_env_kind(shaped) is None


def _bare_agent(cfg):
    """A DevicePPOAgent with only what build_env reads (no device buffers: runs on CPU)."""
    import torch
    from gsamd.ppo_agent import DevicePPOAgent
    a = object.__new__(DevicePPOAgent)
    a.config, a.rank, a.device, a._envs, a.env_factory = cfg, 0, torch.device("cpu"), {}, None
    return a


def test_agent_builds_the_acrobot_env_per_stage():
    from gsamd.config import load_config
    from gsamd.rollout import DeviceAcrobotVecEnv
    cfg = load_config("Acrobot-v1", "ppo")
    a = _bare_agent(cfg)
    a.build_env("train")
    a.build_env("val")
    tr, va = a.get_env("train"), a.get_env("val")
    assert isinstance(tr, DeviceAcrobotVecEnv) and tr.seed == cfg.seed_train and tr.max_steps == 500
    assert isinstance(va, DeviceAcrobotVecEnv) and va.seed == cfg.seed_val
    assert tr.device_native and tr.obs_shape == (6,) and tr.n_actions == 3 and tr.num_envs == 32
    assert tuple(tr.state.shape) == (32, 4) and tuple(tr.meta.shape) == (32, 3) and tuple(tr.obs.shape) == (32, 6)
    short = _bare_agent(load_config("Acrobot-v1", "ppo", overrides=dict(max_episode_steps=50)))
    short.build_env("train")
    assert short.get_env("train").max_steps == 50
    # the dynamics need the env's own shapes
    wrong = _bare_agent(load_config("CartPole-v1", "ppo", overrides=dict(env_dynamics="acrobot")))
    with pytest.raises(ValueError, match="acrobot"):
        wrong.build_env("train")
