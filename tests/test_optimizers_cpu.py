"""config.optimizer = adam / adamw / sgd on the device update paths, without a device: the numpy twin
of the two new steps (tests/optimizer_twin.py) against torch's own optimizers, the config field and
the flags bit it becomes, the C interface's constants and unchanged shape, and the refusal of both
optimizer bits at once before any launch."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import optimizer_twin as OT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PARAMS, N_ZERO, N_STEPS = 5000, 50, 5


def _inputs():
    """5000 parameters of scale 0.5; per step gradients of magnitude 1e-6 .. 1 (log-uniform, random
    sign), exactly zero at the same 50 entries in every step"""
    rng = np.random.default_rng(2024)
    p0 = (0.5 * rng.standard_normal(N_PARAMS)).astype(np.float32)
    zero = rng.permutation(N_PARAMS)[:N_ZERO]
    grads = []
    for _ in range(N_STEPS):
        g = (10.0 ** rng.uniform(-6, 0, N_PARAMS) * rng.choice([-1.0, 1.0], N_PARAMS)).astype(np.float32)
        g[zero] = 0.0
        grads.append(g)
    return p0, grads, zero


@pytest.mark.parametrize("lr", [3e-4, 0.05])
@pytest.mark.parametrize("name", ["adamw", "sgd"])
def test_twin_matches_torch(name, lr):
    """Five steps of the twin against torch.optim.AdamW / torch.optim.SGD (lr only, every other
    argument at its default) on the CPU: max-abs difference <= 1e-6 after every step (the twin sat
    at most 2.4e-7 from torch where this was written; the bar leaves 4x for other BLAS /
    vectorisation builds).  The entries whose gradient is exactly zero are bit-equal to torch after
    every step, and under AdamW bit-equal to p0 multiplied that many times by f32(1 - lr * 0.01)."""
    p0, grads, zero = _inputs()
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = (torch.optim.AdamW if name == "adamw" else torch.optim.SGD)([tp], lr=lr)
    group = opt.param_groups[0]
    if name == "adamw":
        assert group["weight_decay"] == OT.WEIGHT_DECAY and group["betas"] == (0.9, 0.999) and group["eps"] == 1e-8
    else:
        assert group["momentum"] == 0 and group["dampening"] == 0 and group["weight_decay"] == 0
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    worst = 0.0
    for t, g in enumerate(grads, start=1):
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        if name == "adamw":
            p, m, v = OT.adamw_step(p, g, m, v, t, lr)
        else:
            p = OT.sgd_step(p, g, lr)
        want = tp.detach().numpy()
        assert p.dtype == np.float32
        worst = max(worst, float(np.abs(p.astype(np.float64) - want.astype(np.float64)).max()))
        assert np.array_equal(p[zero].view(np.uint32), want[zero].view(np.uint32)), t
        chain = OT.decayed(p0[zero], lr, t) if name == "adamw" else p0[zero]
        assert np.array_equal(p[zero].view(np.uint32), chain.view(np.uint32)), t
        if name == "adamw":
            assert not m[zero].any() and not v[zero].any()
    print("MEASURED %s lr %g: twin - torch max-abs %.2e over %d steps (bar 1e-06)" % (name, lr, worst, N_STEPS))
    assert worst <= 1e-6
    if name == "adamw":
        st = opt.state[tp]
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=0, atol=1e-6)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=0, atol=1e-6)


# ---- the config field and the flags bit -----------------------------------------------------------
def _bare(cls, cfg):
    """An agent with only what hparams() reads (no device buffers)."""
    a = object.__new__(cls)
    a.config, a.rank, a.world_size, a.track_stats, a.global_mode = cfg, 0, 1, False, False
    a.clip_range, a.clip_range_vf, a.vf_coef, a.ent_coef, a.policy_lr = 0.2, 0.2, 0.5, 0.01, cfg.policy_lr
    return a


def test_config_names_resolve_to_the_flags_bit():
    from gsamd._lib import GS_HP_OPT_ADAMW, GS_HP_OPT_SGD
    from gsamd.config import PPOConfig, REINFORCEConfig
    from gsamd.ppo_agent import DevicePPOAgent
    from gsamd.reinforce_agent import DeviceREINFORCEAgent
    both = GS_HP_OPT_ADAMW | GS_HP_OPT_SGD
    kw = dict(env_id="CartPole-v1", n_envs=8, n_steps=32, batch_size=64)
    assert PPOConfig(**kw).optimizer == "adam"
    for given, name, bit in (("adam", "adam", 0), ("adamw", "adamw", GS_HP_OPT_ADAMW), ("sgd", "sgd", GS_HP_OPT_SGD),
                             ("AdamW", "adamw", GS_HP_OPT_ADAMW), ("SGD", "sgd", GS_HP_OPT_SGD),
                             (types.SimpleNamespace(value="AdamW"), "adamw", GS_HP_OPT_ADAMW),
                             (types.SimpleNamespace(value="sgd"), "sgd", GS_HP_OPT_SGD)):
        for cfg_cls, agent_cls in ((PPOConfig, DevicePPOAgent), (REINFORCEConfig, DeviceREINFORCEAgent)):
            cfg = cfg_cls(optimizer=given, **kw)
            assert cfg.optimizer == name
            agent = _bare(agent_cls, cfg)
            assert agent.optimizer_name == name and int(agent.hparams().flags) & both == bit
    for bad in ("rmsprop", "", "adam_w", types.SimpleNamespace(value="lion")):
        for cfg_cls in (PPOConfig, REINFORCEConfig):
            with pytest.raises(ValueError, match="'adam', 'adamw' or 'sgd'"):
                cfg_cls(optimizer=bad, **kw)


# ---- the C interface ------------------------------------------------------------------------------
def test_abi_constants_and_unchanged_shape():
    from gsamd import _lib
    header = open(os.path.join(ROOT, "include", "gsamd.h")).read()
    defs = dict(re.findall(r"^#define\s+(GS_HP_OPT_ADAMW|GS_HP_OPT_SGD|GS_ADAMW_WEIGHT_DECAY)\s+(\S+)", header, re.M))
    assert defs == {"GS_HP_OPT_ADAMW": "4", "GS_HP_OPT_SGD": "8", "GS_ADAMW_WEIGHT_DECAY": "0.01"}
    assert (_lib.GS_HP_OPT_ADAMW, _lib.GS_HP_OPT_SGD, _lib.GS_ADAMW_WEIGHT_DECAY) == (4, 8, 0.01)
    assert not (_lib.GS_HP_OPT_ADAMW | _lib.GS_HP_OPT_SGD) & (_lib.GS_HP_BF16 | _lib.GS_HP_ACT_STATS)
    assert _lib.OPT_FLAGS == {"adam": 0, "adamw": 4, "sgd": 8}
    argtypes = json.load(open(os.path.join(ROOT, "tests", "golden", "lib_argtypes.json")))
    assert set(_lib.EXPORTED) == set(argtypes)                      # no new export
    assert ctypes.sizeof(_lib.PPOHparams) == 48
    assert _lib.lib.gs_abi_version() == 7 == _lib.GS_ABI_VERSION


def test_both_optimizer_bits_are_refused_before_any_launch():
    """GS_HP_OPT_ADAMW | GS_HP_OPT_SGD: GS_E_INVALID naming the optimizer bits from every entry that
    takes an optimizer step, with otherwise valid host-only arguments and no device in sight — the
    first check of each entry.  Either bit alone passes that check (the next one, a null buffer or an
    empty rollout, answers instead)."""
    from gsamd._lib import (GS_HP_OPT_ADAMW, GS_HP_OPT_SGD, CnnDims, MlpDims, PGHparams, PPOHparams, RolloutView,
                            RolloutViewU8, check, lib)
    two, one = MlpDims(4, 64, 64, 2), MlpDims(12, 64, 0, 18)
    cnn = CnnDims(4, 84, 84, 6, 512, 0b011001)

    def calls(flags):
        hp = PPOHparams(0.2, 0.2, 0.5, 0.01, 0.5, 3e-4, 0.9, 0.999, 1e-8, 0.0, 1, flags)
        pg = PGHparams(0.01, 0.5, 1e-2, 0.9, 0.999, 1e-8, 0, flags)
        ro, ro8 = RolloutView(), RolloutViewU8()
        for dims in (two, one):
            yield "gs_ppo_update", lambda d=dims: lib.gs_ppo_update(None, None, None, None, d, hp, ro, None, 64, 1, 0,
                                                                    None, None, None, 0, None, 0, None)
            yield "gs_ppo_minibatch_step", lambda d=dims: lib.gs_ppo_minibatch_step(None, None, None, None, d, hp, ro, None,
                                                                                    64, 1, None, None, None, None, None)
            yield "gs_ppo_rows_update", lambda d=dims: lib.gs_ppo_rows_update(None, None, None, None, d, hp, ro, None, 64, 1,
                                                                              0, None, None, None, 0, None, None)
            yield "gs_ppo_rows_update_masked", lambda d=dims: lib.gs_ppo_rows_update_masked(
                None, None, None, None, d, hp, ro, None, 64, 1, 0, None, None, None, 0, None, None, 0b11)
        yield "gs_pg_update", lambda: lib.gs_pg_update(None, None, None, None, two, pg, ro, None, 64, 1, 0, None, None, 0,
                                                       None, None)
        yield "gs_cnn_ppo_update", lambda: lib.gs_cnn_ppo_update(None, None, None, None, cnn, hp, ro8, None, 48, 1, 0, None,
                                                                 None, None, None, None)

    seen = set()
    for name, call in calls(GS_HP_OPT_ADAMW | GS_HP_OPT_SGD):
        with pytest.raises(ValueError, match=r"optimizer bits GS_HP_OPT_ADAMW and GS_HP_OPT_SGD are both set"):
            check(call(), name)
        seen.add(name)
    assert seen == {"gs_ppo_update", "gs_ppo_minibatch_step", "gs_ppo_rows_update", "gs_ppo_rows_update_masked",
                    "gs_pg_update", "gs_cnn_ppo_update"}
    for flags in (GS_HP_OPT_ADAMW, GS_HP_OPT_SGD):
        for name, call in calls(flags):
            with pytest.raises(ValueError) as e:
                check(call(), name)
            assert "optimizer bits" not in str(e.value), (name, str(e.value))
    # the stage entry times the Adam chain's stages: either bit is refused
    hp = PPOHparams(0.2, 0.2, 0.5, 0.01, 0.5, 3e-4, 0.9, 0.999, 1e-8, 0.0, 1, GS_HP_OPT_SGD)
    with pytest.raises(ValueError, match="gs_ppo_stage: the optimizer bits"):
        check(lib.gs_ppo_stage(0, None, None, None, None, two, hp, RolloutView(), None, 64, 1, None, None, None),
              "gs_ppo_stage")
