"""GPU parity of the NatureCNN / masked-categorical path (C4/C5 rows) through the C-ABI.

Checker: oracle/cnn_ref.py (torch-CPU fp32 restatement, pinned to the reference by
tests/golden/cnn_step.npz in tests/test_oracle_golden.py) and the fixture itself.
Tolerances: loss and metrics 1e-5 relative; log-probs / values 1e-5 absolute; gradients
2e-5 x max|g| (reductions over up to B*400 = 19 200 terms in a different order than
torch-CPU's); post-Adam parameters 2e-6 except where Adam's first step amplifies gradient noise
(see _adam_close).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = {"pong": ([0, 3, 4], 0.2, 0.01, 3e-4, 48, 1, 3), "breakout": ([0, 1, 3, 4], 0.1, 0.01, 3e-4, 40, 2, 5)}
# the bf16 mode's storage path (bf16 activations, dh and weight copy between the kernels) runs
# where the fc kernels take the batch (B % 64 == 0): its small-batch kernel shapes (conv1 in 4
# bands, the filter-split conv forwards) at B = 64 / 128
BF16_CASES = dict(CASES, pong64=([0, 3, 4], 0.2, 0.01, 3e-4, 64, 1, 3),
                  breakout128=([0, 1, 3, 4], 0.1, 0.01, 3e-4, 128, 2, 5))


def _adam_close(p, q, lr):
    """Adam's first step moves a weight by lr * g / (|g| + eps): for the few weights whose
    gradient is ~1e-9 (below fp32 reduction noise) the direction itself is noise.  All but
    1e-4 of the weights must agree to 2e-6 and every weight to 0.1 * lr."""
    d = np.abs(p - q)
    assert (d > 2e-6).sum() <= max(1, int(1e-4 * d.size)), (d > 2e-6).sum()
    assert d.max() <= 0.1 * lr, d.max()


def _setup(cuda, tag, cases=CASES):
    from oracle import cnn_case as K
    from gsamd._lib import PPOHparams, RolloutViewU8
    from gsamd.cnn import DeviceCNNActorCritic
    valid, clip, ent, lr, B, pseed, bseed = cases[tag]
    obs, act, olp, ov, adv, ret = K.cnn_batch(bseed, B, valid)
    pm = DeviceCNNActorCritic(valid_actions=valid, device=cuda, init=False)
    p_ref = K.cnn_params(pseed)
    pm.load_reference_flat(p_ref)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x))[None].to(cuda).contiguous()  # noqa: E731
    bufs = [t(obs), t(act), t(olp), t(ov), t(adv), t(ret)]
    view = RolloutViewU8(*(b.data_ptr() for b in bufs), 1, B)
    hp = PPOHparams(clip, 0.2, 0.5, ent, 0.5, lr, 0.9, 0.999, 1e-8, 0.0, 1, 0)
    idx = torch.arange(B, dtype=torch.int32, device=cuda)
    return pm, p_ref, bufs, view, hp, idx, (obs, act, olp, ov, adv, ret)


@pytest.mark.parametrize("tag", list(CASES))
def test_cnn_update_step_vs_oracle_and_reference(golden, cuda, tag):
    from oracle import cnn_ref as C
    from gsamd._lib import GS_NUM_METRICS, check, lib
    valid, clip, ent, lr, B, _, _ = CASES[tag]
    pm, p_ref, bufs, view, hp, idx, batch = _setup(cuda, tag)
    shapes = C.cnn_param_shapes()
    loss, met, g, logits, values = C.loss_and_grads(p_ref, shapes, *batch, valid=valid, clip=clip, clip_vf=0.2,
                                                    vf_coef=0.5, ent_coef=ent)
    P = p_ref.size
    p1, _, _, gc, total = C.clip_and_adam(p_ref, g, shapes, np.zeros(P, np.float32), np.zeros(P, np.float32), 1, lr)
    grads, m, v = (torch.zeros(pm.n_params, device=cuda) for _ in range(3))
    ws = torch.empty(int(lib.gs_cnn_workspace_bytes(pm.dims, B)), dtype=torch.uint8, device=cuda)
    met_d = torch.zeros(GS_NUM_METRICS, device=cuda)
    stop = torch.zeros(1, dtype=torch.int32, device=cuda)
    check(lib.gs_cnn_ppo_update(pm.params.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr(), pm.dims, hp, view,
                                idx.data_ptr(), B, 1, 0, met_d.data_ptr(), stop.data_ptr(), ws.data_ptr(), None,
                                torch.cuda.current_stream().cuda_stream), "gs_cnn_ppo_update")
    torch.cuda.synchronize()
    rec = met_d.cpu().numpy()
    assert abs(rec[0] - loss) < 1e-5 * max(1.0, abs(loss))
    assert abs(rec[12] - total) < 1e-5 * total
    g_dev = pm.flat_to_reference(grads)
    np.testing.assert_allclose(g_dev, gc, atol=2e-5 * np.abs(gc).max(), rtol=0)
    p_dev = pm.flat_to_reference(pm.params)
    _adam_close(p_dev, p1, lr)
    # the reference's own outputs on the same case
    z = golden("cnn_step.npz")
    assert abs(rec[0] - float(z[f"{tag}/loss"])) < 1e-5 * max(1.0, abs(loss))
    sel = z[f"{tag}/sel"]
    _adam_close(p_dev[sel], z[f"{tag}/params1_sel"], lr)
    ref = dict(zip([str(x) for x in z[f"{tag}/metric_names"]], z[f"{tag}/metric_values"]))
    for key, slot in (("opt/loss/policy", 1), ("opt/loss/value", 2), ("opt/policy/entropy", 3),
                      ("opt/ppo/clip_fraction", 4), ("opt/ppo/approx_kl", 8)):
        assert abs(rec[slot] - ref[key]) < 1e-5 * max(1.0, abs(ref[key])), key
    # pre-clip gradient norms per component, as the reference's compute_grad_norms records them
    # (utils/models.py:196-230: all, cnn, mlp, policy_head, value_head).  1e-4: the reference sums
    # 1.7 M fp32 squares in torch's order (rec[12] meets the f64 oracle's norm at 1e-5 above)
    from gsamd._lib import M
    gn = dict(zip([str(x) for x in z[f"{tag}/grad_norm_names"]], z[f"{tag}/grad_norm_values"]))
    for key, slot in (("opt/grads/norm/all", "grad_norm"), ("opt/grads/norm/cnn", "gn_backbone"),
                      ("opt/grads/norm/mlp", "gn_mlp"), ("opt/grads/norm/policy_head", "gn_policy_head"),
                      ("opt/grads/norm/value_head", "gn_value_head")):
        np.testing.assert_allclose(rec[M[slot]], gn[key], rtol=1e-4, err_msg=key)


@pytest.mark.parametrize("tag", list(CASES))
def test_cnn_policy_act_vs_oracle(cuda, tag):
    from oracle import cnn_ref as C
    valid = CASES[tag][0]
    pm, p_ref, bufs, view, hp, idx, batch = _setup(cuda, tag)
    obs = bufs[0][0]
    logits, values, _ = C.forward(C.unflatten(p_ref, C.cnn_param_shapes()), batch[0], valid)
    ln = (logits - torch.logsumexp(logits, -1, keepdim=True)).numpy()
    a, lp, v = pm.act(obs, mode=1)
    torch.cuda.synchronize()
    a = a.cpu().numpy()
    np.testing.assert_allclose(v.cpu().numpy(), values.numpy(), atol=1e-5, rtol=0)
    assert np.array_equal(a, np.argmax(ln, axis=1))
    np.testing.assert_allclose(lp.cpu().numpy(), ln[np.arange(len(a)), a], atol=1e-5, rtol=0)
    # sampling never draws a masked action, and replay reproduces the log-probs
    rep = obs.repeat(64, 1, 1, 1).contiguous()
    a_s, lp_s, _ = pm.act(rep, mode=0, rng_seed=7, rng_counter=3)
    torch.cuda.synchronize()
    a_s = a_s.cpu().numpy()
    assert set(np.unique(a_s)) <= set(valid)
    ln_rep = np.tile(ln, (64, 1))
    np.testing.assert_allclose(lp_s.cpu().numpy(), ln_rep[np.arange(len(a_s)), a_s], atol=1e-5, rtol=0)
    # the rollout row's obs copy (written by the first convolution from the frames it loads) and
    # the values at the small-batch kernel shapes (conv1 in 4 bands below 128 rows, conv2 / conv3
    # split over 2 workgroups per sample up to 512, the fc forward as split-K partials) and the
    # update-sized ones above
    g = torch.Generator().manual_seed(5)
    P = C.unflatten(p_ref, C.cnn_param_shapes())
    for n in (8, 128, 600):
        o = torch.randint(0, 256, (n,) + tuple(obs.shape[1:]), generator=g, dtype=torch.uint8)
        od = o.to(cuda)
        store = torch.zeros_like(od)
        a_n, lp_n, v_n = pm.act(od, mode=1, obs_store=store)
        torch.cuda.synchronize()
        assert torch.equal(store, od), n
        lg, vals, _ = C.forward(P, o, valid)
        ln_n = (lg - torch.logsumexp(lg, -1, keepdim=True)).numpy()
        np.testing.assert_allclose(v_n.cpu().numpy(), vals.numpy(), atol=1e-5, rtol=0, err_msg=str(n))
        a_n = a_n.cpu().numpy()
        np.testing.assert_allclose(lp_n.cpu().numpy(), ln_n[np.arange(n), a_n], atol=1e-5, rtol=0, err_msg=str(n))


@pytest.mark.parametrize("in_shape,T", [((4, 84, 84), 3), ((4, 52, 48), 2)])
def test_cnn_update_gathered_rows_and_generic_shapes(cuda, in_shape, T):
    """The update reads its minibatch through the sampler's env-major indices into a (T, N)
    rollout buffer (rollout_buffer.py:11-13).  (4, 84, 84) runs the LDS-resident conv kernels,
    (4, 52, 48) the generic implicit-GEMM path (u8 patch loader, NHWC patches, split-K weight
    gradients, dense dgrad + col2im); both against the oracle on the gathered rows.
    Tolerances as in test_cnn_update_step_vs_oracle_and_reference."""
    from oracle import cnn_case as K
    from oracle import cnn_ref as C
    from gsamd._lib import GS_NUM_METRICS, PPOHparams, RolloutViewU8, check, lib
    from gsamd.cnn import DeviceCNNActorCritic
    valid, clip, ent, lr, N = [0, 3, 4], 0.2, 0.01, 3e-4, 20
    B = 32
    obs, act, olp, ov, adv, ret = K.cnn_batch(11, T * N, valid, in_shape=in_shape)   # row = t * N + env
    rng = np.random.default_rng(5)
    idx = rng.permutation(T * N)[:B].astype(np.int32)                     # env-major i = env * T + t
    src = (idx % T) * N + idx // T
    batch = (obs[src], act[src], olp[src], ov[src], adv[src], ret[src])
    shapes = C.cnn_param_shapes(in_shape)
    p_ref = K.cnn_params(3, in_shape=in_shape)
    loss, met, g, logits, values = C.loss_and_grads(p_ref, shapes, *batch, valid=valid, clip=clip, clip_vf=0.2,
                                                    vf_coef=0.5, ent_coef=ent)
    P = p_ref.size
    p1, _, _, gc, total = C.clip_and_adam(p_ref, g, shapes, np.zeros(P, np.float32), np.zeros(P, np.float32), 1, lr)

    pm = DeviceCNNActorCritic(in_shape=in_shape, valid_actions=valid, device=cuda, init=False)
    pm.load_reference_flat(p_ref)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x)).to(cuda).contiguous()  # noqa: E731
    bufs = [t(obs), t(act), t(olp), t(ov), t(adv), t(ret)]
    view = RolloutViewU8(*(b.data_ptr() for b in bufs), T, N)
    hp = PPOHparams(clip, 0.2, 0.5, ent, 0.5, lr, 0.9, 0.999, 1e-8, 0.0, 1, 0)
    idx_d = torch.as_tensor(idx).to(cuda)
    grads, m, v = (torch.zeros(pm.n_params, device=cuda) for _ in range(3))
    ws = torch.empty(int(lib.gs_cnn_workspace_bytes(pm.dims, B)), dtype=torch.uint8, device=cuda)
    met_d = torch.zeros(GS_NUM_METRICS, device=cuda)
    stop = torch.zeros(1, dtype=torch.int32, device=cuda)
    # the loss-only entry (row-parallel loss kernel + its record) on the same minibatch, before the
    # update moves the parameters: the oracle's loss, and the same record from a second call
    loss_recs = []
    for _ in range(2):
        met_l = torch.zeros(GS_NUM_METRICS, device=cuda)
        check(lib.gs_cnn_ppo_loss(pm.params.data_ptr(), pm.dims, hp, view, idx_d.data_ptr(), B, met_l.data_ptr(), None,
                                  ws.data_ptr(), torch.cuda.current_stream().cuda_stream), "gs_cnn_ppo_loss")
        torch.cuda.synchronize()
        loss_recs.append(met_l.cpu().numpy())
    assert abs(loss_recs[0][0] - loss) < 1e-5 * max(1.0, abs(loss))
    assert loss_recs[0].tobytes() == loss_recs[1].tobytes()
    check(lib.gs_cnn_ppo_update(pm.params.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr(), pm.dims, hp, view,
                                idx_d.data_ptr(), B, 1, 0, met_d.data_ptr(), stop.data_ptr(), ws.data_ptr(), None,
                                torch.cuda.current_stream().cuda_stream), "gs_cnn_ppo_update")
    torch.cuda.synchronize()
    rec = met_d.cpu().numpy()
    assert abs(rec[0] - loss) < 1e-5 * max(1.0, abs(loss))
    assert abs(rec[12] - total) < 1e-5 * total
    np.testing.assert_allclose(pm.flat_to_reference(grads), gc, atol=2e-5 * np.abs(gc).max(), rtol=0)
    _adam_close(pm.flat_to_reference(pm.params), p1, lr)


@pytest.mark.parametrize("transport", ["xgmi", "rccl"])
def test_cnn_update_local_comm_equals_no_comm(cuda, transport):
    """gs_cnn_ppo_update with a one-rank communicator (the multi-GPU chain: gradient sum over
    ranks, 1/world scale in the norm and the update) gives bit for bit the single-GPU update on
    a C5-shaped shard (Breakout rgb_ppo, NatureCNN, B=1024): parameters, moments, losses."""
    from gsamd.config import load_config
    from gsamd.distributed import destroy_comm, init_local_comm
    from gsamd.ppo_agent import DevicePPOAgent
    out = []
    for with_comm in (False, True):
        torch.manual_seed(42)
        cfg = load_config("ALE-Breakout-v5", "rgb_ppo", overrides=dict(env_dynamics="synthetic", n_envs=64, n_steps=32, n_epochs=2))
        agent = DevicePPOAgent(cfg, device=cuda, track_stats=False)
        comm = init_local_comm(transport, agent.policy_model.n_params) if with_comm else None
        agent.comm = comm
        agent.train_epoch()
        torch.cuda.synchronize()
        out.append([t.cpu().numpy() for t in (agent.policy_model.params, agent.adam_m, agent.adam_v)] +
                   [agent.minibatch_losses()])
        del agent
        destroy_comm(comm)
    assert np.isfinite(out[0][0]).all()
    for name, x, y in zip(("params", "adam_m", "adam_v", "losses"), out[0], out[1]):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), name


def test_cnn_bf16_mode_deviation_bounded(cuda):
    """The bf16 performance mode (GS_HP_BF16: bf16 MFMA operands in every convolution / GEMM of
    the NatureCNN update, fp32 accumulation, parameters, loss and Adam) run
    beside the fp32 parity path from the same state on the same rollout and sampler order: the
    first minibatch's gradient keeps its direction (cosine > 0.98, relative L2 < 0.25) and the
    per-minibatch losses of one update (C4 shapes, B = 1024, 8 minibatches) stay within 5e-2 of the
    fp32 ones relative to their scale.  The fp32 path stays the default and the parity reference."""
    from gsamd._lib import GS_HP_BF16, check, lib, ptr, stream_handle
    from gsamd.config import load_config
    from gsamd.ppo_agent import DevicePPOAgent
    torch.manual_seed(42)
    cfg = load_config("ALE-Pong-v5", "rgb_ppo", overrides=dict(env_dynamics="synthetic", n_envs=16, n_steps=128,
                                                               n_epochs=4))
    agent = DevicePPOAgent(cfg, device=cuda, use_graph=False, track_stats=False)
    coll = agent.get_rollout_collector("train")
    coll.collect()
    idx = agent.prefetcher.upload(0)
    pm = agent.policy_model
    state = [t.clone() for t in (pm.params, agent.adam_m, agent.adam_v)]
    out = {}
    for name, n in (("fp32", 1), ("bf16", 1), ("fp32", agent.n_minibatches), ("bf16", agent.n_minibatches)):
        for t, s0 in zip((pm.params, agent.adam_m, agent.adam_v), state):
            t.copy_(s0)
        hp = agent.hparams()
        hp.flags = GS_HP_BF16 if name == "bf16" else 0
        check(lib.gs_cnn_ppo_update(ptr(pm.params), ptr(agent.grads), ptr(agent.adam_m), ptr(agent.adam_v), pm.dims,
                                    hp, coll.buffer.view(), ptr(idx), agent.batch_size, n, 0, ptr(agent.metrics_buf),
                                    ptr(agent.stop_flag), ptr(agent.workspace), None, stream_handle()),
              "gs_cnn_ppo_update")
        torch.cuda.synchronize()
        out[(name, n)] = (agent.grads.cpu().numpy().astype(np.float64), agent.metrics_buf[:n, 0].cpu().numpy())
    g32, g16 = out[("fp32", 1)][0], out[("bf16", 1)][0]
    cos = float(g32 @ g16 / (np.linalg.norm(g32) * np.linalg.norm(g16)))
    rel = float(np.linalg.norm(g16 - g32) / np.linalg.norm(g32))
    l32, l16 = out[("fp32", agent.n_minibatches)][1], out[("bf16", agent.n_minibatches)][1]
    dev = np.abs(l16.astype(np.float64) - l32) / max(1.0, float(np.abs(l32).max()))
    print(f"bf16 vs fp32: grad cos {cos:.6f} rel {rel:.4f}; loss dev per minibatch {dev}")
    assert agent.n_minibatches == 8 and np.isfinite(l16).all()
    # the deviation is the mode's own (ReLU units whose pre-activation sign flips under bf16
    # operand rounding; tests/test_gpu_cnn.py::test_cnn_bf16_update_step_vs_bf16_oracle shows the
    # kernels match the bf16-rounding oracle far tighter): direction kept, losses close
    # Adam's first steps move each weight by ~lr * sign(g), so weights whose small gradients change
    # sign under bf16 take opposite steps: the per-minibatch losses drift apart by ~1e-2 of their
    # scale (measured 1.5e-2 max over the 8) and stay there
    assert cos > 0.98 and 0.0 < rel < 0.25, (cos, rel)
    assert dev.max() < 5e-2, dev


@pytest.mark.parametrize("tag", list(BF16_CASES))
def test_cnn_bf16_update_step_vs_bf16_oracle(cuda, tag):
    """The bf16 mode's kernels against oracle/cnn_ref.py's bf16 emulation (operands rounded to
    bf16 at the points the HIP kernels round them, fp32 accumulation).  The bf16 gradient is
    itself sensitive to last-bit changes: perturbing the parameters by 1e-6 relative moves the
    emulation's gradient by 1.4e-2 (breakout) / 2.9e-2 (pong) relative L2 (fp32: 2e-6), as
    bf16 roundings, ReLU signs and clip decisions flip.  So: loss 1e-4 relative, head gradients
    5e-3, the whole clipped gradient within 2e-2 and under half the mode's deviation from the
    fp32 oracle (measured: pong 3.0e-4 vs 4.8e-2, breakout 1.5e-3 vs 3.1e-2)."""
    from oracle import cnn_ref as C
    from gsamd._lib import GS_HP_BF16, GS_NUM_METRICS, check, lib
    valid, clip, ent, lr, B, _, _ = BF16_CASES[tag]
    pm, p_ref, bufs, view, hp, idx, batch = _setup(cuda, tag, BF16_CASES)
    hp.flags = GS_HP_BF16
    shapes = C.cnn_param_shapes()
    kw = dict(valid=valid, clip=clip, clip_vf=0.2, vf_coef=0.5, ent_coef=ent)
    loss16, _, g16, _, _ = C.loss_and_grads(p_ref, shapes, *batch, bf16=True, **kw)
    _, _, g32, _, _ = C.loss_and_grads(p_ref, shapes, *batch, **kw)
    P = p_ref.size
    _, _, _, gc16, _ = C.clip_and_adam(p_ref, g16, shapes, np.zeros(P, np.float32), np.zeros(P, np.float32), 1, lr)
    _, _, _, gc32, _ = C.clip_and_adam(p_ref, g32, shapes, np.zeros(P, np.float32), np.zeros(P, np.float32), 1, lr)
    grads, m, v = (torch.zeros(pm.n_params, device=cuda) for _ in range(3))
    ws = torch.empty(int(lib.gs_cnn_workspace_bytes(pm.dims, B)), dtype=torch.uint8, device=cuda)
    met_d = torch.zeros(GS_NUM_METRICS, device=cuda)
    stop = torch.zeros(1, dtype=torch.int32, device=cuda)
    check(lib.gs_cnn_ppo_update(pm.params.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr(), pm.dims, hp, view,
                                idx.data_ptr(), B, 1, 0, met_d.data_ptr(), stop.data_ptr(), ws.data_ptr(), None,
                                torch.cuda.current_stream().cuda_stream), "gs_cnn_ppo_update")
    torch.cuda.synchronize()
    rec = met_d.cpu().numpy()
    g_dev = pm.flat_to_reference(grads).astype(np.float64)
    rl = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))  # noqa: E731
    r_emu, r_f32 = rl(g_dev, gc16.astype(np.float64)), rl(g_dev, gc32.astype(np.float64))
    per = []
    o = 0
    for n, s in shapes:
        k = int(np.prod(s))
        per.append((n, round(rl(g_dev[o:o + k], gc16[o:o + k].astype(np.float64)), 6)))
        o += k
    print(f"{tag}: vs bf16 oracle {r_emu:.2e}, vs fp32 oracle {r_f32:.2e}, loss {rec[0]} / {loss16}; {per}")
    assert abs(rec[0] - loss16) < 1e-4 * max(1.0, abs(loss16))
    assert all(r < 5e-3 for n, r in per if "head" in n), per
    assert r_emu < 2e-2 and r_emu < 0.5 * r_f32, (r_emu, r_f32, per)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_cnn_update_first_minibatches_vs_oracle(cuda, prec):
    """The production NatureCNN update at its production batch, against the oracle over many
    minibatches (the counterpart of test_gpu_parity.py::test_update_first_minibatches_vs_numpy_oracle):
    Pong rgb_ppo shapes, 32 envs x 256 steps, B = 1024 -> 8 minibatches of one gs_cnn_ppo_update
    call, so the fc kernels at K = 1024, the 16-ahead field gather (k_cnn_gather_chunk), the
    256-workgroup conv weight-gradient walks over 1024 samples and Adam steps 2..8 all run, on the
    rows the sampler picks (env-major indices -> (t, env) rows, rollout_buffer.py:105-173).

    * The update is captured whole into a graph and replayed from the same state: bit-identical to
      the eager run.  Runs of the same call with n = 1..8 minibatches end on that run's states
      after 1..8 steps, bit for bit (the update is deterministic), which gives the device's state
      before every step of the production 8-minibatch run.
    * Teacher-forced oracle, step by step: from the device's state before minibatch k, the oracle
      (oracle/cnn_ref.py, reference steps agents/base_agent.py:591-621) computes that minibatch's
      loss, pre-clip component norms and clip + Adam (step k + 1), with the device's ReLU
      decisions: at B = 1024 a few of the 22 M conv / fc pre-activations of a step sit within
      rounding of zero, their sign is decided by the summation order, and one flip moves every
      gradient entry the unit feeds (round 5: one conv2 flip moved 3.6 K entries by up to
      1.2e-3 x max|g| and the norms by 2.7e-4 after a rounding-level change of the conv1 weight
      gradient's partial sums).  So the oracle takes the step's decisions from the device (a1 / a2
      / a3 / h > 0 in the workspace: gs_cnn_workspace_act_offset; cnn_ref conv_masks / fc_mask),
      and every decision that differs from the oracle's own must be one it could not decide:
      |u| <= 1e-5 of the sum of its terms' magnitudes (cnn_ref.relu_decisions), at most 32 per
      conv layer and 8 in the fc per step (measured: at most 3, |u| / mag <= 4e-8).  fp32 bars,
      then arithmetic only: loss 1e-5 relative, norms 1e-5 relative, the new parameters within
      2e-6 except where Adam's sign-like step on a noise-level gradient moves a weight (at most
      1e-4 of the weights, never more than 2 lr), and within 2e-5 relative L2; the step's clipped
      gradient within 2e-5 relative L2 (measured 2.2e-6), every entry within 1e-4 x max|g| and at
      most 1e-4 of them beyond 2e-5 x max|g| (measured: none).
      bf16 (against the
      bf16 emulation, oracle/cnn_ref.py bf16=True): loss 1e-4 of its scale, every step's clipped
      gradient within 2e-2 of the emulation's and under half its distance to the fp32 oracle's
      (the bars of test_cnn_bf16_update_step_vs_bf16_oracle, at every one of the 8 steps), and
      every step's new parameters: the Adam step on the device's gradient at the fp32 bars, and
      within 3 lr per weight / 0.5 of the update's norm of the emulation's own clip + Adam.
    * Free-running (oracle and device each on their own trajectory, measured 1e-4 loss and 8.5e-5
      parameter deviation after 8 fp32 steps on the first GPU run — Adam amplifies reassociation-level
      gradient differences of near-zero-gradient weights): fp32 losses within 5e-4 relative,
      parameters within 5e-4 relative L2."""
    from gsamd._lib import GS_HP_BF16, M, check, lib, ptr
    from gsamd.config import load_config
    from gsamd.ppo_agent import DevicePPOAgent
    from oracle import cnn_ref as C
    torch.manual_seed(3)
    cfg = load_config("ALE-Pong-v5", "rgb_ppo", overrides=dict(env_dynamics="synthetic", n_envs=32, n_steps=256,
                                                               n_epochs=1))
    agent = DevicePPOAgent(cfg, device=cuda, use_graph=False, track_stats=False)
    coll = agent.get_rollout_collector("train")
    coll.collect()
    B, K = agent.batch_size, agent.n_minibatches
    assert (B, K) == (1024, 8)
    idx = agent.prefetcher.upload(0)
    pm = agent.policy_model
    state = [t.clone() for t in (pm.params, agent.adam_m, agent.adam_v)]
    hp = agent.hparams()
    hp.flags = GS_HP_BF16 if prec == "bf16" else 0
    buf = coll.buffer
    s = torch.cuda.Stream(device=cuda)

    def run(n):
        check(lib.gs_cnn_ppo_update(ptr(pm.params), ptr(agent.grads), ptr(agent.adam_m), ptr(agent.adam_v), pm.dims,
                                    hp, buf.view(), ptr(idx), B, n, 0, ptr(agent.metrics_buf), ptr(agent.stop_flag),
                                    ptr(agent.workspace), None, s.cuda_stream), "gs_cnn_ppo_update")
    h_off = int(lib.gs_cnn_workspace_hidden_offset(pm.dims, B))
    HID = 512
    assert h_off >= 0 and h_off % 4 == 0 and h_off + 4 * B * HID <= agent.workspace.numel()
    assert int(lib.gs_cnn_workspace_act_offset(pm.dims, B, 4)) == h_off
    # the activations' NHWC shapes at 84 x 84 (conv1 20x20x32, conv2 9x9x64, conv3 7x7x64) and the fc
    act_shapes = [(20, 20, 32), (9, 9, 64), (7, 7, 64), (HID,)]
    act_offs = [int(lib.gs_cnn_workspace_act_offset(pm.dims, B, layer)) for layer in (1, 2, 3, 4)]

    def decisions():   # the last step's activations in the workspace -> its ReLU decisions (NCHW)
        out = []
        for off, sh in zip(act_offs, act_shapes):
            n = B * int(np.prod(sh))
            assert off >= 0 and off % 4 == 0 and off + 4 * n <= agent.workspace.numel()
            a = agent.workspace[off:off + 4 * n].view(torch.float32).view(B, *sh) > 0
            out.append((a.permute(0, 3, 1, 2) if len(sh) == 3 else a).cpu().numpy())
        return out

    def restore():
        for t, s0 in zip((pm.params, agent.adam_m, agent.adam_v), state):
            t.copy_(s0)
        agent.metrics_buf.zero_()
        agent.stop_flag.zero_()

    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        run(K)
    torch.cuda.synchronize()
    eager = [t.clone() for t in (pm.params, agent.adam_m, agent.adam_v, agent.metrics_buf)]
    # graph capture of the whole update (the first, eager call above set every kernel attribute)
    restore()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run(K)
    restore()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(("params", "adam_m", "adam_v", "records"), eager,
                          (pm.params, agent.adam_m, agent.adam_v, agent.metrics_buf)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"graph replay != eager: {name}"
    rec = eager[3].cpu().numpy()
    # the device's state after n = 0..K steps of the same call (prefix runs)
    to_ref = lambda t: pm.flat_to_reference(t).astype(np.float32)  # noqa: E731
    states, grads, masks = [tuple(to_ref(t) for t in state)], [None], [None]
    for n in range(1, K + 1):
        restore()
        torch.cuda.synchronize()               # the restore copies ran on the current stream, run on s
        with torch.cuda.stream(s):
            run(n)
        torch.cuda.synchronize()
        states.append(tuple(to_ref(t) for t in (pm.params, agent.adam_m, agent.adam_v)))
        grads.append(to_ref(agent.grads))      # step n's clipped gradient
        masks.append(decisions())              # step n's conv and fc ReLU decisions
        assert np.array_equal(agent.metrics_buf[:n].cpu().numpy().view(np.uint32), rec[:n].view(np.uint32)), n
    assert np.array_equal(states[K][0].view(np.uint32), to_ref(eager[0]).view(np.uint32))

    # the same rows on the host: env-major sample i = env * T + t -> row (t, env)
    T, N = cfg.n_steps, cfg.n_envs
    ii = idx.cpu().numpy().astype(np.int64)[:K * B]
    src = (ii % T) * N + ii // T
    flat = lambda x: x.reshape(T * N, *x.shape[2:]).cpu().numpy()  # noqa: E731
    rows = tuple(flat(x)[src] for x in (buf.obs, buf.actions, buf.logprobs, buf.values, buf.advantages, buf.returns))
    kw = dict(valid=cfg.valid_actions, clip=float(hp.clip_range), clip_vf=float(hp.clip_range_vf),
              vf_coef=float(hp.vf_coef), ent_coef=float(hp.ent_coef))
    lr = float(hp.lr)
    shapes = C.cnn_param_shapes()
    slots = [M[k] for k in ("grad_norm", "gn_backbone", "gn_mlp", "gn_policy_head", "gn_value_head")]
    rl = lambda a, b: float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b))  # noqa: E731
    worst = {"loss": 0.0, "norm": 0.0, "p_rel": 0.0, "p_off": 0, "p_max": 0.0, "emu_vs_f32": []}
    fails = []      # every step is evaluated and printed before the bars are applied

    def need(ok, what):
        if not ok:
            fails.append(what)
    for k in range(K):
        sl = slice(k * B, (k + 1) * B)
        p, m, v = states[k]
        bf = prec == "bf16"
        p_dev, g_dev = states[k + 1][0], grads[k + 1]
        fc_mask = conv_masks = None
        if not bf:
            # the device's conv and fc ReLU decisions; where they differ from the oracle's own, the
            # oracle's pre-activation must sit within rounding of zero
            dev = masks[k + 1]
            dec = C.relu_decisions(p, shapes, rows[0][sl], dev)
            worst.setdefault("relu_decisions_from_device", []).append([(n_, float(f"{r_:.2e}")) for n_, r_ in dec])
            for (n_, r_), cap, name in zip(dec, (32, 32, 32, 8), ("conv1", "conv2", "conv3", "fc")):
                need(n_ <= cap and r_ <= 1e-5, ("relu decisions", k, name, n_, r_))
            conv_masks, fc_mask = dev[:3], dev[3]
        loss, _, g, _, _ = C.loss_and_grads(p, shapes, *(x[sl] for x in rows), bf16=bf, fc_mask=fc_mask,
                                            conv_masks=conv_masks, **kw)
        p1, _, _, gc, _ = C.clip_and_adam(p, g, shapes, m, v, k + 1, lr)
        d_loss = abs(rec[k, M["loss"]] - loss) / max(1.0, abs(loss))
        worst["loss"] = max(worst["loss"], d_loss)
        if bf:
            _, _, g32, _, _ = C.loss_and_grads(p, shapes, *(x[sl] for x in rows), **kw)
            _, _, _, gc32, _ = C.clip_and_adam(p, g32, shapes, m, v, k + 1, lr)
            worst["emu_vs_f32"].append((round(rl(g_dev, gc), 5), round(rl(g_dev, gc32), 5)))
            need(d_loss < 1e-4, ("loss", k, float(rec[k, M["loss"]]), loss))
            # the step's new parameters (the bf16 mode's clip + Adam is fp32): (1) exactly the Adam
            # step (torch's single-tensor Adam, cnn_ref.clip_and_adam with no clipping) on the device's own
            # clipped gradient — 2e-6 except where Adam's sign-like step on a noise-level gradient
            # moves a weight (at most 1e-4 of them, never more than 2 lr); (2) against the emulation's
            # clip + Adam on ITS gradient (within 2e-2 of the device's, above): every weight within
            # 3 lr and the update p1 - p within 0.5 of its norm (Adam rescales each weight's step by
            # its own moment, so the gradient's relative difference reaches the update unevenly)
            pa = C.clip_and_adam(p, g_dev.astype(np.float32), shapes, m, v, k + 1, lr, max_norm=1e30)[0]
            d = np.abs(p_dev.astype(np.float64) - pa)
            du = np.linalg.norm((p_dev.astype(np.float64) - p) - (p1 - p)) / np.linalg.norm(p1.astype(np.float64) - p)
            de = float(np.abs(p_dev.astype(np.float64) - p1).max())
            worst.setdefault("bf16_params", []).append((int((d > 2e-6).sum()), float(f"{d.max():.2e}"),
                                                        float(f"{du:.3e}"), float(f"{de:.2e}")))
            need((d > 2e-6).sum() <= max(1, int(1e-4 * d.size)) and d.max() <= 2 * lr,
                 ("bf16 params vs Adam on the device gradient", k, int((d > 2e-6).sum()), float(d.max())))
            need(de <= 3 * lr and du < 0.5, ("bf16 params vs the emulation's clip + Adam", k, de, du))
            continue
        # the clipped gradient: at B = 1024 a few pre-activations sit within rounding of 0, so a
        # ReLU decision flips between the device's and the oracle's summation order and moves the
        # entries that unit feeds (first GPU run: 592 of 1.69 M beyond 2e-5 x max|g|, the largest
        # 1.1e-4 x max|g|); the rest agree to the single-step bar
        gm = np.abs(gc).max()
        dg = np.abs(g_dev.astype(np.float64) - gc)
        worst["g_off"] = max(worst.get("g_off", 0), int((dg > 2e-5 * gm).sum()))
        worst["g_rel"] = max(worst.get("g_rel", 0.0), rl(g_dev, gc))
        worst.setdefault("g_off_share", []).append(float((dg > 2e-5 * gm).mean()))
        o, blk = 0, {}                # where the off entries sit (parameter blocks), for the log
        for n_, sh in shapes:
            n_el = int(np.prod(sh))
            c_ = int((dg[o:o + n_el] > 2e-5 * gm).sum())
            if c_:
                blk[n_] = (c_, round(float(dg[o:o + n_el].max() / gm), 6))
            o += n_el
        worst.setdefault("g_off_blocks", []).append(blk)
        need((dg > 2e-5 * gm).sum() <= 1e-4 * dg.size and dg.max() <= 1e-4 * gm,
             ("grad entries", k, int((dg > 2e-5 * gm).sum()), float(dg.max() / gm)))
        need(rl(g_dev, gc) < 2e-5, ("grad rel L2", k, rl(g_dev, gc)))
        comp = {"cnn": 0.0, "mlp": 0.0, "policy_head": 0.0, "value_head": 0.0}
        o = 0
        for n_, sh in shapes:
            n_el = int(np.prod(sh))
            comp[n_.split(".")[0]] += float(np.sum(g[o:o + n_el].astype(np.float64) ** 2))
            o += n_el
        norms = np.array([np.sqrt(sum(comp.values()))] + [np.sqrt(comp[c]) for c in ("cnn", "mlp", "policy_head",
                                                                                      "value_head")])
        d_norm = float(np.max(np.abs(rec[k, slots] - norms) / norms))
        d = np.abs(p_dev.astype(np.float64) - p1)
        worst["norm"] = max(worst["norm"], d_norm)
        worst["p_rel"] = max(worst["p_rel"], rl(p_dev, p1))
        worst["p_off"] = max(worst["p_off"], int((d > 2e-6).sum()))
        worst["p_max"] = max(worst["p_max"], float(d.max()))
        need(d_loss < 1e-5, ("loss", k, float(rec[k, M["loss"]]), loss))
        need(d_norm < 1e-5, ("norms", k, d_norm))
        need((d > 2e-6).sum() <= max(1, int(1e-4 * d.size)) and d.max() <= 2 * lr,
             ("params entries", k, int((d > 2e-6).sum()), float(d.max())))
        need(rl(p_dev, p1) < 2e-5, ("params rel L2", k, rl(p_dev, p1)))
    print(f"{prec} teacher-forced: {worst}")
    assert not fails, fails
    if prec == "bf16":
        # each step's clipped gradient within 2e-2 of the emulation's and under half its distance
        # to the fp32 oracle's (test_cnn_bf16_update_step_vs_bf16_oracle's bars)
        assert all(e < 2e-2 and e < 0.5 * f for e, f in worst["emu_vs_f32"]), worst["emu_vs_f32"]
        return
    # free-running: the oracle on its own trajectory from the same start
    p, m, v = states[0]
    losses = []
    for k in range(K):
        sl = slice(k * B, (k + 1) * B)
        loss, _, g, _, _ = C.loss_and_grads(p, shapes, *(x[sl] for x in rows), **kw)
        p, m, v, _, _ = C.clip_and_adam(p, g, shapes, m, v, k + 1, lr)
        losses.append(loss)
    dl = np.abs(rec[:K, M["loss"]] - np.array(losses)) / np.maximum(1.0, np.abs(losses))
    print(f"fp32 free-running: loss dev {dl.max():.2e}, params rel L2 {rl(states[K][0], p):.2e}")
    assert dl.max() < 5e-4 and rl(states[K][0], p) < 5e-4


@pytest.mark.parametrize("tag", list(CASES))
def test_cnn_activation_stats_vs_reference(golden, cuda, tag):
    """gs_cnn_activation_stats against the reference's forward hooks on the same case
    (cnn_step.npz activation_names / values: utils/models.py:121-147 on cnn.0, cnn.2, cnn.4, mlp.0,
    the pre-activation outputs of each Conv2d / Linear): mean and std within 1e-5 of the layer's
    std, dead_pct / dead_max within one row (1 / B).  Also through the agent: the keys the
    reference records (opt/activations/<layer>/{mean,std,dead_pct,dead_max})."""
    from gsamd._lib import check, lib, ptr, stream_handle
    valid, clip, ent, lr, B, _, _ = CASES[tag]
    pm, p_ref, bufs, view, hp, idx, batch = _setup(cuda, tag)
    ws = torch.empty(int(lib.gs_cnn_workspace_bytes(pm.dims, B)), dtype=torch.uint8, device=cuda)
    out = torch.zeros(16, dtype=torch.float64, device=cuda)
    check(lib.gs_cnn_activation_stats(ptr(pm.params), pm.dims, view, ptr(idx), B, ptr(out), ptr(ws), stream_handle()),
          "gs_cnn_activation_stats")
    torch.cuda.synchronize()
    dev = out.cpu().numpy()
    z = golden("cnn_step.npz")
    ref = dict(zip([str(x) for x in z[f"{tag}/activation_names"]], z[f"{tag}/activation_values"]))
    layers = ("cnn.0", "cnn.2", "cnn.4", "mlp.0")
    assert set(ref) == {f"opt/activations/{n}/{k}" for n in layers for k in ("mean", "std", "dead_pct", "dead_max")}
    for li, n in enumerate(layers):
        sd = ref[f"opt/activations/{n}/std"]
        for ki, k in enumerate(("mean", "std", "dead_pct", "dead_max")):
            want, got = ref[f"opt/activations/{n}/{k}"], dev[4 * li + ki]
            tol = 1e-5 * sd if k in ("mean", "std") else 1.0 / B + 1e-9
            assert abs(got - want) <= tol, (n, k, got, want)


def _cnn_stats_update(cuda, env, over, n_up):
    """A pixel agent with its first rollout collected; run(k) restores the initial state and runs the
    first k minibatches of the update (gs_cnn_ppo_update with the agent's hparams, GS_HP_ACT_STATS
    included), returning the records."""
    from gsamd._lib import check, lib, ptr, stream_handle
    from gsamd.config import load_config
    from gsamd.ppo_agent import DevicePPOAgent
    torch.manual_seed(0)
    cfg = load_config(env, "rgb_ppo", overrides=dict(env_dynamics="synthetic", **over))
    agent = DevicePPOAgent(cfg, device=cuda, use_graph=False, track_stats=True)
    assert agent.device_activation_stats
    coll = agent.get_rollout_collector("train")
    coll.collect()
    idx = agent.prefetcher.upload(0)
    pm = agent.policy_model
    st0 = [t.clone() for t in (pm.params, agent.adam_m, agent.adam_v)]

    def run(k):
        for t, t0 in zip((pm.params, agent.adam_m, agent.adam_v), st0):
            t.copy_(t0)
        agent.metrics_buf.zero_()
        if k:
            check(lib.gs_cnn_ppo_update(ptr(pm.params), ptr(agent.grads), ptr(agent.adam_m), ptr(agent.adam_v), pm.dims,
                                        agent.hparams(), coll.buffer.view(), ptr(idx), agent.batch_size, k, 0,
                                        ptr(agent.metrics_buf), ptr(agent.stop_flag), ptr(agent.workspace), None,
                                        stream_handle()), "gs_cnn_ppo_update")
        torch.cuda.synchronize()
        return agent.metrics_buf[:k].cpu().numpy().copy()

    def ref_stats(k):    # gs_cnn_activation_stats (separate fp32 forward) before step k
        run(k)
        out = torch.zeros(16, dtype=torch.float64, device=cuda)
        check(lib.gs_cnn_activation_stats(ptr(pm.params), pm.dims, coll.buffer.view(), ptr(idx[k * agent.batch_size:]),
                                          agent.batch_size, ptr(out), ptr(agent.workspace), stream_handle()),
              "gs_cnn_activation_stats")
        torch.cuda.synchronize()
        return out.cpu().numpy()
    return agent, run, ref_stats


def test_cnn_agent_records_activation_stats(cuda):
    """The pixel agent records the NatureCNN's activation statistics under the reference's keys
    (base_agent.py:335-347 -> opt/activations/{cnn.0,cnn.2,cnn.4,mlp.0}/*) as the epoch mean over
    every minibatch of the update, each taken under the parameters that minibatch's loss used (the
    reference's per-training_step hook record): at B = 64 the update computes them with the separate
    fp32 forward (gs_cnn_activation_stats' kernels) before each step, so every minibatch's values are
    those of gs_cnn_activation_stats on its rows and pre-step parameters, bit for bit."""
    from gsamd._lib import ACT_SLOT
    agent, run, ref_stats = _cnn_stats_update(cuda, "ALE-Breakout-v5", dict(n_envs=8, n_steps=32, batch_size=64,
                                                                           n_epochs=1), 4)
    n = agent.n_minibatches
    assert n == 4
    rec = run(n)
    for k in range(n):
        np.testing.assert_array_equal(rec[k, ACT_SLOT:ACT_SLOT + 16], ref_stats(k).astype(np.float32), err_msg=str(k))
    # through the agent's epoch bookkeeping: the epoch means of those records
    run(0)
    agent.update_phase()
    m = agent.epoch_metrics()
    keys = agent.activation_keys()
    assert len(keys) == 16 and set(keys) <= set(m)
    want = rec[:, ACT_SLOT:ACT_SLOT + 16].astype(np.float64).mean(axis=0)
    np.testing.assert_allclose(np.array([m[k] for k in keys]), want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_cnn_update_activation_stats_epilogues(cuda, prec):
    """The production batch (B = 1024, Pong): the statistics come from the update's own forward
    kernels (the conv1 / conv2 / conv3 LDS convolutions' and the fc kernel's epilogues: integer dead
    counters, per-wave sums), for every minibatch under the parameters its loss used.  Against
    gs_cnn_activation_stats (a separate fp32 forward) on the same rows and pre-step parameters: fp32
    mean / std within 1e-5 x std (+ 1e-7), dead fractions within 1/B; bf16 (the forward's operands
    rounded to bf16) mean / std within 2e-2 x std, dead fractions within 4/B."""
    from gsamd._lib import ACT_SLOT
    over = dict(n_envs=32, n_steps=32, n_epochs=3)
    if prec == "bf16":
        over["precision"] = "bf16"
    agent, run, ref_stats = _cnn_stats_update(cuda, "ALE-Pong-v5", over, 3)
    B, n = agent.batch_size, agent.n_minibatches
    assert B == 1024 and n == 3
    rec = run(n)
    rtol, dtol = (1e-5, 1.0 / B) if prec == "fp32" else (2e-2, 4.0 / B)
    for k in range(n):
        ref, got = ref_stats(k), rec[k, ACT_SLOT:ACT_SLOT + 16].astype(np.float64)
        for l in range(4):
            sd = ref[4 * l + 1]
            for j in range(4):
                tol = rtol * sd + 1e-7 if j < 2 else dtol
                assert abs(got[4 * l + j] - ref[4 * l + j]) <= tol, (prec, k, l, j, got[4 * l + j], ref[4 * l + j])
    assert np.isfinite(rec[:, ACT_SLOT:ACT_SLOT + 16]).all() and (rec[:, ACT_SLOT + 1::4] > 0).all()
