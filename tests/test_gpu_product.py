"""The shipped Python surface (mebt.transformer.Net2NetTransformer & friends, backed by
libmebt_hip.so) against the golden vectors of the reference: forward, loss/accuracy, the sampling
loops (bit-exact token ids for identical noise) and three optimiser steps.  GPU only."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import closed_form as cf
from oracle import mebt_oracle as orc
from tests.golden import make_golden as mg
from tests.helpers import load_golden, build_product, closed_form_hook, assert_same_trajectory

DEV = "cuda"


@pytest.mark.parametrize("name", ["c1", "micro_budget"])
def test_module_forward_and_shared_step(name):
    g = load_golden("forward_" + name)
    model = build_product(name, "f32")
    x, idx = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["indices"]).to(DEV)
    for c, (mode, t) in enumerate(zip(g["case_mode"], g["case_t"])):
        model.train(mode == "train")
        with torch.no_grad():
            logits, z_t, ntw, seq_len = model(x, None, t=float(t), indices=idx)
        meta = g[f"c{c}_meta"]
        assert (z_t.cpu().numpy() == g[f"c{c}_z_targets"]).all()
        assert ntw == meta[0] and seq_len == meta[1]
        np.testing.assert_allclose(logits.cpu()[..., g["cols"]].numpy(), g[f"c{c}_cols"], atol=1e-4, rtol=0)
        # shared_step (fused loss + top-1/top-5) with the python RNG draw forced to t
        import random
        orig = random.random
        random.random = lambda: float(t)
        try:
            with torch.no_grad():
                a1, a5, loss, ratio = model.shared_step({"video": x, "indices": idx}, 0)
        finally:
            random.random = orig
        assert abs(float(loss) - meta[2]) < 2e-5 * abs(meta[2])
        assert abs(float(a1) - meta[3]) < 1e-3 and abs(float(a5) - meta[4]) < 1e-3


def test_state_dict_roundtrip_and_names():
    model = build_product("micro", "f32")
    sd = model.state_dict()
    shapes = orc.param_shapes(mg.oracle_cfg("micro"))
    assert set(sd.keys()) == set(shapes.keys())                      # SURVEY.md §A.2 schema
    ref = cf.state_dict_numpy(shapes)
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(shapes[k]) and np.array_equal(v.cpu().numpy(), ref[k]), k


def test_sample_loops_bit_exact():
    g = load_golden("sample_loops")
    for i, (strategy, sched, run) in enumerate(zip(g["run_strategy"], g["run_schedule"], g["runs"])):
        n_steps, temp, k, p, ctemp = run
        model = build_product("micro", "f32", schedule=str(sched)).eval()
        hook, state = closed_form_hook()
        model.noise_hook = hook
        x = torch.zeros(2, 2, 4, 4, dtype=torch.long, device=DEV)
        xs, ci, ti = model.sample(x, None, float(temp), None if k < 0 else int(k), None if p < 0 else float(p), int(n_steps),
                                  None, None, strategy=str(strategy), context_temperature=float(ctemp), skips=False)
        assert state["k"] == int(g[f"r{i}_ndraws"]), (i, state["k"])
        assert (xs.cpu().numpy() == g[f"r{i}_x"]).all(), i
        assert (ci.cpu().numpy() == g[f"r{i}_ci"]).all() and (ti.cpu().numpy() == g[f"r{i}_ti"]).all(), i
    # continuation from given index sets
    model = build_product("micro", "f32", schedule="cosine").eval()
    hook, _ = closed_form_hook()
    model.noise_hook = hook
    idx = torch.from_numpy(g["cont_idx"]).to(DEV)
    xs, ci, ti = model.sample(torch.from_numpy(g["cont_x0"]).to(DEV), None, 1.0, None, None, 4, idx[:, :10], idx[:, 10:],
                              context_temperature=3.0, skips=False)
    assert (xs.cpu().numpy() == g["cont_x"]).all() and (ci.cpu().numpy() == g["cont_ci"]).all() and (ti.cpu().numpy() == g["cont_ti"]).all()


def test_draft_and_revise_bit_exact():
    g = load_golden("sample_loops")
    opt = lambda v, f: None if v < 0 else f(v)
    for i, r in enumerate(g["dnr"]):
        model = build_product("micro", "f32").eval()
        hook, state = closed_form_hook()
        model.noise_hook = hook
        xs = model.draft_and_revise(torch.from_numpy(g[f"d{i}_x0"]).to(DEV), None, int(r[0]), float(r[1]), opt(r[2], int),
                                    opt(r[3], float), int(r[4]), float(r[5]), opt(r[6], int), opt(r[7], float), int(r[8]), bool(r[9]))
        assert state["k"] == int(g[f"d{i}_ndraws"])
        assert (xs.cpu().numpy() == g[f"d{i}_x"]).all(), i


def test_edit_mode_sample_and_draft_and_revise_bit_exact():
    """`edit=True` (reference transformer.py:373-376,399: the mask schedule counts only the edited tokens; :658-660: the revise
    passes of draft_and_revise drop the caller's index sets) against vectors from the imported reference."""
    g = load_golden("edit_beta_priors")
    model = build_product("micro", "f32", schedule="cosine").eval()
    hook, state = closed_form_hook()
    model.noise_hook = hook
    idx = torch.from_numpy(g["edit_idx"]).to(DEV)
    xs, ci, ti = model.sample(torch.from_numpy(g["edit_x0"]).to(DEV), None, 1.0, None, None, 5, idx[:, :12], idx[:, 12:],
                              context_temperature=3.0, skips=False, edit=True)
    assert state["k"] == int(g["edit_ndraws"])
    assert (xs.cpu().numpy() == g["edit_x"]).all() and (ci.cpu().numpy() == g["edit_ci"]).all() and (ti.cpu().numpy() == g["edit_ti"]).all()
    # the same call without edit=True takes different steps (the schedule then counts all N tokens): the flag is live
    hook2, _ = closed_form_hook()
    model.noise_hook = hook2
    xs2, ci2, _ = model.sample(torch.from_numpy(g["edit_x0"]).to(DEV), None, 1.0, None, None, 5, idx[:, :12], idx[:, 12:],
                               context_temperature=3.0, skips=False, edit=False)
    assert ci2.shape != ci.shape or not (xs2.cpu().numpy() == g["edit_x"]).all()
    model = build_product("micro", "f32").eval()
    hook, state = closed_form_hook()
    model.noise_hook = hook
    idx = torch.from_numpy(g["edit_dnr_idx"]).to(DEV)
    xs = model.draft_and_revise(torch.from_numpy(g["edit_dnr_x0"]).to(DEV), None, 4, 1.0, None, None, 4, 0.7, None, None, 2, False, False,
                                idx[:, :16], idx[:, 16:], True)
    assert state["k"] == int(g["edit_dnr_ndraws"])
    assert (xs.cpu().numpy() == g["edit_dnr_x"]).all()


def test_beta_schedule_training_forward():
    """beta(t) schedule (reference transformer.py:113-119,229-241): at each global step the module hands the reference's (alpha,
    beta) to torch's Beta, and the train-mode shared_step with the drawn t gives the reference's loss / accuracies."""
    import torch.distributions.beta as tdb
    g = load_golden("edit_beta_priors")
    model = build_product("micro", "f32", beta_params=[3.0, 9.0], beta_iter=1000).train()
    calls, forced = [], list(g["beta_forced_t"])

    class FakeBeta:
        def __init__(self, a, b):
            calls.append((float(a), float(b)))

        def sample(self):
            return torch.tensor(forced[len(calls) - 1])
    real = tdb.Beta
    tdb.Beta = torch.distributions.beta.Beta = FakeBeta
    try:
        for s, gs in enumerate(g["beta_gsteps"]):
            model.global_step = int(gs)
            x, idx = torch.from_numpy(g[f"beta{s}_x"]).to(DEV), torch.from_numpy(g[f"beta{s}_indices"]).to(DEV)
            with torch.no_grad():
                acc1, acc5, loss, ratio = model.shared_step({"video": x, "label": x, "indices": idx}, 0)
            meta = g["beta_meta"][s]
            assert abs(float(loss) - meta[0]) < 2e-5 * abs(meta[0]) and abs(float(acc1) - meta[1]) < 1e-3 and abs(float(acc5) - meta[2]) < 1e-3
            assert abs(float(ratio) - meta[3]) < 1e-7
    finally:
        tdb.Beta = torch.distributions.beta.Beta = real
    np.testing.assert_allclose(np.array(calls), g["beta_calls"], rtol=0, atol=0)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_windowed_train_step_c1(dtype):
    """The video-length curriculum on the GPU (every 128-frame config trains this way): t_prior = gaussian2, the mask sampler's
    two numpy draws forced to a window of T = 1 of 2 latent frames starting at frame 1, so seq_len = 64 < N = 128
    (reference transformer.py:243-245, mask_sampler.py:83-99) — one optimizer step of the HIP engine on C1 against the
    imported reference: the prior handed to np.random.choice, loss, every gradient norm / probe, post-step parameter norms."""
    from mebt_amd.trainer import TrainLoop
    g = load_golden("train_window_c1")
    names = [str(n) for n in g["names"]]
    model = build_product("c1", dtype, t_prior="gaussian2").train()
    model.learning_rate, model.weight_decay, model.warmup_steps, model.cosine_lr = 1e-3, 0.05, 0, False
    model.global_step = int(g["global_step"])
    loop = TrainLoop(model, fused_optimizer=False)
    rec = {}
    real_choice, real_randint = np.random.choice, np.random.randint

    def fake_choice(a, p=None, **kw):
        rec["a"], rec["p"] = np.asarray(a).copy(), np.asarray(p).copy()
        return 1

    def fake_randint(lo, hi=None, **kw):
        rec["randint"] = (lo, hi)
        return 1
    np.random.choice, np.random.randint = fake_choice, fake_randint
    try:
        stats = loop.step(torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["indices"]).to(DEV), t=float(g["t"])).cpu().numpy()
    finally:
        np.random.choice, np.random.randint = real_choice, real_randint
    assert list(rec["a"]) == list(g["choice_a"]) and tuple(rec["randint"]) == tuple(g["randint"])
    np.testing.assert_allclose(rec["p"], g["choice_p"], rtol=1e-12)
    tol = 1.0 if dtype == "f32" else 60.0
    assert int(stats[3]) == 3 * 39
    assert abs(stats[4] - g["meta"][0]) < tol * 5e-5 * abs(g["meta"][0]), (stats[4], g["meta"][0])
    nm = loop.native
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    grads = nm.views(shapes, grads=True)
    gn = np.array([float(grads[n].double().norm()) for n in names])
    np.testing.assert_allclose(gn, g["gradnorm"], rtol=tol * 5e-4, atol=1e-7 * tol)
    if dtype == "f32":
        probe = g["probe"]
        gp = np.stack([grads[n].reshape(-1)[torch.from_numpy(probe % grads[n].numel()).to(DEV)].cpu().numpy() for n in names])
        np.testing.assert_allclose(gp, g["gprobe"], atol=3e-6, rtol=5e-3)
        sd = model.state_dict()
        pn = np.array([float(sd[n].double().norm()) for n in names])
        np.testing.assert_allclose(pn, g["pnorm"], rtol=2e-5)


def test_script_drivers_bit_exact():
    """bidirect_sample / extrapolate (sample_vqgan_transformer_videos.py:22-157) against vectors produced by
    the reference script's own functions (tests/golden/make_golden.py:gen_script_drivers)."""
    from mebt_amd.sampling import bidirect_sample, extrapolate
    g = load_golden("script_drivers")
    model = build_product("micro", "f32", schedule="cosine").eval()
    hook, state = closed_form_hook()
    model.noise_hook = hook
    log = bidirect_sample(model, 2, 8, 8, 4, temperature=1.0, top_k=None, top_p=None, vid_n_steps=4, vid_c_temp=3.0,
                          ctemp_schedule='linear', strategy='maskgit', bootstrap=3)
    assert state["k"] == int(g["bi_ndraws"]) and (log["code_maps"].cpu().numpy() == g["bi_code_maps"]).all()
    np.testing.assert_allclose(log["score"].cpu().numpy(), g["bi_score"], rtol=1e-4)
    assert "samples" not in log and log["class_label"].shape == (2, 1)
    hook, state = closed_form_hook()
    model.noise_hook = hook
    log = bidirect_sample(model, 2, 8, 8, 4, temperature=0.9, top_k=64, top_p=None, vid_n_steps=3, vid_c_temp=2.0)
    assert state["k"] == int(g["bi2_ndraws"]) and (log["code_maps"].cpu().numpy() == g["bi2_code_maps"]).all()
    np.testing.assert_allclose(log["score"].cpu().numpy(), g["bi2_score"], rtol=1e-4)
    hook, state = closed_form_hook()
    model.noise_hook = hook
    log = extrapolate(model, torch.from_numpy(g["ex_vq0"]).to(DEV), 16, 8, 4, temperature=1.0, vid_n_steps=3, vid_c_temp=2.5)
    assert state["k"] == int(g["ex_ndraws"]) and (log["code_maps"].cpu().numpy() == g["ex_code_maps"]).all()
    # sliding-window continuation: equals the oracle driven by the same noise
    hook, _ = closed_form_hook()
    model.noise_hook = hook
    log = bidirect_sample(model, 2, 16, 8, 4, vid_n_steps=3, vid_c_temp=2.0)
    noise_fn, _, _ = mg.oracle_noise_fns()
    cfg = mg.oracle_cfg("micro", schedule="cosine")
    with torch.no_grad():
        cm, score = orc.bidirect_sample(orc.closed_form_params(cfg), cfg, 2, 16, 8, 4, 1.0, None, None, 3, 2.0, noise_fn)
    assert (log["code_maps"].cpu() == cm).all()
    np.testing.assert_allclose(log["score"].cpu().numpy(), score.numpy(), rtol=1e-4)


def test_sampling_command_lines_micro_golden(tmp_path, monkeypatch):
    """`python -m mebt_amd.sample` then `python -m mebt_amd.draft_and_revise --np_draft <its codemap>` (the two stages of the shipped
    pipelines, reference sample_vqgan_transformer_videos.py:160-297 / draft_and_revise_videos.py:64-198) on a Lightning-format
    checkpoint of the micro model: the code map file of the first equals the reference script's own output
    (tests/golden/script_drivers.npz), the second equals the oracle's draft_and_revise(skip_draft=True) on that draft."""
    from mebt_amd import sample as sample_cli, draft_and_revise as dnr_cli, scripts_common
    g = load_golden("script_drivers")
    model = build_product("micro", "f32", schedule="linear", device="cpu")
    ckpt = str(tmp_path / "micro.ckpt")
    torch.save({"state_dict": model.state_dict(), "hyper_parameters": model.hparams, "global_step": 11, "epoch": 0}, ckpt)
    monkeypatch.chdir(tmp_path)
    real_load = scripts_common.load_model
    hooks = []

    def load_with_noise(args):
        m = real_load(args)
        hook, state = closed_form_hook()
        m.noise_hook = hook
        hooks.append(state)
        return m

    monkeypatch.setattr(sample_cli, "load_model", load_with_noise)
    monkeypatch.setattr(dnr_cli, "load_model", load_with_noise)
    out = sample_cli.main(f"--gpt_ckpt {ckpt} --exp_name micro --dtype f32 --batch_size 2 --n_sample 1 --total_length 8 --step_size 8 --context_size 4 "
                          "--temp 1.0 --vid_n_steps 4 --vid_c_temp 3.0 --bootstrap 3 --no_phase --save_codemap --no_np --dataset stl -v".split())
    assert out == "results/micro/numpy_files_8/stl/VID_n_steps4_temp1.0_ctemp3.0linear_maskgit_cosine_no_phase_run0"
    code = np.load(out + "_codemap.npy")
    assert code.shape == (1, 2, 4, 4) and hooks[0]["k"] == int(g["bi_ndraws"])          # --n_sample 1 of the batch of 2 (:279)
    assert (code == g["bi_code_maps"][:1]).all()
    # --base_np: `extrapolate` of given code maps (reference :262-273), against the reference script's own output
    base_np = str(tmp_path / "base_codes.npy")
    np.save(base_np, g["ex_vq0"])
    out_ex = sample_cli.main(f"--gpt_ckpt {ckpt} --exp_name micro --dtype f32 --batch_size 2 --n_sample 2 --total_length 16 --step_size 8 --context_size 4 "
                             f"--temp 1.0 --vid_n_steps 3 --vid_c_temp 2.5 --base_np {base_np} --no_phase --save_codemap --no_np --dataset stl --run 1".split())
    code_ex = np.load(out_ex + "_codemap.npy")
    assert hooks[-1]["k"] == int(g["ex_ndraws"]) and (code_ex == g["ex_code_maps"]).all()
    full = str(tmp_path / "VID_n_steps4_maskgit_cosine_ctemp3.0_draft_codemap.npy")
    np.save(full, g["bi_code_maps"])
    out2 = dnr_cli.main(f"--gpt_ckpt {ckpt} --exp_name micro --dtype f32 --batch_size 2 --n_sample 2 --total_length 8 --step_size 8 --context_size 8 "
                        f"--n_revise 2 --M 2 --revise_t 0.8 --np_draft {full} --save_codemap --dataset stl --no_phase".split())
    assert out2 == "results/micro/numpy_files_8/stl/VID_dnr_nd4_dt0.0_nr2_rt0.8_M2_ctemp3.0_run0"
    assert open(out2 + ".txt").read() == full
    code2 = np.load(out2 + "_codemap.npy")
    noise_fn, perm_fn, _ = mg.oracle_noise_fns()
    cfg = mg.oracle_cfg("micro")
    with torch.no_grad():
        ref = orc.draft_and_revise(orc.closed_form_params(cfg), cfg, torch.from_numpy(g["bi_code_maps"]), 4, 0.0, None, None, 2, 0.8, None, None, 2, True,
                                   perm_fn, noise_fn)
    assert code2.shape == (2, 2, 4, 4) and (code2.reshape(2, -1) == ref.numpy()).all()


def test_encode_to_c_is_the_sos_pair():
    """reference transformer.py:696-701 with the only conditioning stage there is (SOSProvider, :204-212)"""
    model = build_product("micro", "f32").eval()
    x = torch.zeros(3, 2, 4, 4, dtype=torch.long, device=DEV)
    q, idx = model.encode_to_c(x)
    assert q.shape == (3, 1) and idx.shape == (3, 1) and q.dtype == torch.long and int(idx.abs().sum()) == 0 and idx.device == x.device


def test_sample_debug_tuple_and_gpt_forward_boundary():
    model = build_product("micro", "f32", schedule="cosine").eval()
    hook, _ = closed_form_hook()
    model.noise_hook = hook
    x = torch.zeros(2, 2, 4, 4, dtype=torch.long, device=DEV)
    out = model.sample(x, None, 1.0, None, None, 4, None, None, context_temperature=2.0, skips=False, debug=True)
    assert len(out) == 6 and out[5].shape == (2, 32, 16384) and len(out[3]) == len(out[4]) + 1
    # GPT.forward on embedded inputs == oracle
    cfg = mg.oracle_cfg("micro")
    P = orc.closed_form_params(cfg)
    xx, idx = mg.inputs("micro", 2, "gptfwd")
    ci, ti = idx[:, :9], idx[:, 9:]
    sos, ctx, tgt = orc.embed(P, cfg, xx.reshape(2, -1), ci, ti)
    ref = orc.gpt_forward(P, cfg, sos, ctx, tgt)
    got, _ = model.transformer(sos.to(DEV), ctx.to(DEV), tgt.to(DEV), None, 0.)
    np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), atol=1e-4, rtol=0)


@pytest.mark.parametrize("name", ["micro", "micro_budget"])
@pytest.mark.parametrize("path", ["fused", "reference_style"])
def test_lightning_style_training_steps(name, path):
    """training_step -> loss.backward() -> optimizer_step, as the Lightning loop drives the
    reference; 'reference_style' computes F.cross_entropy on the returned logits exactly like
    reference shared_step (transformer.py:722-730) and lets autograd call the HIP backward."""
    import random
    import torch.nn.functional as F
    g = load_golden("train_" + name)
    model = build_product(name, "f32").train()
    model.learning_rate, model.weight_decay = float(g["lr"]), float(g["wd"])
    opt = model.configure_optimizers()
    assert [len(grp["params"]) for grp in opt.param_groups] == list(g["group_sizes"])
    assert [grp["weight_decay"] for grp in opt.param_groups] == list(g["group_wd"])
    names = [str(n) for n in g["names"]]
    for s, t in enumerate(g["ts"]):
        x, idx = torch.from_numpy(g[f"s{s}_x"]).to(DEV), torch.from_numpy(g[f"s{s}_indices"]).to(DEV)
        orig = random.random
        random.random = lambda: float(t)
        try:
            if path == "fused":
                loss = model.training_step({"video": x, "indices": idx}, 0)
            else:
                logits, target, ntw, seq_len = model(x, None, indices=idx)
                B = logits.shape[0]
                ce = F.cross_entropy(logits.reshape(-1, logits.size(-1)), target.reshape(-1), reduction='sum',
                                     label_smoothing=model.label_smoothing)
                loss = ce / (B * seq_len * (ntw / float(seq_len)) ** model.config.avg_loss)
        finally:
            random.random = orig
        loss.backward()
        meta = g[f"s{s}_meta"]
        assert abs(float(loss) - meta[0]) < 5e-5 * abs(meta[0]), (s, float(loss), meta[0])
        sd = dict(model.named_parameters())
        gn = np.array([float(sd[n].grad.double().norm()) for n in names])
        np.testing.assert_allclose(gn, g[f"s{s}_gradnorm"], rtol=2e-3, atol=1e-6)
        model.optimizer_step(optimizer=opt)
        model.trainer.global_step += 1
        pn = np.array([float(sd[n].detach().double().norm()) for n in names])
        np.testing.assert_allclose(pn, g[f"s{s}_pnorm"], rtol=2e-5)


@pytest.mark.parametrize("name", ["micro", "micro_budget"])
@pytest.mark.parametrize("overlap", [False, True])
def test_trainloop_steps_vs_golden(name, overlap):
    """TrainLoop (what bench.py and the launcher drive): loss and parameter norms after each step equal the
    reference's (tests/golden/train_*.npz); with `overlap_optimizer` the bucket-wise `mebt_adamw_range` calls
    on the optimizer stream must give the same parameters as the single `mebt_adamw_step` (not bitwise: the
    embedding gradients are accumulated with float atomics, whose order differs from run to run)."""
    from mebt_amd.trainer import TrainLoop
    g = load_golden("train_" + name)
    names = [str(n) for n in g["names"]]
    finals = []
    for ov in ([False, True] if overlap else [False]):
        model = build_product(name, "f32").train()
        model.learning_rate, model.weight_decay, model.warmup_steps, model.cosine_lr = float(g["lr"]), float(g["wd"]), 0, False
        loop = TrainLoop(model, overlap_optimizer=ov)
        for s, t in enumerate(g["ts"]):
            x, idx = torch.from_numpy(g[f"s{s}_x"]).to(DEV), torch.from_numpy(g[f"s{s}_indices"]).to(DEV)
            stats = loop.step(x, idx, t=float(t)).cpu().numpy()
            meta = g[f"s{s}_meta"]
            assert abs(stats[4] - meta[0]) < 5e-5 * abs(meta[0]), (s, stats[4], meta[0])
            sd = model.state_dict()
            pn = np.array([float(sd[n].double().norm()) for n in names])
            np.testing.assert_allclose(pn, g[f"s{s}_pnorm"], rtol=2e-5)
        finals.append({k: v.clone() for k, v in model.state_dict().items()})
    if overlap:
        for k in finals[0]:
            assert_same_trajectory(finals[0][k], finals[1][k], k, lr=float(g["lr"]))


@pytest.mark.parametrize("name", ["micro", "micro_budget"])
def test_trainloop_fused_optimizer(name):
    """Optimizer-in-backward (`mebt_model_set_fused_adamw`): in fp32 the three steps still match the reference's
    golden losses / parameter norms; in bf16 the fused epilogue gives the same parameters, moments and bf16 mirror
    as the separate AdamW pass (same math on the same fp32 gradient values)."""
    from mebt_amd.trainer import TrainLoop
    g = load_golden("train_" + name)
    names = [str(n) for n in g["names"]]
    model = build_product(name, "f32").train()
    model.learning_rate, model.weight_decay, model.warmup_steps, model.cosine_lr = float(g["lr"]), float(g["wd"]), 0, False
    loop = TrainLoop(model, fused_optimizer=True)
    assert loop.fused_optimizer
    for s, t in enumerate(g["ts"]):
        x, idx = torch.from_numpy(g[f"s{s}_x"]).to(DEV), torch.from_numpy(g[f"s{s}_indices"]).to(DEV)
        stats = loop.step(x, idx, t=float(t)).cpu().numpy()
        assert abs(stats[4] - g[f"s{s}_meta"][0]) < 5e-5 * abs(g[f"s{s}_meta"][0])
        sd = model.state_dict()
        np.testing.assert_allclose(np.array([float(sd[n].double().norm()) for n in names]), g[f"s{s}_pnorm"], rtol=2e-5)
    finals = []
    for fused in (False, True):
        model = build_product(name, "bf16").train()
        model.learning_rate, model.weight_decay, model.warmup_steps, model.cosine_lr = float(g["lr"]), float(g["wd"]), 0, False
        loop = TrainLoop(model, fused_optimizer=fused)
        assert loop.fused_optimizer == fused
        for s, t in enumerate(list(g["ts"]) + [0.0]):                 # + a step with NC = 0 (empty key-side reductions)
            s = min(s, len(g["ts"]) - 1)
            x, idx = torch.from_numpy(g[f"s{s}_x"]).to(DEV), torch.from_numpy(g[f"s{s}_indices"]).to(DEV)
            loop.step(x, idx, t=float(t))
        nm = loop.native
        torch.cuda.synchronize()
        finals.append([nm.W.clone(), nm.P.clone(), nm.Wlp.clone().float(), nm.adam[0].clone(), nm.adam[1].clone()])
    for a, b, what in zip(finals[0], finals[1], ("W", "P", "bf16 mirror", "exp_avg", "exp_avg_sq")):
        assert_same_trajectory(a, b, what, lr=float(g["lr"]))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_fused_cross_entropy_forward_and_gradient(dtype, monkeypatch):
    """`mebt_loss_with_grad` (loss statistics + d loss / d logits from one pass over the logits, the default of `TrainLoop.step`)
    against the separate cross-entropy forward / backward kernels (`MEBT_FUSED_CE=0`): the same expressions in the same summation
    order, so statistics and parameters after three steps agree to fp32 rounding (measured: 2.6e-8 on the weights; the compiler
    contracts the two kernels' arithmetic differently), incl. a run with gradient accumulation."""
    from mebt_amd.trainer import TrainLoop
    g = load_golden("train_micro")
    finals = []
    for fused in ("1", "0"):
        monkeypatch.setenv("MEBT_FUSED_CE", fused)
        for accum in (1, 2):
            model = build_product("micro", dtype).train()
            model.learning_rate, model.weight_decay, model.warmup_steps, model.cosine_lr = float(g["lr"]), float(g["wd"]), 0, False
            loop = TrainLoop(model, fused_optimizer=False, accumulate_grad_batches=accum)
            stats = []
            for s, t in enumerate(g["ts"]):
                x, idx = torch.from_numpy(g[f"s{s}_x"]).to(DEV), torch.from_numpy(g[f"s{s}_indices"]).to(DEV)
                stats.append(loop.step(x, idx, t=float(t)).cpu())
            torch.cuda.synchronize()
            nm = loop.native
            finals.append((fused, accum, torch.stack(stats), nm.W.clone(), nm.P.clone()))
    for a, b in ((finals[0], finals[2]), (finals[1], finals[3])):
        assert a[1] == b[1] and a[0] != b[0]
        assert (a[2] - b[2]).abs().max() <= 1e-6 * a[2].abs().max(), (a[1], a[2], b[2])
        tol = 1e-6 if dtype == "f32" else 2e-5                      # bf16 engine: a last-bit difference in dlogits can flip a bf16 rounding downstream
        assert (a[3] - b[3]).abs().max() <= tol * a[3].abs().max() and (a[4] - b[4]).abs().max() <= tol * max(1.0, float(a[4].abs().max())), (a[1], (a[3] - b[3]).abs().max())


def test_launcher_trains_from_token_file(tmp_path):
    """`python -m mebt_amd.train` (counterpart of train_transformer.py) on a token file in the reference's vtokens
    container layout: runs, logs finite losses, writes a Lightning-layout checkpoint that loads back."""
    import subprocess, sys, os, re
    rs = np.random.RandomState(3)
    lens = [5, 9, 4, 7, 12, 6]
    idx = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    f = str(tmp_path / "tok.npz")
    np.savez(f, train_data=rs.randint(0, 16384, size=(int(idx[-1]), 8, 8)).astype(np.int64), train_idx=idx,
             test_data=rs.randint(0, 16384, size=(6, 8, 8)).astype(np.int64), test_idx=np.array([0, 6], np.int64))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "mebt_amd.train", "--preset", "tiny", "--tokens", f, "--max_steps", "6", "--log_every", "2",
                          "--ckpt_every", "6", "--default_root_dir", str(tmp_path / "runs")], cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    losses = [float(v) for v in re.findall(r"train/loss ([0-9.]+)", out.stdout)]
    assert len(losses) == 3 and all(np.isfinite(losses)) and losses[0] < 12.0, out.stdout
    ck = torch.load(str(tmp_path / "runs" / "step=6.ckpt"), map_location="cpu", weights_only=False)
    assert set(ck) >= {"state_dict", "hyper_parameters", "global_step"} and ck["global_step"] == 6
    from mebt.transformer import Net2NetTransformer
    m = Net2NetTransformer.load_from_checkpoint(str(tmp_path / "runs" / "step=6.ckpt"))
    assert torch.equal(m.state_dict()["transformer.head.weight"].cpu(), ck["state_dict"]["transformer.head.weight"])
    # --ckpt_path resumes (optimizer moments, step counters, RNG): the run continues at step 7 and stops at max_steps
    assert {"adam", "step_count", "rng"} <= set(ck["mebt_amd_loop"]) and ck["mebt_amd_loop"]["step_count"] == 6
    out2 = subprocess.run([sys.executable, "-m", "mebt_amd.train", "--preset", "tiny", "--tokens", f, "--max_steps", "10", "--log_every", "2",
                           "--ckpt_every", "10", "--default_root_dir", str(tmp_path / "runs"), "--ckpt_path", str(tmp_path / "runs" / "step=6.ckpt"),
                           "--accumulate_grad_batches", "1"], cwd=root, capture_output=True, text=True, timeout=600)
    assert out2.returncode == 0, out2.stderr[-2000:]
    steps = [int(v) for v in re.findall(r"step (\d+):", out2.stdout)]
    assert steps == [8, 10], out2.stdout
    ck2 = torch.load(str(tmp_path / "runs" / "step=10.ckpt"), map_location="cpu", weights_only=False)
    assert ck2["global_step"] == 10 and ck2["mebt_amd_loop"]["step_count"] == 10


# ---- robustness of the host side -------------------------------------------------------------------------
def test_bf16_mirror_follows_torch_side_weight_writes():
    """The bf16 weight mirror must follow writes made through torch AFTER the engine exists: load_state_dict, an in-place
    op on a Parameter (each Parameter has its own version counter, separate from the flat buffer's)."""
    from oracle import closed_form as cf
    m = build_product("c1", "bf16").eval()
    g = load_golden("forward_c1")
    x, idx = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["indices"]).to(DEV)
    ci, ti = idx[:, :70].contiguous(), idx[:, 70:].contiguous()
    l0, _ = m.reconstruct_mask(x, ci, ti)
    l0 = l0.clone()
    sd2 = {k: (v * 1.5 if k.endswith("mlp.0.weight") or k.endswith("attn.query.weight") else v) for k, v in m.state_dict().items()}
    sd2 = {k: v.detach().cpu().clone() for k, v in sd2.items()}
    m.load_state_dict(sd2)
    l1, _ = m.reconstruct_mask(x, ci, ti)
    fresh = build_product("c1", "bf16").eval()
    fresh.load_state_dict(sd2)
    fresh = fresh.to(DEV)
    lf, _ = fresh.reconstruct_mask(x, ci, ti)
    assert (l1 - l0).abs().max().item() > 1e-2                 # the new weights are in use ...
    assert torch.equal(l1, lf)                                  # ... exactly as in a model built with them
    with torch.no_grad():
        m.transformer.blocks[1].mlp[2].weight.mul_(0.5)         # in-place op on one Parameter
        fresh.transformer.blocks[1].mlp[2].weight.mul_(0.5)
    l2, _ = m.reconstruct_mask(x, ci, ti)
    fresh._native.sync_lowp(force=True)
    lf2, _ = fresh.reconstruct_mask(x, ci, ti)
    assert (l2 - l1).abs().max().item() > 1e-3 and torch.equal(l2, lf2)


def test_resume_equals_uninterrupted_training(tmp_path):
    """6 steps straight == 3 steps, save (model + TrainLoop state), load into a NEW model, 3 more: moments, optimizer
    step, LR warm-up position, dropout seeds and the python RNG (which draws t) all continue (fp32 parity mode; the
    P-side gradients are atomically accumulated, hence the 1e-6 instead of bit equality)."""
    import random
    from mebt_amd import presets
    from mebt_amd.trainer import TrainLoop

    def make():
        torch.manual_seed(3)
        cfg = presets.tiny()
        cfg.model.params.embd_pdrop = cfg.model.params.resid_pdrop = cfg.model.params.attn_pdrop = 0.1
        cfg.exp.exact_lr, cfg.exp.warmup_steps = 1e-3, 5
        return presets.build_model(cfg, compute_dtype="f32")

    g = torch.Generator().manual_seed(8)
    xs = [torch.randint(0, 16384, (4, 2, 8, 8), generator=g).to(DEV) for _ in range(6)]
    idxs = [torch.stack([torch.randperm(128, generator=g) for _ in range(4)]).to(DEV) for _ in range(6)]
    ref = make().to(DEV).train()
    sd0 = {k: v.detach().cpu().clone() for k, v in ref.state_dict().items()}
    loop = TrainLoop(ref, max_steps=10)
    random.seed(123)
    for i in range(6):
        loop.step(xs[i], idxs[i])                              # t drawn from the python RNG
    a = make()
    a.load_state_dict(sd0)
    a = a.to(DEV).train()
    la = TrainLoop(a, max_steps=10)
    random.seed(123)
    for i in range(3):
        la.step(xs[i], idxs[i])
    path = str(tmp_path / "ck.pt")
    torch.save({"state_dict": {k: v.detach().cpu() for k, v in a.state_dict().items()}, "loop": la.state_dict()}, path)
    random.seed(999)                                            # the resumed run must not depend on the process RNG state
    ck = torch.load(path, weights_only=False)
    b = make()
    b.load_state_dict(ck["state_dict"])
    b = b.to(DEV).train()
    lb = TrainLoop(b, max_steps=10)
    lb.load_state_dict(ck["loop"])
    assert lb.step_count == 3 and b.global_step == 3 and b.trainer.global_step == 3
    for i in range(3, 6):
        lb.step(xs[i], idxs[i])
    for (k, p), (_, q) in zip(ref.state_dict().items(), b.state_dict().items()):
        # attn.key.bias has a mathematically zero gradient: AdamW normalises its rounding noise (atomic summation order)
        # into +-lr steps, so it is only bounded, not reproduced
        # elsewhere the atomically accumulated gradients (embedding rows, bias column sums) differ in the last bit between two runs
        # and AdamW turns that into up to ~1e-6 on single elements whose gradient is near its epsilon (seen: 1.15e-6 on one
        # tok_emb element): single elements are bounded well below one step (lr = 1e-3), the mean at rounding level — a resume
        # that lost the moments, the step count, the warm-up position or a seed moves every element by ~lr
        d = (p.float() - q.float()).abs()
        if k.endswith("attn.key.bias"):
            assert d.max().item() <= 6e-3, k
        else:
            assert d.max().item() <= 5e-5, (k, d.max().item())
            assert d.mean().item() <= 1e-6 * (1 + p.abs().max().item()), (k, d.mean().item())
    for u, v in zip(loop.native.adam, lb.native.adam):
        assert (u - v).abs().max().item() <= 1e-6 * (1e-3 + u.abs().max().item())
    # a run that restarts the counters (weights only) is NOT the same: the warm-up LR and bias correction restart
    c = make()
    c.load_state_dict(ck["state_dict"])
    c = c.to(DEV).train()
    lc = TrainLoop(c, max_steps=10)
    random.seed(123)
    for i in range(3, 6):
        lc.step(xs[i], idxs[i])
    assert max((p - q).abs().max().item() for p, q in zip(ref.state_dict().values(), c.state_dict().values())) > 1e-4
    # the Lightning-style optimizer facade persists its state too
    opt = b.configure_optimizers()
    osd = opt.state_dict()
    assert len(osd["mebt_flat_adam"]) == 4 and "steps" in osd
    opt.load_state_dict(osd)


def test_backward_of_a_stale_forward_raises():
    """one set of saved activations: forward, forward, backward(first) must not silently use the second's"""
    model = build_product("micro", "f32").train()
    g = load_golden("forward_micro")
    x, idx = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["indices"]).to(DEV)
    l1, *_ = model(x, None, t=0.5, indices=idx)
    l2, *_ = model(x, None, t=0.3, indices=idx)
    with pytest.raises(RuntimeError, match="overwritten"):
        l1.sum().backward()
    l2.sum().backward()                                          # the latest one is fine
    assert model.transformer.head.weight.grad is not None


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_gradient_accumulation_equals_mean_of_microbatch_gradients(dtype):
    """accumulate_grad_batches = 3 (reference train_transformer.py:46-49): the optimizer sees the mean of the three
    micro-batch gradients (each with its own t, NC/NT), compared with the oracle's autograd gradients averaged on the host,
    and takes ONE step for three calls."""
    from mebt_amd.trainer import TrainLoop
    model = build_product("c1", dtype).train()
    model.learning_rate = 1e-3
    loop = TrainLoop(model, accumulate_grad_batches=3)
    assert not loop.fused_optimizer
    cfg = mg.oracle_cfg("c1")
    P = {k: v.clone().requires_grad_(True) for k, v in orc.closed_form_params(cfg).items()}
    ts = (0.5, 0.2, 0.7)
    acc = {k: torch.zeros_like(v) for k, v in P.items()}
    for i, t in enumerate(ts):
        x, idx = mg.inputs("c1", 2, f"acc{i}")
        for p in P.values():
            p.grad = None
        logits, z_t, ntw, seq_len = orc.forward(P, cfg, x, idx, t, training=True)
        _, _, loss = orc.loss_and_acc(logits, z_t, ntw, seq_len, cfg)
        loss.backward()
        for k, p in P.items():
            if p.grad is not None:
                acc[k] += p.grad / 3
        loop.step(x.to(DEV), idx.to(DEV), t=t)
        assert loop.step_count == (1 if i == 2 else 0) and model.global_step == (1 if i == 2 else 0)
    torch.cuda.synchronize()
    gv = loop.native.views(orc.param_shapes(cfg), grads=True)
    lim = 2e-3 if dtype == "f32" else 8e-2
    bad = []
    for k, ref in acc.items():
        err = (gv[k].cpu() - ref).abs().max().item() / (ref.abs().max().item() + 1e-6)
        if not err < lim:
            bad.append((k, round(err, 5)))
    assert not bad, bad[:20]
    # the fused optimizer cannot accumulate: the engine refuses instead of silently dropping micro-batches
    nm = loop.native
    nm.set_grad_accumulate(True)
    nm.set_fused_adamw(1e-3, 0.01, 1)
    x, idx = mg.inputs("c1", 2, "acc0")
    ci, ti, _ = orc.divide_indices(idx, 0.5, cfg, True)
    lg = nm.forward(x.reshape(2, -1).to(DEV), ci.to(DEV), ti.to(DEV), training=True)
    with pytest.raises(RuntimeError, match="exclude each other"):
        nm.backward(lg, 1.0)
    nm.set_fused_adamw(step=0)
    nm.set_grad_accumulate(False)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_gpt_forward_boundary_backward(dtype):
    """GPT.forward(sos, contexts, targets) on caller-embedded tensors under autograd (mebt_gpt_forward
    'and the matching _backward'): gradients with respect to the three inputs and every block / ln_f / head parameter
    against the oracle's autograd (reference gpt.py:234-253)."""
    model = build_product("micro", dtype).eval()
    cfg = mg.oracle_cfg("micro")
    P = {k: v.clone().requires_grad_(True) for k, v in orc.closed_form_params(cfg).items()}
    xx, idx = mg.inputs("micro", 2, "gptbwd")
    ci, ti = idx[:, :9], idx[:, 9:]
    with torch.no_grad():
        sos, ctx, tgt = orc.embed(P, cfg, xx.reshape(2, -1), ci, ti)
    g = torch.Generator().manual_seed(4)
    w = torch.randn(2, ti.shape[1], 16384, generator=g) * 1e-2
    ins = [t.detach().clone().requires_grad_(True) for t in (sos, ctx, tgt)]
    ref = orc.gpt_forward(P, cfg, *ins)
    (ref * w).sum().backward()
    dev_ins = [t.detach().to(DEV).requires_grad_(True) for t in (sos, ctx, tgt)]
    got, _ = model.transformer(*dev_ins, None, 0.)
    assert got.requires_grad
    tol = 1e-4 if dtype == "f32" else 2e-2
    assert (got.detach().cpu() - ref.detach()).abs().max().item() < tol
    (got * w.to(DEV)).sum().backward()
    lim = 2e-3 if dtype == "f32" else 8e-2
    for a, b, name in zip(dev_ins, ins, ("sos", "contexts", "targets")):
        err = (a.grad.cpu() - b.grad).abs().max().item() / b.grad.abs().max().item()
        assert err < lim, (name, err)
    bad = []
    for k, p in model.named_parameters():
        if not k.startswith("transformer."):
            continue
        refg = P[k].grad
        scale = P[k.replace("attn.key.bias", "attn.query.bias")].grad.abs().max().item()    # key.bias: zero gradient, judged on the query-bias scale
        err = (p.grad.cpu() - refg).abs().max().item() / (scale + 1e-12)
        if not err < lim:
            bad.append((k, round(err, 5)))
    assert not bad, bad[:20]
    # without autograd interest the inference path is taken (no activations kept)
    with torch.no_grad():
        inf, _ = model.transformer(sos.to(DEV), ctx.to(DEV), tgt.to(DEV), None, 0.)
    assert not inf.requires_grad and (inf.cpu() - ref.detach()).abs().max().item() < tol


def test_bench_plain_run_times_the_steps_asked_for_and_dumps_the_last_ones_outputs(tmp_path):
    """`bench.py --steps K --warmup W` without --full: ONE line with the headline fields, exactly K timed steps, nothing measured
    beyond them; `--dump-outputs DIR` writes the last timed step's statistics row and a fixed sample of the fp32 weights it updated
    (float arrays, 64 MB at most).  Two runs with the same arguments and the same GEMM picks (one tune cache: the first run tunes
    and writes it, the second reads it) compute the same arrays up to the order of atomically accumulated sums - far closer than
    the ~lr per element that any change of the inputs, the weights or the sample positions would move the updated weights."""
    import json, subprocess, sys
    from mebt_amd import presets
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MEBT_DP_FORCE")}
    env["MEBT_GEMM_TUNE_CACHE"] = str(tmp_path / "tune_cache.txt")
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        out = subprocess.run([sys.executable, "bench.py", "--preset", "tiny", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)],
                             cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        lines = [l for l in out.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, out.stdout
        r = json.loads(lines[0])
        assert r["steps"] == 3 and r["warmup"] == 1 and r["higher_is_better"] is True and r["dtype"] == "bf16"
        assert r["value"] > 0 and r["ms_per_step"] > 0 and r["metric"] and r["unit"]
        assert not {"roofline", "windows", "gpu_state", "host_enqueue_ms_per_step", "secondary", "cpu_baseline"} & set(r), sorted(r)
        files = sorted(os.listdir(d))
        assert files == ["master_P_sample.npy", "master_W_sample.npy", "step_stats.npy"], files
        assert sum((d / f).stat().st_size for f in files) <= 64 << 20
        arrs = {f[:-4]: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrs.values())
        st = arrs["step_stats"]
        assert st.shape == (5,) and abs(st[4] - r["config"]["loss"]) <= 1e-4 and st[3] > 0 and st[3] % 6 == 0      # batch 6
        runs.append(arrs)
    a, b = runs
    assert (tmp_path / "tune_cache.txt").is_file()
    np.testing.assert_allclose(b["step_stats"][[0, 4]], a["step_stats"][[0, 4]], rtol=1e-5)      # CE sum, loss
    assert np.abs(a["step_stats"][1:4] - b["step_stats"][1:4]).max() <= 1                         # top-1 / top-5 hits, rows
    lr = presets.tiny().exp.exact_lr
    for k in ("master_W_sample", "master_P_sample"):
        assert a[k].shape == b[k].shape
        assert_same_trajectory(a[k], b[k], k, lr=lr)
