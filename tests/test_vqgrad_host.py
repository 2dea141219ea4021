"""First-stage backward, the parts that need no GPU: the gradient fixture of the real reference (tests/golden/vqgrad) against float64
autograd of the CPU oracle's layers, the host-side plan of the convolution data gradient (taps, parity classes, zero box, halo fold)
against a scatter through the forward's own clamp rule, and the host interface of `VQGAN.recon_backward` / `configure_optimizers`."""
import argparse

import numpy as np
import pytest
import torch

from oracle import vqgan_oracle as vq
from tests import vqgrad_common as vc
from tests.golden import make_golden as mg


@pytest.fixture(scope="module")
def fx():
    return vc.load_fixture()


def test_fixture_gradients_match_float64_autograd_of_the_oracle(fx):
    """all 68 gradients of the reference's fp32 backward within 1e-5 of the tensor's maximum of the float64 oracle (measured 3.2e-6); the
    three bias gradients that are exactly zero (GroupNorm with one channel per group in front) against their layer's weight gradient"""
    cfg = mg.vqgan_cfg("vq_micro")
    P = vq.closed_form_params(cfg)
    x, ids = torch.from_numpy(fx["x"]), torch.from_numpy(fx["ids_0"])
    assert float(fx["l1_weight"]) == vc.L1_WEIGHT
    # the ids are the oracle's own, and not near a tie
    ids_o, _, dist = vq.encode(P, cfg, x, return_all=True)
    assert torch.equal(ids_o, ids)
    b2 = torch.topk(dist, 2, dim=1, largest=False).values
    assert float(((b2[:, 1] - b2[:, 0]) / b2[:, 0].abs()).min()) >= 2e-3
    g64, rl, cl = vc.objective_grads(P, cfg, x, ids)
    ref = vc.fixture_grads(fx)
    assert sorted(ref) == sorted(g64) and len(ref) == 68
    assert abs(rl - fx["step_losses"][0, 0]) < 1e-5 * rl and abs(cl - fx["step_losses"][0, 1]) < 1e-5 * cl
    worst = 0.0
    for k in g64:
        assert ref[k].shape == g64[k].shape and ref[k].dtype == np.float32
        err = np.abs(ref[k] - g64[k]).max() / vc.scale_of(k, g64)
        worst = max(worst, err)
        assert err < 1e-5, (k, err)
    for k in vc.ZERO_BIAS:
        assert np.abs(g64[k]).max() < 1e-12 * vc.scale_of(k, g64), k            # exactly zero in exact arithmetic
    print(f"[vqgrad fixture] worst deviation from float64 {worst:.2e} of the tensor's maximum")
    # the losses fall over the two recorded SGD steps, and no L1 sign hangs on rounding
    tot = fx["step_losses"].sum(1)
    assert tot[2] < tot[1] < tot[0]
    _, _, rec, _ = vc.objective({k: v.double() for k, v in P.items()}, cfg, x.double(), ids)
    assert float((rec - x).abs().min()) >= 1e-4


GEOMETRIES = [("conv", 3, (1, 1, 1)), ("conv", 4, (2, 2, 2)), ("conv", 4, (1, 2, 2)), ("conv", 1, (1, 1, 1)),
              ("convt", 4, (2, 2, 2)), ("convt", 4, (1, 2, 2))]
DIMS = [(4, 6, 10), (2, 3, 5), (2, 4, 6), (1, 4, 4), (1, 2, 2)]


@pytest.mark.parametrize("kind,k,stride", GEOMETRIES)
def test_dgrad_plan_equals_the_scatter_of_the_forward_rule(kind, k, stride):
    """The plan is integers and weight re-layouts only.  Walked in numpy exactly as the GPU path walks it (zero box, clamped-gather
    convolution per class onto the padded lattice, fold), it must give what scattering w^T dy through the forward's clamp gives — on a
    ragged shape, with both halos of a k = 3 layer on a two-voxel axis, on a one-voxel axis (both halos on ONE voxel) and on a 1 x 2 x 2
    input.  It also checks that no tap leaves the zero box and that the classes tile the lattice once."""
    from mebt_amd.vqgan import _Conv
    g = torch.Generator().manual_seed(k * 10 + len(kind))
    cin, cout, B = 3, 2, 2
    w = torch.randn(cout, cin, k, k, k, generator=g) if kind == "conv" else torch.randn(cin, cout, k, k, k, generator=g)
    cv = _Conv(w, None, (k, k, k), stride, kind == "convt", "f32")
    ran = 0
    for dims in DIMS:
        if kind == "conv" and any(d % s for d, s in zip(dims, stride)):
            continue                                                   # the encoder only halves even axes
        od = cv.out_dims(dims)
        dy = torch.randn(B, *od, cout, generator=g, dtype=torch.float64).numpy()
        got, want = vc.run_dgrad_plan(cv, dims, dy), vc.scatter_dgrad(cv, dims, dy)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (kind, k, stride, dims)
        # ... and the forward rule itself is the oracle's layer: autograd of the float64 layer gives the same dx
        x = torch.zeros(B, cin, *dims, dtype=torch.float64, requires_grad=True)
        fn = vq.same_pad_conv3d if kind == "conv" else vq.same_pad_conv_transpose3d
        y = fn(x, w.double(), None, stride)
        y.backward(torch.from_numpy(dy).permute(0, 4, 1, 2, 3))
        assert np.abs(x.grad.permute(0, 2, 3, 4, 1).numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (kind, k, stride, dims)
        ran += 1
    assert ran >= 2


def test_full_weight_grad_puts_every_class_entry_back():
    """the class layout [Cout][tap][Cin] scattered back to the nn.Conv3d / nn.ConvTranspose3d shapes inverts the forward's re-layout"""
    from mebt_amd.vqgan import _Conv
    g = torch.Generator().manual_seed(5)
    for kind, k, stride, shape in (("conv", 4, (2, 2, 2), (5, 3, 4, 4, 4)), ("convt", 4, (1, 2, 2), (3, 5, 4, 4, 4)), ("conv", 3, (1, 1, 1), (2, 4, 3, 3, 3))):
        w = torch.randn(*shape, generator=g)
        cv = _Conv(w, None, (k, k, k), stride, kind == "convt", "f32")
        assert torch.equal(cv.full_weight_grad([c[2] for c in cv.classes]), w)


def _host_model(**kw):
    from mebt_amd.vqgan import VQGAN
    c = mg.VQGAN_CONFIGS["vq_micro"]
    return VQGAN(argparse.Namespace(n_hiddens=c["n_hiddens"], downsample=c["downsample"], image_channels=3, embedding_dim=c["embedding_dim"],
                                    n_codes=c["n_codes"], sequence_length=4, sample_every_n_frames=1, resolution=16, **kw))


def test_recon_backward_refuses_the_perceptual_term_and_names_the_follow_up():
    m = _host_model(perceptual_weight=0.5)
    with pytest.raises(NotImplementedError, match="LPIPS backward"):
        m.recon_backward(torch.zeros(1, 3, 4, 16, 16))


def test_configure_optimizers_is_the_references_autoencoder_adam():
    m = _host_model(lr=1.5e-4)
    opt = m.configure_optimizers()
    assert isinstance(opt, torch.optim.Adam) and len(opt.param_groups) == 1
    grp = opt.param_groups[0]
    assert grp["lr"] == 1.5e-4 and tuple(grp["betas"]) == (0.5, 0.9)
    want = [p for n, p in m.named_parameters() if n.startswith(vc.TRAINED)]
    assert len(want) == 68 and len(grp["params"]) == 68 and all(a is b for a, b in zip(grp["params"], want))


def test_default_grad_scale_is_a_power_of_two_that_places_the_l1_seed():
    m = _host_model(l1_weight=4.0)
    for l1w, n in ((4.0, 6144), (1e-4, 6144), (4.0, 16 * 786432), (4.0, 4 * 786432)):
        m.args.l1_weight = l1w
        S = m.default_grad_scale(n, 4096)
        assert np.frexp(S)[0] == 0.5 and 2.0 ** -4 < S * l1w / n <= 2.0 ** -3
        assert S == vc.default_scale(l1w, n)
