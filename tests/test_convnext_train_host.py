"""Host side of the ConvNeXt-tiny training path (no GPU): the opt-in switch, stochastic-depth probabilities, Options validation,
the unchanged refusals of a default model, the declared backward entries, and self-checks of the reference code the GPU tests
(tests/test_gpu_convnext_bwd.py) compare with."""
import copy

import pytest
import torch

import convnext_ref as R
import convnext_train_ref as T
from agplace_amd.convnext import STAGE_FIRST_BLOCK, ConvNeXt
from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
from agplace_amd.network_mm.image_fe import ImageFE
from agplace_amd.options import Options


@pytest.mark.parametrize("layers", ["2_2_2", "3_3_9", "1_0_2"])
def test_sd_probs_count_blocks_of_the_full_network(layers):
    counts = [int(v) for v in layers.split("_")]
    fe = ConvNeXt(counts)
    assert fe.stochastic_depth_prob == 0.1 and "stochastic_depth_prob" not in dict(fe.named_parameters())
    probs = fe.sd_probs()
    assert [len(p) for p in probs] == counts
    assert STAGE_FIRST_BLOCK == T.STAGE_FIRST_BLOCK == (0, 3, 6)
    for s, first in enumerate(STAGE_FIRST_BLOCK):
        assert probs[s] == pytest.approx([0.1 * (first + b) / 17 for b in range(counts[s])], abs=0, rel=1e-15)
    assert probs == T.sd_probs(counts)
    # the whole stage 3 of the full network ends at k = 14 of 17: features[7] (dropped by the truncation) holds 15 .. 17
    assert ConvNeXt([3, 3, 9]).sd_probs()[2][-1] == pytest.approx(0.1 * 14 / 17)


def test_first_block_never_drops():
    assert ConvNeXt([2, 2, 2]).sd_probs()[0][0] == 0.0
    assert ConvNeXt([0, 1, 1]).sd_probs()[0] == [] and ConvNeXt([0, 1, 1]).sd_probs()[1][0] > 0


def test_options_convnext_train_is_validated():
    assert Options().convnext_train is False
    assert Options(convnext_train=True).copy().convnext_train is True
    assert Options().copy(convnext_train=True).convnext_train is True
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="convnext_train"):
            Options(convnext_train=bad)


def test_switch_is_off_by_default_and_reaches_the_trunks():
    assert ConvNeXt([1, 1, 1])._train_enabled is False
    fe = ConvNeXt([1, 1, 1])
    assert fe.enable_training() is fe and fe._train_enabled and not fe.enable_training(False)._train_enabled
    base = dict(dbimage_fe="convnext_tiny", dbimage_fe_layers="1_1_1", maptype="a_b")
    assert not any(e.fe._train_enabled for e in DBVanilla2D("db", 256, opt=Options(**base)).dbimage_fes)
    assert all(e.fe._train_enabled for e in DBVanilla2D("db", 256, opt=Options(convnext_train=True, **base)).dbimage_fes)


def test_default_model_still_refuses_with_the_old_patterns():
    fe = ImageFE("convnext_tiny", "1_1_1")
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(NotImplementedError, match="gradients"):
        fe.eval()(x)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="train"):
        fe.train()(x)
    with pytest.raises(NotImplementedError, match="enable_training"):
        fe.fe.forward_maps_train(x)
    m = DBVanilla2D("db", 256, opt=Options(dbimage_fe="convnext_tiny", dbimage_fe_layers="1_1_1", maptype="a"))
    tiles = {"db_map": torch.zeros(1, 1, 3, 32, 32)}
    with pytest.raises(NotImplementedError, match="train"):
        m.train()(tiles, mode="db")
    with pytest.raises(NotImplementedError, match="gradients"):
        m.eval()(tiles, mode="db")


def test_switched_on_model_keeps_the_other_refusals():
    m = DBVanilla2D("db", 256, opt=Options(dbimage_fe="convnext_tiny", dbimage_fe_layers="1_1_1", maptype="a", convnext_train=True))
    with pytest.raises(NotImplementedError, match="uint8"):
        m.train()({"db_map": torch.zeros(1, 1, 32, 32, 3, dtype=torch.uint8)}, mode="db")
    with pytest.raises(NotImplementedError, match="db_frames"):
        m({"db_frames": torch.zeros(1, 1, 32, 32, 3, dtype=torch.uint8)}, mode="db")
    fe = ConvNeXt([1, 1, 1]).enable_training()
    with pytest.raises(ValueError, match="GPU"):
        fe.forward_maps_train(torch.zeros(1, 3, 32, 32))
    # a frozen trunk in .eval() takes the inference path (which, on the CPU, fails its own input check, not a refusal)
    m.freeze_backbone().eval()
    with pytest.raises(ValueError, match="forward_maps: x must be"):
        m({"db_map": torch.zeros(1, 1, 3, 32, 32)}, mode="db")


def test_backward_entries_are_declared_and_sized():
    from agplace_amd import _lib
    L = _lib.load()
    for name in ("agp_cnx_mlp_fwd_rows", "agp_cnx_mlp_bwd", "agp_cnx_dwconv_ln_bwd", "agp_cnx_downsample_bwd", "agp_cnx_stem_bwd",
                 "agp_cnx_bwd_workspace_bytes", "agp_cnx_bwd_slice_pixels"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    S = L.agp_cnx_bwd_slice_pixels()
    assert S == 1024
    assert L.agp_cnx_bwd_workspace_bytes(1, 4, 4, 100) == -1
    for c in (96, 192, 384):
        small, big = L.agp_cnx_bwd_workspace_bytes(1, 1, 1, c), L.agp_cnx_bwd_workspace_bytes(64, 64, 64, c)
        assert small >= 4 * 8 * c * c
        # no P x 4C term: per 1024-pixel slice 8 C^2 + 7 C floats of partial planes, plus stream-sized maps
        P = 64 * 64 * 64
        assert big <= 4 * ((P // S) * (8 * c * c + 7 * c) + 2.7 * P * c) + 65536


# --------------------------------------------------------------------------------- self-checks of the reference code
def test_gelu_grad_formula_against_autograd():
    x = torch.linspace(-6, 6, 4001, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(R.gelu_exact(x).sum(), x)
    assert float((T.gelu_grad(x.detach()) - g).abs().max()) <= 1e-12


def test_layernorm_backward_formula_against_autograd():
    z = R.seeded_input((3, 5, 96), 4, torch.float64).requires_grad_(True) * 2.0 + 0.3
    gamma = (0.5 + R.seeded_input((96,), 5, torch.float64).abs()).requires_grad_(True)
    beta = R.seeded_input((96,), 6, torch.float64).requires_grad_(True)
    gxn = R.seeded_input((3, 5, 96), 7, torch.float64)
    zz = z.detach().requires_grad_(True)
    out = torch.nn.functional.layer_norm(zz, (96,), gamma, beta, R.LN_EPS)
    want = torch.autograd.grad((out * gxn).sum(), [zz, gamma, beta])
    got = T.layernorm_bwd(zz.detach(), gamma.detach(), gxn)
    for a, b in zip(got, want):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


def test_scaled_block_restatement():
    """scale = None is the eval block; scale = 1 equals it; scale = 0 is the identity for that image only."""
    blk = R.seeded_trunk([1, 1, 1], 2).features[1][0]
    x = R.seeded_input((2, 96, 5, 4), 3, torch.float64)
    with torch.no_grad():
        assert torch.equal(T.scaled_block(blk, x, None), blk(x))
        assert torch.allclose(T.scaled_block(blk, x, torch.ones(2, dtype=torch.float64)), blk(x), rtol=0, atol=1e-14)
        y = T.scaled_block(blk, x, torch.tensor([0.0, 1.0 / 0.9], dtype=torch.float64))
        assert torch.equal(y[0], x[0]) and R.rel_l2(y[1], x[1]) >= 0.3


def test_reference_gradients_are_finite_and_felt():
    """The truths of the GPU tests, fp64: every parameter gradient of the trunk is finite and non-zero, with and without scales;
    an image dropped in a block gets no gradient through that block's branch; a downsample's dropped row / column gets exactly 0."""
    m = R.seeded_trunk([2, 1, 2], 2)
    x = R.seeded_input((2, 3, 32, 48), 2, torch.float64)
    R.check_weights_are_felt(m, x)
    probs = [p for stage in T.sd_probs([2, 1, 2]) for p in stage]
    scales = [None] + [torch.full((2,), 1.0 / (1.0 - p), dtype=torch.float64) for p in probs[1:]]
    scales[3][0] = 0.0
    for sc in (None, scales):
        mm = copy.deepcopy(m)
        maps = T.forward_maps_scaled(mm, x, sc)
        sum(v.square().sum() for v in maps).backward()
        for name, p in mm.features.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
    blk = m.features[5][0]
    xin = R.seeded_input((2, 384, 2, 3), 9, torch.float64).requires_grad_(True)
    T.scaled_block(blk, xin, torch.tensor([0.0, 1.25], dtype=torch.float64)).sum().backward()
    assert torch.equal(xin.grad[0], torch.ones_like(xin.grad[0])) and not torch.equal(xin.grad[1], torch.ones_like(xin.grad[1]))
    for C, (n, h, w) in ((96, (2, 7, 9)), (192, (1, 5, 4)), (384, (3, 2, 3))):
        ds = R.randomize_convnext(R.ConvNeXtTiny(), 2).double().features[{96: 2, 192: 4, 384: 6}[C]]
        gx, grads = T.module_truth(ds, R.seeded_input((n, C, h, w), 1, torch.float64), R.seeded_input((n, 2 * C, h // 2, w // 2), 2, torch.float64),
                                   torch.float64)
        assert bool((gx[:, :, 2 * (h // 2):] == 0).all()) and bool((gx[:, :, :, 2 * (w // 2):] == 0).all())
        assert float(gx[:, :, :2 * (h // 2), :2 * (w // 2)].abs().min()) > 0
        assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads.values())
