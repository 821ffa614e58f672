"""Options.convnext_range_guard without a GPU: the option, the refusal it lifts, and -- with the fp64 reference
(tests/convnext_guard_ref.py) -- the conditions on the INPUTS that tests/test_gpu_convnext_guard.py relies on: the clean model keeps
every rounding place below 65504 / 4, every planted case has its one place above 2 x 65504 and every other place below 65504 / 4.
The device's fp32 / fp16 error (about 1e-3 relative) is then far from the decision `> 65504`; these are conditions on the inputs,
not tolerances on a result.  The exact-boundary pair is exempt on its one place: the hidden unit sits at exactly 65504.0 or 65505.0.
"""
import pytest
import torch

import convnext_guard_ref as G

pytestmark = pytest.mark.filterwarnings("ignore::UserWarning")

SHAPES = ((2, 3, 32, 32), (1, 3, 36, 44))


@pytest.fixture(autouse=True)
def _the_switch_exists():
    """Every test here is about Options.convnext_range_guard, the reference conditions included: without the switch none applies."""
    from agplace_amd.options import Options
    assert Options(convnext_range_guard=True).convnext_range_guard is True


DB = dict(dbimage_fe="convnext_tiny", dbimage_fe_layers="1_1_1", maptype="sat_road")
MMO = dict(mm_imgfe="convnext_tiny", mm_imgfe_layers="1_1_1", mm_imgfe_planes="96_192_384", mm_imgfe_dim=384, mm_stg2fuse_dim=384,
           mm_voxfe_planes="64_128_384", mm_voxfe_dim=384, mm_bevfe_planes="64_128_384", mm_bevfe_dim=384)


def test_option_is_validated_and_not_a_reference_option():
    import argparse
    from agplace_amd.options import Options, from_reference_opt
    assert Options().convnext_range_guard is False
    assert Options(convnext_range_guard=True).convnext_range_guard is True
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="convnext_range_guard"):
            Options(convnext_range_guard=bad)
    ns = argparse.Namespace(convnext_range_guard=True, fp16_range_guard=True)
    o = from_reference_opt(ns)
    assert o.convnext_range_guard is False and o.fp16_range_guard is True
    assert Options(convnext_range_guard=True).copy(margin=0.2).convnext_range_guard is True


def test_refusal_stays_without_the_switch_and_is_lifted_with_it():
    from agplace_amd import convnext as cnx
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.network.image_fe import ImageFE
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    text = ("ConvNeXt: convnext_precision=4 together with fp16_range_guard=True is not built (the guard's word "
            "is not wired into the fp16 ConvNeXt kernels); use convnext_precision=3 or turn the guard off")
    builders = (lambda o: DBVanilla2D("db", 256, opt=o.copy(**DB)), lambda o: MM(opt=o.copy(**MMO)))
    for build in builders:
        with pytest.raises(NotImplementedError) as e:
            build(Options(convnext_precision=4, fp16_range_guard=True, convnext_range_guard=False))
        assert str(e.value) == text
    with pytest.raises(NotImplementedError) as e:
        cnx.precision_from_options(Options(convnext_precision=4, fp16_range_guard=True))
    assert str(e.value) == text
    fe = ImageFE("convnext_tiny", "1_1_1", opt=Options(convnext_precision=4, fp16_range_guard=True)).eval()
    with torch.no_grad(), pytest.raises(NotImplementedError) as e:
        fe(torch.zeros(1, 3, 32, 32))
    assert str(e.value) == ("ImageFE('convnext_tiny'): precision 4 together with fp16_range_guard=True is not "
                            "built (the guard's word is not wired into the fp16 ConvNeXt kernels)")
    # with the switch: accepted by both models (construction only) and by precision_from_options, with or without fp16_range_guard
    for both in (True, False):
        o = Options(convnext_precision=4, fp16_range_guard=both, convnext_range_guard=True)
        assert cnx.precision_from_options(o) == 4
        db, mm = (b(o) for b in builders)
        assert [e.fe.precision for e in db.dbimage_fes] == [4, 4] and mm.image_fe.fe.precision == 4
        # the trunks inside a model report through it: they know the model's options
        assert all(e.model_opt is db.opt for e in db.dbimage_fes) and mm.image_fe.model_opt is mm.opt
        assert ImageFE("convnext_tiny", "1_1_1", opt=o).model_opt is None
    # accepted and inert with precision 3 and on a ResNet trunk
    assert cnx.precision_from_options(Options(convnext_range_guard=True, fp16_range_guard=True)) == 3
    assert ImageFE("resnet18", "2_2_2", opt=Options(convnext_range_guard=True)).fe_type == "resnet18"


def test_when_the_guard_binds():
    from agplace_amd import range_guard
    from agplace_amd.options import Options
    on, off = Options(convnext_range_guard=True), Options()
    assert range_guard.active_cnx(on, 4) and not range_guard.active_cnx(on, 3) and not range_guard.active_cnx(off, 4)
    assert not range_guard.active_cnx(on, 4, train=True)
    assert range_guard.cnx_tag(off, 4) is None and range_guard.cnx_tag(on, 3, 4) is None
    assert range_guard.cnx_tag(on, 4) == "cnx4" and range_guard.cnx_tag(on, 4, 4) == "cnx4"           # fp16_range_guard off
    both = Options(convnext_range_guard=True, fp16_range_guard=True)
    assert range_guard.cnx_tag(both, 4, 4) == "cnx4+4" and range_guard.cnx_tag(both, 4, 2) == "cnx4+2"
    assert range_guard.cnx_tag(both, 4, 3) == "cnx4"                                                  # mode-3 maps: nothing to cover
    assert range_guard.bound_word() is None
    range_guard.note_planes(torch.zeros(1, dtype=torch.int32))                                        # unbound: nothing happens


def _message(tag):
    from agplace_amd import range_guard
    g = range_guard.Guard("MM")
    g.reset = lambda: None                    # (no word was ever made; the real reset synchronises the device)
    g.last_prec = tag
    with pytest.raises(ValueError) as e:
        g.report("this")
    return str(e.value)


def test_report_texts():
    msg = _message("cnx4")
    for part in ("MM: in this batch", "ConvNeXt trunk's precision-4 products", "stored saturated", "a block's LayerNorm output",
                 "the GELU output", "a downsample's LayerNorm output", "an fp16 weight plane", "are wrong",
                 "reports, it does not rescue", "convnext_precision = 3"):
        assert part in msg, part
    assert "mfma_precision" not in msg
    both = _message("cnx4+4")
    assert "convnext_precision = 3" in both and "precision mode 4" in both and "mfma_precision = 3" in both
    assert "stage 2, the voxel branch" in both
    # the two existing texts, byte for byte
    assert _message(4) == ("MM: in this batch a feature map left fp16's range (|v| > 65504) and was stored saturated in "
                           "precision mode 4: its outputs are wrong. Run this model with Options.mfma_precision = 3 "
                           "(split-bf16 maps, fp32 range). For the image path agplace_amd.map_exponents.calibrate chooses per-map "
                           "power-of-two exponents that keep such a checkpoint in this mode; the guard watches the STORED values, so "
                           "with exponents installed it reports what the calibration did not cover")
    assert _message("train16") == ("MM: in this batch a training forward (Options.train_precision = 16) stored an fp16 "
                                   "value saturated (|v| > 65504 before the clamp): a pre-BatchNorm plane or a conv1 -> conv2 plane of the "
                                   "fast mode, or an fp16 operand plane of the one-pass weight gradient (DESIGN.md section 2). The step "
                                   "trained on clamped activations or clamped weight-gradient operands. The guard reports, it does "
                                   "not rescue: lower the weights' / BatchNorm gammas' scale, or train this model in the tight mode "
                                   "(train_precision = 32), whose maps are split-bf16")


def test_weight_plane_flags():
    """prep_block / prep_down at precision 4 carry the clamp flag of their planes (int32 [1]; NaN is kept, not clamped); the trunk's
    cached planes carry the OR of all of them, per parameter version."""
    from agplace_amd import convnext as cnx
    m = G.clean_trunk().float()
    fe = cnx.ConvNeXt(G.LAYERS)
    fe.load_state_dict(m.state_dict(), strict=True)
    with torch.no_grad():
        blk, ds = fe.features[1][0], fe.features[2]
        assert cnx.prep_block(blk)["sat"] is None and cnx.prep_down(*ds)["sat"] is None
        p = cnx.prep_block(blk, prec=4)
        assert p["sat"].dtype == torch.int32 and p["sat"].tolist() == [0] and cnx.prep_down(*ds, prec=4)["sat"].tolist() == [0]
        assert fe._prepared(4)["sat"].tolist() == [0] and "sat" not in fe._prepared(3)
        blk.block[3].weight[7, 9] = 65504.0               # exactly the limit: not clamped
        assert cnx.prep_block(blk, prec=4)["sat"].tolist() == [0]
        blk.block[3].weight[7, 9] = float("nan")          # kept, not reported
        assert cnx.prep_block(blk, prec=4)["sat"].tolist() == [0]
        blk.block[3].weight[7, 9] = -65520.0
        assert cnx.prep_block(blk, prec=4)["sat"].tolist() == [1]
        assert fe._prepared(4)["sat"].tolist() == [1]     # a new parameter version: the planes and the flag are rebuilt
        blk.block[3].weight[7, 9] = 0.0
        blk.block[5].weight[1, 2] = float("inf")
        assert cnx.prep_block(blk, prec=4)["sat"].tolist() == [1]
        blk.block[5].weight[1, 2] = 0.0
        ds[1].weight[0, 0, 1, 1] = 1e6
        assert cnx.prep_down(*ds, prec=4)["sat"].tolist() == [1] and fe._prepared(4)["sat"].tolist() == [1]
        ds[1].weight[0, 0, 1, 1] = 0.0
        assert fe._prepared(4)["sat"].tolist() == [0]


# ------------------------------------------------------------------------------------------ conditions the GPU file relies on
@pytest.mark.parametrize("shape", SHAPES)
def test_clean_model_is_far_inside(shape):
    mx = G.operand_maxima(G.clean_trunk(), G.image(shape))
    assert len(mx) == 16 and max(mx.values()) < G.LIMIT / 4 and not G.expected_flag(mx)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("place,stage", G.CASES)
def test_planted_cases_touch_one_place(place, stage, shape):
    x = G.image(shape)
    mx = G.operand_maxima(G.plant(G.clean_trunk(), place, stage, x), x)
    assert G.expected_flag(mx)
    for key, v in mx.items():
        if key == (stage, place):
            assert v > 2 * G.LIMIT, (key, v)
        else:
            assert v < G.LIMIT / 4, (key, v)


@pytest.mark.parametrize("value,flag", [(65504.0, False), (65505.0, True)])
def test_exact_boundary_pair(value, flag):
    assert float(torch.tensor(value, dtype=torch.float32)) == value
    for shape in SHAPES:
        x = G.image(shape)
        mx = G.operand_maxima(G.plant_boundary(G.clean_trunk(), 0, value), x)
        assert mx[(0, 3)] == value and G.expected_flag(mx) == flag
        assert all(v < G.LIMIT / 4 for k, v in mx.items() if k != (0, 3))


def test_replay_pair_of_images():
    """The replay test's two images and hidden unit: the unit's maximum over the bad image is at least 1.3 x its maximum over the
    good one and 65504 lies at their geometric mean, so the good image stays below 65504 / sqrt(1.3) and the bad one goes above
    65504 x sqrt(1.3); every other place stays below 65504 / 4 on both."""
    good, bad = G.image((1, 3, 32, 32), 11), G.image((1, 3, 32, 32), 12)
    m, unit, ratio = G.replay_case(G.clean_trunk(), good, bad)
    assert ratio >= 1.3, ratio
    mg, mb = G.operand_maxima(m, good), G.operand_maxima(m, bad)
    assert mg[(0, 3)] <= G.LIMIT / 1.3 ** 0.5 * (1 + 1e-9) and mb[(0, 3)] >= G.LIMIT * 1.3 ** 0.5 * (1 - 1e-9), (mg[(0, 3)], mb[(0, 3)])
    # (the scaled W1 row is rounded to fp16 again, 2^-11 relative per element, so the geometric mean sits within that of 65504)
    assert abs((mg[(0, 3)] * mb[(0, 3)]) ** 0.5 / G.LIMIT - 1) < 2.0 ** -11
    assert not G.expected_flag(mg) and G.expected_flag(mb)
    for mx in (mg, mb):
        assert all(v < G.LIMIT / 4 for k, v in mx.items() if k != (0, 3))
