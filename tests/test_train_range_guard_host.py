"""The training range guard's host side (Options.train_range_guard, agplace_amd/range_guard.py): the option, the predicate
beside range_guard.active (which keeps its definition) and the models' constructors.  Nothing here needs a GPU."""
import types

import pytest
import torch


def test_option_default_validation_copy_and_reference():
    from agplace_amd.options import Options, from_reference_opt
    assert Options().train_range_guard is False
    on = Options(train_range_guard=True)
    assert on.train_range_guard is True
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="train_range_guard"):
            Options(train_range_guard=bad)
    o = Options()
    o.train_range_guard = "on"
    with pytest.raises(ValueError, match="train_range_guard"):
        o.validate()
    # copy() carries it, in both directions, and keeps the other guard's switch apart
    assert on.copy().train_range_guard is True
    assert on.copy(train_precision=16).train_range_guard is True
    assert on.copy(train_range_guard=False).train_range_guard is False
    assert on.fp16_range_guard is False and Options(fp16_range_guard=True).train_range_guard is False
    # not a reference option: a namespace cannot switch it on
    ns = types.SimpleNamespace(train_range_guard=True, features_dim=256)
    assert from_reference_opt(ns).train_range_guard is False
    assert from_reference_opt(types.SimpleNamespace()).train_range_guard is False


def test_active_train_follows_the_option_and_active_keeps_its_definition():
    from agplace_amd import range_guard
    from agplace_amd.options import Options
    on = Options(train_range_guard=True)
    assert range_guard.active_train(on)
    assert range_guard.active_train(on.copy(train_precision=16))
    assert not range_guard.active_train(Options())
    assert not range_guard.active_train(Options(fp16_range_guard=True))
    assert not range_guard.active_train(types.SimpleNamespace())          # (an options object from before the field existed)
    # the inference predicate is what it was: training never binds through it, whatever the new option says
    assert range_guard.active(on, 4, True) is False
    assert range_guard.active(on, 4, False) is False
    both = Options(fp16_range_guard=True, train_range_guard=True)
    assert range_guard.active(both, 4, False) and range_guard.active(both, 2, False)
    assert not range_guard.active(both, 4, True) and not range_guard.active(both, 3, False)
    assert range_guard.train_tag(on) == "train32" and range_guard.train_tag(on.copy(train_precision=16)) == "train16"


def test_guarded_train_is_a_no_op_without_the_option():
    """Off (the default): no guard object is made and nothing is looked up on the model."""
    from agplace_amd import range_guard
    from agplace_amd.options import Options
    m = torch.nn.Linear(2, 2)
    with range_guard.guarded_train(m, Options()):
        pass
    assert "_fp16_guard" not in m.__dict__
    range_guard.poll(m)
    assert range_guard.ok(m)


def test_training_report_names_the_model_and_the_training_forward():
    from agplace_amd import range_guard
    g = range_guard.Guard("MM")
    g.reset = lambda: None                    # (no word was ever made; the real reset synchronises the device)
    g.last_prec = "train16"
    with pytest.raises(ValueError, match=r"^MM: in an earlier batch a training forward \(Options.train_precision = 16\)"):
        g.report("an earlier")
    g.last_prec = 4
    with pytest.raises(ValueError, match=r"^MM: .*fp16's range.*mfma_precision = 3"):
        g.report("an earlier")


@pytest.mark.parametrize("mode", [16, 32])
def test_models_build_with_the_option_on_the_cpu(mode):
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.network.image_fe import ImageFE as DBImageFE
    from agplace_amd.network_mm.image_fe import ImageFE
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    opt = Options(train_precision=mode, train_range_guard=True)
    for m in (MM(opt=opt), DBVanilla2D("db", opt.features_dim, opt=opt), ImageFE("resnet18", "2_2_2", opt=opt),
              DBImageFE("resnet50", "3_4_6", opt=opt)):
        m.train()
        m.poll_fp16_range()                   # nothing published yet: silent, and no device is touched
        assert m.fp16_range_ok()
    # ConvNeXt trunks store no fp16 in training: the option is accepted with them, with and without the trunk's training opt-in
    for extra in ({}, {"convnext_train": True}):
        copt = Options(dbimage_fe="convnext_tiny", dbimage_fe_layers="1_1_1", train_range_guard=True, **extra)
        DBVanilla2D("db", copt.features_dim, opt=copt)
        ImageFE("convnext_tiny", "1_1_1", opt=copt)
