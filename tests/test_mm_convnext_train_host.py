"""Host-side tests (no GPU) of MM's opt-in ConvNeXt training: the switch, and the training reference of the GPU tests
(tests/mm_convnext_train_ref.py) pinned to the inference reference it restates."""
import torch

import mm_convnext_ref as ref
import mm_convnext_train_ref as tref
from agplace_amd.network_mm.mm import MM
from oracle import nets


def test_switch_enables_the_trunks_training_path():
    assert MM(opt=ref.options()).image_fe.fe._train_enabled is False
    assert MM(opt=ref.options(convnext_train=True)).image_fe.fe._train_enabled is True


def test_training_reference_equals_the_inference_reference_in_eval():
    """training=False, no scales: the seven outputs of mm_convnext_ref.forward_q exactly -- dense stand-ins and from `coords`."""
    from oracle import sparse as osp
    opt = ref.options("2_1_1")
    params, trunk = ref.seeded_params(opt, seed=3)
    data = nets.synth_query(2, 64, 96, opt, seed=4, dtype=torch.float64)
    cloud = {"query_image": data["query_image"]}
    cloud["coords"], cloud["features"] = osp.synth_cloud(2, 60, extent=10, seed=6)
    for d in (data, cloud):
        with torch.no_grad():
            want = ref.forward_q(d, params, opt, trunk=trunk)
            got = tref.forward_q(d, params, opt, trunk, scales=None, training=False, pattern=None)
        assert set(got) == set(want) and len(got) == 7
        for k in want:
            assert torch.equal(got[k], want[k]), k


def test_adopted_trunk_shares_its_leaves_with_the_parameter_dict():
    """adopt_trunk: the same maps as the seeded trunk, and a backward through forward_q reaches the trunk's weights under their
    image_fe.fe.* names; unit scales change nothing, a zero scale removes its block."""
    import convnext_ref
    opt = ref.options("1_1_1")
    params, trunk0 = ref.seeded_params(opt, seed=3)
    params = {k: v.clone() for k, v in params.items()}
    trunk = tref.adopt_trunk(params, [1, 1, 1])
    data = nets.synth_query(2, 64, 96, opt, seed=4, dtype=torch.float64)
    with torch.no_grad():
        want = convnext_ref.forward_maps(trunk0, data["query_image"])
        ones = [torch.ones(2, dtype=torch.float64)] * 3
        for a, b in zip(want, tref.convnext_train_ref.forward_maps_scaled(trunk, data["query_image"], ones)):
            assert torch.allclose(a, b, rtol=1e-12, atol=1e-12)
        zero = tref.forward_q(data, params, opt, trunk, scales=[None, None, torch.zeros(2, dtype=torch.float64)])
        full = tref.forward_q(data, params, opt, trunk)
        assert not torch.equal(zero["imagevec_org"], full["imagevec_org"])
    assert params["image_fe.fe.features.0.0.weight"] is trunk.features[0][0].weight
    assert not params["image_fe.fe.classifier.2.weight"].requires_grad
    tref.forward_q(data, params, opt, trunk)["embedding"].sum().backward()
    for k in ("image_fe.fe.features.0.0.weight", "image_fe.fe.features.5.0.block.3.weight"):
        assert params[k].grad is not None and float(params[k].grad.abs().max()) > 0, k
