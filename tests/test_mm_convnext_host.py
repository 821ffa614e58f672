"""Host-side tests (no GPU) of MM with mm_imgfe='convnext_tiny': the container, its refusals, and the fp64 reference the GPU
tests compare against (tests/mm_convnext_ref.py) pinned to oracle.nets.mm_forward_q."""
import pytest
import torch

import mm_convnext_ref as ref
from agplace_amd.network_mm.image_fe import ImageFE
from agplace_amd.network_mm.mm import MM
from agplace_amd.options import Options
from oracle import nets, resnet


def test_supported_configuration_constructs_with_the_reference_shapes():
    m = MM(opt=ref.options("2_1_2"))
    sd = m.state_dict()
    assert tuple(sd["fuseblocktoshallow.updimsimg.0.weight"].shape) == (384, 96)
    assert tuple(sd["fuseblocktoshallow.updimsimg.1.weight"].shape) == (384, 192)
    assert tuple(sd["fuseblocktoshallow.updimsvox.1.weight"].shape) == (384, 128)
    assert tuple(sd["fuseblocktoshallow.blocks.2.blocks.0.func.func.fc.weight"].shape) == (384, 384)
    assert tuple(sd["stg2fuseblock.ffnsimg.0.conv1.weight"].shape) == (384, 384, 3, 3)
    assert tuple(sd["stg2fusefc.weight"].shape) == (384, 384)
    trunk = {k[len("image_fe."):] for k in sd if k.startswith("image_fe.")}
    assert trunk == set(ImageFE("convnext_tiny", "2_1_2").state_dict())
    assert any(k.startswith("image_fe.fe.features.") for k in sd) and any(k.startswith("image_fe.fe.classifier.") for k in sd)


def test_state_dict_matches_the_reference_parameter_dict_and_loads_strictly():
    opt = ref.options("1_1_1")
    params, _ = ref.seeded_params(opt, seed=2, dtype=torch.float32)
    m = MM(opt=opt)
    sd = m.state_dict()
    assert set(sd) == set(params)
    assert all(tuple(sd[k].shape) == tuple(params[k].shape) for k in sd), [k for k in sd if sd[k].shape != params[k].shape]
    m.load_state_dict(params, strict=True)
    assert torch.equal(m.state_dict()["stg2fuseblock.ffnsimg.0.conv2.weight"], params["stg2fuseblock.ffnsimg.0.conv2.weight"])


@pytest.mark.parametrize("field,kw", [
    ("mm_imgfe_planes", dict(mm_imgfe_planes="64_128_256")),
    ("mm_imgfe_dim", dict(mm_imgfe_dim=256)),
    ("mm_stg2fuse_dim", dict(mm_stg2fuse_dim=256)),
    ("mm_voxfe_planes", dict(mm_voxfe_planes="64_128_256")),
    ("mm_voxfe_planes", dict(mm_voxfe_planes="32_128_384")),
    ("mm_voxfe_dim", dict(mm_voxfe_dim=256)),
    ("mm_imgfe_layers", dict(mm_imgfe_layers="2_2")),
    ("mm_imgfe_layers", dict(mm_imgfe_layers="2_2_2_2")),
])
def test_inconsistent_fields_are_refused_by_name(field, kw):
    with pytest.raises(NotImplementedError, match="convnext_tiny") as e:
        MM(opt=ref.options().copy(**kw))
    assert field in str(e.value)


def test_defaults_beside_the_trunk_are_still_refused():
    with pytest.raises(NotImplementedError, match="convnext_tiny"):
        MM(opt=Options(mm_imgfe="convnext_tiny"))


def test_refusals_that_need_no_device():
    m = MM(opt=ref.options())
    data = {"query_image": torch.zeros(1, 3, 64, 96)}
    with pytest.raises(NotImplementedError, match="train"):
        m.train()(data, mode="q")
    m.eval()
    with pytest.raises(NotImplementedError, match="gradient"):
        m(data, mode="q")
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="uint8"):
            m({"query_image": torch.zeros(1, 1, 64, 96, 3, dtype=torch.uint8)}, mode="q")
        with pytest.raises(NotImplementedError, match="query_frames"):
            m({"query_frames": torch.zeros(1, 1, 64, 96, 3, dtype=torch.uint8)}, mode="q")
        from agplace_amd import map_exponents, pair
        from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
        with pytest.raises(NotImplementedError, match="embed_pair"):
            pair.embed_pair(m, DBVanilla2D("db", 384, opt=Options(features_dim=384)).eval(), data, {"db_map": torch.zeros(1, 1, 3, 64, 64)})
        with pytest.raises(NotImplementedError, match="calibrate"):
            map_exponents.calibrate(m, [data])


def test_substream_option_goes_straight_to_forward_q(monkeypatch):
    m = MM(opt=ref.options(query_substreams=2)).eval()
    seen = []
    monkeypatch.setattr(m, "forward_q", lambda d, **k: seen.append(k) or "direct")
    monkeypatch.setattr(m, "_forward_q_substreams", lambda *a: pytest.fail("sub-stream split taken"))
    with torch.no_grad():
        assert m({"query_image": torch.zeros(4, 3, 64, 96)}, mode="q") == "direct" and seen == [{}]


def test_reference_glue_equals_the_oracle_on_resnet_maps():
    """The restated glue of tests/mm_convnext_ref.py against oracle.nets.mm_forward_q: both fed the maps of one resnet18 run
    (fp64), all seven outputs equal exactly -- for every final_fusetype, with and without output_l2."""
    for fuse, l2 in (("add", True), ("cat", False), ("catadd", True)):
        # (catadd adds the last term to the concatenation of the others: two terms, as in tests/test_oracle_golden.py)
        opt = Options(final_fusetype=fuse, output_l2=l2, **(dict(final_type=["imageorg", "stg2image"]) if fuse == "catadd" else {}))
        params = nets.init_mm_params(opt, seed=1, dtype=torch.float64)
        data = nets.synth_query(2, 32, 64, opt, seed=3, dtype=torch.float64)
        want = nets.mm_forward_q(data, params, opt)
        maps = resnet.forward_resnet(data["query_image"], params, opt.mm_imgfe, 3, prefix="image_fe.fe.")
        got = ref.forward_q(data, params, opt, maps=maps)
        assert set(got) == set(want) and len(got) == 7
        for k in want:
            assert torch.equal(got[k], want[k]), (fuse, l2, k)
