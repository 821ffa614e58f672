"""The CPU restatement of convnext_tiny (tests/convnext_ref.py) against torchvision's published structure."""
import torch
import torch.nn.functional as F

import convnext_ref as R


def expected_keys(depths=(3, 3, 9, 3), stages=4):
    """torchvision's convnext_tiny state_dict keys, written out from its definition (not read from the restatement)."""
    keys = ["features.0.0.weight", "features.0.0.bias", "features.0.1.weight", "features.0.1.bias"]
    for s in range(stages):
        for b in range(depths[s]):
            pre = f"features.{1 + 2 * s}.{b}."
            keys.append(pre + "layer_scale")
            for k in (0, 2, 3, 5):
                keys += [pre + f"block.{k}.weight", pre + f"block.{k}.bias"]
        if s < stages - 1:
            pre = f"features.{2 + 2 * s}."
            keys += [pre + "0.weight", pre + "0.bias", pre + "1.weight", pre + "1.bias"]
    return keys + ["classifier.0.weight", "classifier.0.bias", "classifier.2.weight", "classifier.2.bias"]


def test_full_model_parameter_count_and_keys():
    m = R.ConvNeXtTiny()
    assert sum(p.numel() for p in m.parameters()) == 28_589_128
    keys = list(m.state_dict().keys())
    assert len(keys) == 182 and keys == expected_keys()
    assert m.state_dict()["features.1.0.layer_scale"].shape == (96, 1, 1)
    assert m.state_dict()["features.6.1.weight"].shape == (768, 384, 2, 2)
    assert m.state_dict()["features.5.8.block.3.weight"].shape == (1536, 384)


def test_truncated_trunk_and_map_shapes():
    t = R.trunk([2, 2, 2]).eval()
    assert sum(p.numel() for p in t.features.parameters()) == 3_549_216
    assert list(t.state_dict().keys()) == expected_keys((2, 2, 2), 3)
    with torch.no_grad():
        maps = R.forward_maps(t, torch.randn(2, 3, 70, 100))
    assert [tuple(m.shape) for m in maps] == [(2, 96, 17, 25), (2, 192, 8, 12), (2, 384, 4, 6)]
    assert len(R.trunk([3, 3, 9]).features[5]) == 9 and len(R.trunk([2, 1, 2]).features[3]) == 1


def test_gelu_and_layernorm2d_match_torch():
    torch.manual_seed(0)
    x = torch.randn(3, 24, 5, 7, dtype=torch.float64) * 3
    assert torch.allclose(R.gelu_exact(x), F.gelu(x), rtol=0, atol=1e-14)
    ln = R.LayerNorm2d(24, eps=1e-6).double()
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5)
        ln.bias.normal_()
        want = F.layer_norm(x.permute(0, 2, 3, 1), (24,), ln.weight, ln.bias, 1e-6).permute(0, 3, 1, 2)
        assert torch.allclose(ln(x), want, rtol=0, atol=1e-12)


def test_default_initialisation_is_the_identity_and_seeded_weights_are_not():
    with torch.no_grad():
        blk = R.ConvNeXtTiny().double().features[1][0]
        y = torch.randn(1, 96, 8, 8, dtype=torch.float64)
        assert R.rel_l2(blk(y), y) < 1e-5
    R.check_weights_are_felt(R.seeded_trunk([3, 3, 9], 2), R.seeded_input((1, 3, 32, 32), 2))
