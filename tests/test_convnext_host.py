"""Host side of the ConvNeXt-tiny trunk: construction, keys, truncation, refusals (no GPU)."""
import os

import numpy as np
import pytest
import torch

import convnext_ref as R
from agplace_amd.convnext import ConvNeXt
from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
from agplace_amd.network.image_fe import ImageFE as ImageFEdb
from agplace_amd.network_mm.image_fe import ImageFE
from agplace_amd.network_mm.mm import MM
from agplace_amd.options import Options

FLOW = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convnext_flow.npz"))


@pytest.mark.parametrize("cls", [ImageFE, ImageFEdb])
def test_keys_and_last_dim_follow_the_reference(cls):
    fe = cls("convnext_tiny", str(FLOW["layers"]))
    assert list(fe.fe.state_dict().keys()) == [str(k) for k in FLOW["keys"]]
    assert fe.last_dim == int(FLOW["last_dim"]) == 384
    assert not any(p.requires_grad for p in fe.fe.classifier.parameters())
    assert all(p.requires_grad for p in fe.fe.features.parameters())


def test_truncation_counts_blocks():
    assert sum(p.numel() for p in ImageFE("convnext_tiny", "2_2_2").fe.features.parameters()) == 3_549_216
    a, b = ImageFE("convnext_tiny", "3_3_9").fe, ImageFE("convnext_tiny", "2_2_2").fe
    assert len(a.features[5]) == 9 and len(b.features[5]) == 2 and len(a.state_dict()) > len(b.state_dict())
    assert len(ImageFE("convnext_tiny", "7_7_12").fe.features[5]) == 9       # a slice past the end keeps what there is


def test_strict_load_from_the_restatement():
    ref = R.seeded_trunk([2, 1, 2], 5, dtype=torch.float32)
    fe = ImageFE("convnext_tiny", "2_1_2")
    fe.fe.load_state_dict(ref.state_dict(), strict=True)
    assert torch.equal(fe.fe.features[3][0].block[5].weight, ref.features[3][0].block[5].weight)
    with pytest.raises(RuntimeError):
        ImageFE("convnext_tiny", "2_2_2").fe.load_state_dict(ref.state_dict(), strict=True)


def test_initialisation():
    fe = ConvNeXt([1, 1, 1])
    assert float(fe.features[1][0].layer_scale.detach().max()) == pytest.approx(1e-6)
    assert float(fe.features[0][0].bias.detach().abs().max()) == 0 and float(fe.features[1][0].block[2].weight.detach().min()) == 1
    w = fe.features[1][0].block[3].weight.detach()
    assert 0.015 < float(w.std()) < 0.025 and float(w.abs().max()) <= 2.0


def test_entry_counts_other_than_three_are_refused():
    with pytest.raises(NotImplementedError):
        ImageFE("convnext_tiny", "2_2")
    with pytest.raises(NotImplementedError, match="768"):
        ImageFE("convnext_tiny", "3_3_9_3")


def test_map_sizes():
    assert ConvNeXt.map_sizes(70, 100) == [(17, 25), (8, 12), (4, 6)]
    assert ConvNeXt.map_sizes(16, 16) == [(4, 4), (2, 2), (1, 1)]
    for hw in ((15, 64), (64, 3)):
        with pytest.raises(ValueError):
            ConvNeXt.map_sizes(*hw)


def test_splitmap_api_and_other_precisions_are_refused():
    fe = ImageFE("convnext_tiny", "1_1_1").eval()
    with pytest.raises(NotImplementedError, match="SplitMap"):
        fe.forward_maps(torch.zeros(1, 3, 32, 32))
    for prec in (1, 2, 4):
        with pytest.raises(ValueError, match="prec"):
            fe(torch.zeros(1, 3, 32, 32), prec=prec)


def test_mm_names_the_missing_case():
    with pytest.raises(NotImplementedError, match="convnext_tiny"):
        MM(opt=Options(mm_imgfe="convnext_tiny"))


def test_dbvanilla2d_container():
    opt = Options(dbimage_fe="convnext_tiny", dbimage_fe_layers="2_1_2", maptype="a_b")
    m = DBVanilla2D("db", 256, opt=opt)
    lin = m.dbimage_mlps[1].seq[0]
    assert (lin.in_features, lin.out_features) == (384, 256)
    assert "dbimage_fes.1.fe.features.1.0.block.3.weight" in m.state_dict()
    m.freeze_backbone()
    assert not any(p.requires_grad for p in m.dbimage_fes.parameters()) and all(p.requires_grad for p in m.dbimage_mlps.parameters())
    # the refusals that need no device: .train(), uint8 tiles, decoded frames
    with pytest.raises(NotImplementedError, match="train"):
        m.train()({"db_map": torch.zeros(1, 2, 3, 32, 32)}, mode="db")
    m.eval()
    with pytest.raises(NotImplementedError, match="uint8"):
        m({"db_map": torch.zeros(1, 2, 32, 32, 3, dtype=torch.uint8)}, mode="db")
    with pytest.raises(NotImplementedError, match="db_frames"):
        m({"db_frames": torch.zeros(1, 2, 32, 32, 3, dtype=torch.uint8)}, mode="db")


def test_workspace_has_no_hidden_map_term():
    from agplace_amd import _lib
    L = _lib.load()
    for c in (96, 192, 384):
        for n, h, w in ((1, 1, 1), (2, 9, 5), (64, 64, 64), (64, 16, 16)):
            P = n * h * w
            b = L.agp_cnx_workspace_bytes(n, h, w, c)
            assert 0 < b <= 1.25 * P * c * 4 + 65536
    assert L.agp_cnx_workspace_bytes(1, 4, 4, 100) == -1
