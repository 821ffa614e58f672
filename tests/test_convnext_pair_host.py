"""Options.convnext_pair (lock-step ConvNeXt trunks in agplace_amd.pair.embed_pair) on the host: the switch, the refusals that stay
with it off, and pair.can_pair's ConvNeXt rule on CPU-constructed models.  No GPU needed."""
import argparse

import pytest
import torch

import mm_convnext_ref as ref
from agplace_amd import _lib, pair
from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
from agplace_amd.network_mm.mm import MM
from agplace_amd.options import Options, from_reference_opt

GROUPED = ("agp_cnx_stem_fwd_grouped", "agp_cnx_stem_u8_fwd_grouped", "agp_cnx_dwconv_ln_fwd_grouped", "agp_cnx_mlp_fwd_grouped",
           "agp_cnx_downsample_fwd_grouped", "agp_cnx_dwconv_ln_f16_fwd_grouped", "agp_cnx_mlp_f16_fwd_grouped",
           "agp_cnx_downsample_f16_fwd_grouped")


def test_switch_is_a_bool_and_off_by_default():
    assert Options().convnext_pair is False
    assert Options(convnext_pair=True).convnext_pair is True
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="convnext_pair"):
            Options(convnext_pair=bad)
    assert from_reference_opt(argparse.Namespace(convnext_pair=True)).convnext_pair is False
    assert Options(convnext_pair=True).copy().convnext_pair is True


def test_grouped_entries_are_declared_and_exported():
    L = _lib.load()
    for name in GROUPED:
        assert name in _lib.SIGNATURES and hasattr(L, name)
    # one group is legal, none or five are not; a null table is refused before anything is read
    bad = 1                                                 # AGP_E_BADARG
    g = (_lib.CnxGroup * 5)()
    for name in GROUPED:
        args = ([96] if "stem" not in name else []) + ([1e-6] if "mlp" not in name else []) + [None]
        assert getattr(L, name)(None, 1, *args) == bad, name
        assert getattr(L, name)(g, 0, *args) == bad and getattr(L, name)(g, 5, *args) == bad, name
        assert getattr(L, name)(g, 1, *args) == bad, name   # a zeroed descriptor: null pointers


def _mm(layers="1_1_1", **kw):
    return MM(opt=ref.options(layers, **kw)).eval()


def _db(layers="1_1_1", fe="convnext_tiny", **kw):
    return DBVanilla2D("db", 384, opt=Options(dbimage_fe=fe, dbimage_fe_layers=layers, features_dim=384, **kw)).eval()


QDATA = {"query_image": torch.zeros(1, 3, 32, 32)}
DBDATA = {"db_map": torch.zeros(1, 1, 3, 32, 32)}


def test_refusals_stay_with_the_switch_off():
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="pair.embed_pair with a ConvNeXt database model"):
            pair.embed_pair(_mm(), _db(), QDATA, DBDATA)
        with pytest.raises(NotImplementedError, match="pair.embed_pair with a ConvNeXt database model"):
            pair.embed_pair(_mm(convnext_pair=True), _db(), QDATA, DBDATA)
        with pytest.raises(NotImplementedError, match="pair.embed_pair with a ConvNeXt query model"):
            pair.embed_pair(_mm(), _db(convnext_pair=True), QDATA, DBDATA)
        with pytest.raises(NotImplementedError, match="lock-step trunks and row-sliced outputs"):
            _mm().forward_q(QDATA, image_maps=[None] * 3)
        with pytest.raises(NotImplementedError, match=r"lock-step trunks \(pair.embed_pair\) are not built"):
            _db().forward_db(DBDATA, trunk_maps={})
        # row-sliced outputs stay refused with the switch on, and so do query sub-streams, by name
        with pytest.raises(NotImplementedError, match="row-sliced outputs"):
            _mm(convnext_pair=True).forward_q(QDATA, out_rows={"embedding": torch.zeros(1, 384)})
        with pytest.raises(NotImplementedError, match="query_substreams"):
            pair.embed_pair(_mm(convnext_pair=True, query_substreams=2), _db(convnext_pair=True), QDATA, DBDATA)


def _can(q, d, dbdata=DBDATA):
    with torch.no_grad():
        return pair.can_pair(q, d, QDATA, dbdata)


def test_can_pair_rule_by_rule():
    on = dict(convnext_pair=True)
    assert _can(_mm(**on), _db(**on)) is True
    assert _can(_mm("2_2_2", **on), _db("2_2_2", **on)) is True
    # the switch in one model only
    assert _can(_mm(**on), _db()) is False and _can(_mm(), _db(**on)) is False
    # different block counts, different precisions
    assert _can(_mm("1_2_1", **on), _db("1_1_1", **on)) is False
    assert _can(_mm(convnext_precision=4, **on), _db(convnext_precision=3, **on)) is False
    assert _can(_mm(convnext_precision=4, **on), _db(convnext_precision=4, **on)) is True
    # a ResNet on either side
    assert _can(MM(opt=Options(**on)).eval(), _db(**on)) is False
    assert _can(_mm(**on), _db("2_2_2", fe="resnet18", **on)) is False
    # a ConvNeXt range-guard tag that would bind (precision 4 with convnext_range_guard), on either model
    g = dict(convnext_precision=4, convnext_range_guard=True, **on)
    assert _can(_mm(**g), _db(convnext_precision=4, **on)) is False
    assert _can(_mm(convnext_precision=4, **on), _db(**g)) is False
    assert _can(_mm(convnext_range_guard=True, **on), _db(convnext_range_guard=True, **on)) is True      # precision 3: binds nothing
    # db_map 5-D or 6-D; at most four trunks; the share_dbfe / nmap rule; training is never paired
    assert _can(_mm(**on), _db(**on), {"db_map": torch.zeros(1, 2, 1, 3, 32, 32)}) is True
    assert _can(_mm(**on), _db(**on), {"db_map": torch.zeros(1, 3, 32, 32)}) is False
    three = {"db_map": torch.zeros(1, 3, 3, 32, 32)}
    assert _can(_mm(**on), _db(maptype="a_b_c", **on), three) is True
    assert _can(_mm(**on), _db(maptype="a_b_c_d", **on), {"db_map": torch.zeros(1, 4, 3, 32, 32)}) is False
    assert _can(_mm(**on), _db(maptype="a_b_c", share_dbfe=True, **on), three) is False
    assert pair.can_pair(_mm(**on), _db(**on), QDATA, DBDATA) is False                                   # gradients enabled
    # uint8 tiles need Options.convnext_u8 on the model concerned (else the separate forwards refuse them by name)
    u8 = {"db_map": torch.zeros(1, 1, 32, 32, 3, dtype=torch.uint8)}
    assert _can(_mm(**on), _db(**on), u8) is False and _can(_mm(**on), _db(convnext_u8=True, **on), u8) is True
