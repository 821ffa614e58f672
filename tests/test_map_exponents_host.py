"""Host-side logic of the map exponents (agplace_amd/map_exponents.py): choosing, naming, installing, folding.  No GPU."""
import json
import math

import pytest
import torch

from agplace_amd import map_exponents as me
from agplace_amd import ops

F16 = 65504.0


def test_thresholds_on_both_sides_of_a_power_of_two():
    # headroom 2: a map may peak at 65504 / 4 = 16376 and stay at exponent 0; every doubling beyond costs one
    assert me.choose_exponents({"a": F16 / 4})["a"] == 0
    assert me.choose_exponents({"a": math.nextafter(F16 / 4, math.inf)})["a"] == 1
    assert me.choose_exponents({"a": F16 / 2})["a"] == 1
    assert me.choose_exponents({"a": math.nextafter(F16 / 2, math.inf)})["a"] == 2
    for e in range(1, 12):
        m = F16 / 4 * 2.0 ** e
        assert me.choose_exponents({"a": m})["a"] == e
        assert me.choose_exponents({"a": math.nextafter(m, math.inf)})["a"] == e + 1
        assert me.choose_exponents({"a": math.nextafter(m, 0.0)})["a"] == e
    # the closed form e = max(0, ceil(log2(m * 2^headroom_bits / 65504))), where its logarithm is not at a rounding edge
    for m in (1.0, 3.0e4, 1.0e5, 2.0 ** 17, 2.0 ** 22 - 1, 7.7e8):
        assert me.choose_exponents({"a": m})["a"] == max(0, math.ceil(math.log2(m * 4 / F16)))


def test_headroom_bits_is_policy():
    m = 2.0 ** 18
    es = [me.choose_exponents({"a": m}, headroom_bits=hb)["a"] for hb in range(5)]
    assert es == [es[0] + hb for hb in range(5)] and es[0] == 3          # 2^18 / 2^3 = 32768 <= 65504 < 2^18 / 2^2
    assert me.choose_exponents({"a": F16}, headroom_bits=0)["a"] == 0
    with pytest.raises(ValueError):
        me.choose_exponents({"a": 1.0}, headroom_bits=-1)
    with pytest.raises(ValueError):
        me.choose_exponents({"a": 1.0}, headroom_bits=1.5)


def test_group_takes_the_maximum_of_its_members_and_small_maps_give_zero():
    absmax = {"stem": 10.0, "l1.0.out": 3.0e5, "l1.1.out": 2.0e4, "l1.0.conv1": 5.0, "l2.0.out": 1.0e-3, "l2.0.conv1": 0.0}
    groups = {"l1": ["stem", "l1.0.out", "l1.1.out"], "l2": ["l2.0.out", "l2.0.downsample"], "l3": ["never.measured"]}
    got = me.choose_exponents(absmax, groups)
    assert got == {"l1": me.choose_exponents({"x": 3.0e5})["x"], "l2": 0, "l3": 0, "l1.0.conv1": 0, "l2.0.conv1": 0}
    assert got["l1"] == 5                                                  # 3e5 * 4 / 65504 = 18.3 -> 2^5
    assert all(isinstance(v, int) for v in got.values())
    json.dumps(got)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -1.0])
def test_nan_inf_negative_maxima_raise(bad):
    with pytest.raises(ValueError, match="measured maximum"):
        me.choose_exponents({"a": 1.0, "b": bad})
    with pytest.raises(ValueError, match="measured maximum"):
        me.choose_exponents({"a": 1.0, "b": bad}, {"g": ["a", "b"]})


def _mm():
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    return MM(opt=Options())


def test_names_grouping_and_round_trip_on_mm():
    m = _mm()
    groups, alone = me.map_names(m)
    assert groups["image_fe.layer1"] == ["image_fe.stem", "image_fe.layer1.0.out", "image_fe.layer1.1.out"]
    assert groups["image_fe.layer2"][0] == "image_fe.layer2.0.downsample"
    # the stage-2 block's input and output sit in the last stage's residual chain
    assert groups["image_fe.layer3"][-2:] == ["stg2.0.in", "stg2.0.out"]
    assert "image_fe.layer1.0.conv1" in alone and "stg2.0.conv1" in alone
    keys0 = set(m.state_dict())
    d = me.get_exponents(m)
    assert set(d) == set(groups) | set(alone) and not any(d.values())
    d["image_fe.layer3"], d["stg2.0.conv1"], d["image_fe.layer2.1.conv1"] = 3, 2, 1
    assert me.set_exponents(m, json.loads(json.dumps(d))) == d
    assert me.get_exponents(m) == d
    assert set(m.state_dict()) == keys0                                    # not parameters, not buffers
    assert m.stg2fuseblock.ffnsimg[0]._map_exp == {"conv1": 2}
    me.clear_exponents(m)
    assert not any(me.get_exponents(m).values())
    with pytest.raises(ValueError):
        me.set_exponents(m, {"image_fe.layer9": 1})
    with pytest.raises(ValueError):
        me.set_exponents(m, {"image_fe.layer1": -1})
    with pytest.raises(ValueError):
        me.set_exponents(m, {"image_fe.layer1": 1.5})


def test_bottleneck_names():
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.options import Options
    db = DBVanilla2D("db", 256, opt=Options(dbimage_fe="resnet50"))
    groups, alone = me.map_names(db)
    assert groups["dbimage_fes.0.layer1"][:3] == ["dbimage_fes.0.stem", "dbimage_fes.0.layer1.0.downsample", "dbimage_fes.0.layer1.0.out"]
    assert "dbimage_fes.0.layer2.3.conv1" in alone and "dbimage_fes.0.layer2.3.conv2" in alone
    assert "dbimage_fes.0.layer2.3.conv3" not in alone


def test_exponents_are_part_of_the_cache_key_and_fold_exactly():
    from agplace_amd.resnet import ResNet
    torch.manual_seed(0)
    net = ResNet("resnet18", nstages=3)
    for bn in [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]:
        bn.weight.data.uniform_(0.5, 1.5)
        bn.bias.data.normal_()
    k0 = net._version_key()
    p0 = net._prepared(scaled=True)
    assert net._prepared(scaled=False) is p0                               # no exponent set: ONE set of constants
    me.set_exponents(net, {"layer1": 2, "layer2": 5, "layer2.0.conv1": 3, "layer3": 1})
    assert net._version_key() != k0
    p1 = net._prepared(scaled=True)
    pu = net._prepared(scaled=False)                                       # mode 3 / training: unscaled
    assert p1 is not pu and all(v == 0 for v in pu["exp"].values())

    def same(a, b):
        return torch.equal(a, b)
    for key in [k for k in p0 if k != "exp"]:
        a, b = (p0[key], pu[key]) if key == "stem" else (p0[key][0] + [p0[key][1]], pu[key][0] + [pu[key][1]])
        for x, y in zip(a if isinstance(a, list) else [a], b if isinstance(b, list) else [b]):
            if x is not None:
                assert same(x.scale, y.scale) and same(x.shift, y.shift)
    # stem: writes layer1's group (2); layer2.0: conv1 2 -> 3, conv2 3 -> 5, downsample 2 -> 5; layer3.0.conv1 5 -> 0
    s = p0["stem"]
    assert same(p1["stem"].scale, s.scale / 4) and same(p1["stem"].shift, s.shift / 4)
    (c1, c2), ds = p1[(1, 0)]
    (u1, u2), uds = pu[(1, 0)]
    assert same(c1.scale, u1.scale * 2.0 ** (2 - 3)) and same(c1.shift, u1.shift * 2.0 ** -3)
    assert same(c2.scale, u2.scale * 2.0 ** (3 - 5)) and same(c2.shift, u2.shift * 2.0 ** -5)
    assert same(ds.scale, uds.scale * 2.0 ** (2 - 5)) and same(ds.shift, uds.shift * 2.0 ** -5)
    assert same(p1[(2, 0)][0][0].scale, pu[(2, 0)][0][0].scale * 2.0 ** 5) and same(p1[(2, 0)][0][0].shift, pu[(2, 0)][0][0].shift)
    assert p1["exp"][(1, 0, 0)] == 3 and p1["exp"][(1, 1, 1)] == 5 and p1["exp"][("ds", 2, 0)] == 1 and p1["exp"]["stem"] == 2
    me.clear_exponents(net)
    assert net._version_key() == k0


def test_fold_exp_identity_and_splitmap_default():
    s, t = torch.rand(8), torch.rand(8)
    a, b = ops.fold_exp(s, t, 0, 0)
    assert a is s and b is t
    m = ops.SplitMap(None, None, 1, 2, 2, 8, 1)
    assert m.exp == 0
