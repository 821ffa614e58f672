"""-m gpu tests of the map exponents (agplace_amd/map_exponents.py): the abs-max kernel, calibration of a checkpoint whose maps
leave fp16's range, bit-neutrality on a healthy one, forced exponents, GeM folding, captured replays, mode 3 / training, and the
launch census.  Descriptor bars are those of the mode-4 model tests (tests/test_gpu_models.py)."""
import collections
import math

import pytest
import torch

from oracle import nets, resnet as oresnet
from gpu_util import cpu_state, elem_rel, frac_within, randomize_bn, rel_l2, rel_max, to_dev

pytestmark = pytest.mark.gpu

TOL = 1e-3                      # tests/test_gpu_models.py: TOL, and for mode 4 elem_rel < 0.15, frac_within(2e-2) >= 0.99
ETOL4, RTOL4 = 0.15, 2e-2
FE_BOUND4 = (1e-3, 4e-3)        # tests/test_gpu_models.py FE_BOUNDS[2] = FE_BOUNDS[4]: the op-level export's map bar (rel_l2, rel_max)


@pytest.fixture(autouse=True)
def _inference_mode(request):
    if "train" in request.node.name:
        yield
    else:
        with torch.no_grad():
            yield


def _assert_mm_bars(out, ref, tag):
    """The bars of test_mm_forward_q_matches_oracle at mfma_precision = 4."""
    assert set(out.keys()) == set(ref.keys())
    for k in ref:
        figs = (rel_l2(out[k], ref[k]), rel_max(out[k], ref[k]), elem_rel(out[k], ref[k]), frac_within(out[k], ref[k], RTOL4))
        print(f"MAPEXP {tag} {k}: rel_l2 {figs[0]:.2e} rel_max {figs[1]:.2e} elem_rel {figs[2]:.2e} frac_within {figs[3]:.4f}")
        assert figs[0] < TOL and figs[1] < TOL, (tag, k, figs)
        assert figs[2] < ETOL4, (tag, k, figs)
        assert figs[3] >= 0.99, (tag, k, figs)


def _assert_db_bars(out, ref, tag):
    """The bars of test_dbvanilla2d_matches_oracle."""
    figs = (rel_l2(out, ref), rel_max(out, ref))
    print(f"MAPEXP {tag} db embedding: rel_l2 {figs[0]:.2e} rel_max {figs[1]:.2e}")
    assert out.shape == ref.shape
    assert figs[0] < TOL and figs[1] < TOL, (tag, figs)


# ------------------------------------------------------------------ 1. the abs-max kernel
@pytest.mark.parametrize("prec", [3, 4])
@pytest.mark.parametrize("n,c,h,w,pad", [(1, 8, 1, 1, 1), (3, 24, 7, 13, 1), (2, 64, 17, 31, 1), (5, 256, 9, 11, 1), (2, 40, 5, 3, 3),
                                         (2, 128, 56, 336, 1)])
def test_map_absmax_equals_torch(dev, prec, n, c, h, w, pad):
    from agplace_amd import ops
    g = torch.Generator().manual_seed(n * 1000 + c)
    x = torch.randn(n, c, h, w, generator=g) * 37.0
    x[n - 1, c - 1, h - 1, w - 1] = -4320.0                       # the maximum is a NEGATIVE value in the last vector
    m = ops.pack_f32(x.to(dev), c, pad, prec)
    word = torch.empty(3, dtype=torch.float32, device=dev)
    ops.absmax_reset(word)
    assert torch.equal(word.cpu(), torch.zeros(3))
    ops.map_absmax(m, word[1:2])
    want = m.to_f32().abs().max()
    assert float(want) == 4320.0
    assert torch.equal(word.cpu(), torch.tensor([0.0, float(want), 0.0]))        # exact: a maximum has no rounding
    # accumulation: a smaller map leaves the word, a larger one raises it
    y = torch.randn(n, c, h, w, generator=g)
    my = ops.pack_f32(y.to(dev), c, pad, prec)
    ops.map_absmax(my, word[1:2])
    assert float(word[1]) == 4320.0
    y[0, 0, 0, 0] = 5.0e4
    my = ops.pack_f32(y.to(dev), c, pad, prec)
    ops.map_absmax(my, word[1:2])
    assert float(word[1]) == float(my.to_f32().abs().max()) > 4320.0
    # an image slice of a map (what a chunked stage-1 pass hands over)
    if n > 1:
        ops.absmax_reset(word)
        ops.map_absmax(ops.slice_map(m, 0, n - 1), word[0:1])
        assert float(word[0]) == float(m.to_f32()[: n - 1].abs().max())


def test_map_absmax_propagates_nan_and_rejects_bad_arguments(dev):
    from agplace_amd import _lib, ops
    from agplace_amd import map_exponents as me
    x = torch.randn(2, 16, 5, 5)
    x[1, 3, 2, 2] = float("nan")
    m = ops.pack_f32(x.to(dev), 16, 1, 3)
    word = torch.empty(1, dtype=torch.float32, device=dev)
    ops.absmax_reset(word)
    ops.map_absmax(m, word)
    assert math.isnan(float(word[0]))                             # NaN patterns sort above +inf in the unsigned order: they stick
    ops.map_absmax(ops.pack_f32(torch.ones(2, 16, 5, 5, device=dev), 16, 1, 3), word)
    assert math.isnan(float(word[0]))
    with pytest.raises(ValueError):
        me.choose_exponents({"a": float(word[0])})
    L = _lib.load()
    assert L.agp_map_absmax(m.hi.data_ptr(), None, 2, 5, 5, 12, 1, word.data_ptr(), _lib.stream()) != 0      # c % 8
    assert L.agp_map_absmax(None, None, 2, 5, 5, 16, 1, word.data_ptr(), _lib.stream()) != 0


# ------------------------------------------------------------------ the oracle's maxima
class _OracleMaxima:
    """Records max |x| of every map the fp32 CPU oracle forms while it computes the reference outputs: the post-ReLU maps
    (oracle.resnet._relu keys "relu", "layerL.B.reluK", "<prefix>relu1/2" of the stage-2 block), the downsample outputs
    (oracle.resnet._bn of "...downsample.1") and the stage-2 block's input.  One dict per oracle trunk call, in call order."""

    def __init__(self, monkeypatch):
        self.calls = []
        relu0, bn0, fr0, bb0 = oresnet._relu, oresnet._bn, oresnet.forward_resnet, nets.basic_block_conv
        me = self

        def relu(z, pattern, key):
            o = relu0(z, pattern, key)
            me.calls[-1][key] = max(me.calls[-1].get(key, 0.0), float(o.abs().max()))
            return o

        def bn(x, p, name, training=False):
            o = bn0(x, p, name, training)
            if "downsample" in name:
                me.calls[-1][name] = float(o.abs().max())
            return o

        def forward_resnet(*a, **k):
            me.calls.append({})
            return fr0(*a, **k)

        def basic_block_conv(x, params, prefix, *a, **k):
            me.calls[-1][prefix + "in"] = float(x.abs().max())
            return bb0(x, params, prefix, *a, **k)
        monkeypatch.setattr(oresnet, "_relu", relu)
        monkeypatch.setattr(oresnet, "_bn", bn)
        monkeypatch.setattr(oresnet, "forward_resnet", forward_resnet)
        monkeypatch.setattr(nets, "basic_block_conv", basic_block_conv)

    @staticmethod
    def named(rec, prefix, kind, nblocks, stg2=False):
        """A recorded call as {our map name: maximum}."""
        out = {prefix + "stem": rec["relu"]}
        last = 2 if kind == "basic" else 3
        for li, nb in enumerate(nblocks):
            for bi in range(nb):
                pre = f"layer{li + 1}.{bi}."
                for k in range(1, last):
                    out[f"{prefix}{pre}conv{k}"] = rec[f"{pre}relu{k}"]
                out[f"{prefix}{pre}out"] = rec[f"{pre}relu{last}"]
                if pre + "downsample.1" in rec:
                    out[f"{prefix}{pre}downsample"] = rec[pre + "downsample.1"]
        if stg2:
            s = "stg2fuseblock.ffnsimg.0."
            out["stg2.0.in"], out["stg2.0.conv1"], out["stg2.0.out"] = rec[s + "in"], rec[s + "relu1"], rec[s + "relu2"]
        return out


def _check_chosen(got, oracle_absmax, groups, tag):
    """`got` (calibrated on the GPU in mode 3) against choose_exponents on the oracle's maxima: non-zero exactly where the oracle
    demands it, and the same exponent wherever the oracle's maximum is not within 1e-3 of a power-of-two threshold (mode 3
    measures the maps to ~1e-5)."""
    from agplace_amd import map_exponents as me
    want = me.choose_exponents(oracle_absmax, groups)
    print(f"MAPEXP {tag} exponents", {k: v for k, v in got.items() if v}, "oracle", {k: v for k, v in want.items() if v})
    assert set(got) == set(want)
    members = dict(groups)
    for k in want:
        m = max(oracle_absmax[n] for n in members.get(k, [k]) if n in oracle_absmax)
        lo = me.choose_exponents({"x": m * (1 - 1e-3)})["x"]
        hi = me.choose_exponents({"x": m * (1 + 1e-3)})["x"]
        if lo == hi:
            assert got[k] == want[k], (tag, k, got[k], want[k], m)
            assert (got[k] != 0) == (m * 4 > 65504.0)
        else:
            assert got[k] in (lo, hi), (tag, k, got[k], lo, hi, m)


HOT = 2.0 ** 15


def _hot_pair(dev, dbfe="resnet18", guard=True):
    """A ResNet18 MM and a DBVanilla2D with randomized BatchNorm statistics whose layer2.0.bn1 affine terms are inflated by 2^15:
    from that block-internal map on, every map of the image path is ~2^15 times its ordinary size."""
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    opt = Options(mfma_precision=4, fp16_range_guard=guard, dbimage_fe=dbfe)
    torch.manual_seed(31)
    modelq = randomize_bn(MM(opt=opt))
    modeldb = randomize_bn(DBVanilla2D("db", opt.features_dim, opt=opt), seed=1)
    for bn in (modelq.image_fe.fe.layer2[0].bn1, modeldb.dbimage_fes[0].fe.layer2[0].bn1):
        bn.weight.data *= HOT
        bn.bias.data *= HOT
    return modelq.to(dev).eval(), modeldb.to(dev).eval(), opt


def _in_hot_band(v):
    return 2.0 ** 17 <= v <= 2.0 ** 22


# ------------------------------------------------------------------ 2. the test that fails without the feature
def test_hot_checkpoint_runs_in_mode4_after_calibration(dev, monkeypatch):
    """A checkpoint whose maps peak at 2^17 .. 2^22 in the fp32 oracle: mode 4 alone saturates (the guard raises); after
    map_exponents.calibrate the guard is silent and every descriptor meets the mode-4 bars against the oracle -- separately,
    through pair.embed_pair, for 5-D and 6-D database input."""
    from agplace_amd import map_exponents as me
    from agplace_amd import pair
    modelq, modeldb, opt = _hot_pair(dev)
    data = nets.synth_query(3, 64, 192, opt, seed=5)
    tiles5 = torch.randn(3, 1, 3, 64, 64, generator=torch.Generator().manual_seed(6))
    tiles6 = torch.randn(2, 2, 1, 3, 64, 64, generator=torch.Generator().manual_seed(7))
    # ---- the oracle first: outputs, and the maxima of its maps
    rec = _OracleMaxima(monkeypatch)
    ref_q = nets.mm_forward_q(data, cpu_state(modelq), opt)
    ref_5 = nets.dbvanilla2d_forward_db({"db_map": tiles5}, cpu_state(modeldb), opt)["embedding"]
    ref_6 = nets.dbvanilla2d_forward_db({"db_map": tiles6}, cpu_state(modeldb), opt)["embedding"]
    mq = rec.named(rec.calls[0], "image_fe.", "basic", [2, 2, 2], stg2=True)
    m5 = rec.named(rec.calls[1], "dbimage_fes.0.", "basic", [2, 2, 2])
    m6 = rec.named(rec.calls[2], "dbimage_fes.0.", "basic", [2, 2, 2])
    mdb = {k: max(m5[k], m6[k]) for k in m5}
    for tag, mm in (("query", mq), ("db", mdb)):
        pre = "image_fe." if tag == "query" else "dbimage_fes.0."
        stage_outs = [mm[pre + "layer2.1.out"], mm[pre + "layer3.1.out"]]
        internal = [v for k, v in mm.items() if k.endswith("conv1")]
        print(f"MAPEXP oracle maxima {tag}", {k: f"{v:.3g}" for k, v in mm.items()})
        assert any(_in_hot_band(v) for v in stage_outs), (tag, stage_outs)          # not vacuous: the oracle's maps ARE hot ...
        assert any(_in_hot_band(v) for v in internal), (tag, internal)
        assert max(mm.values()) <= 2.0 ** 22
        assert mm[pre + "layer1.1.out"] * 4 < 65504.0                               # ... and layer 1 is not
    for r in list(ref_q.values()) + [ref_5, ref_6]:
        assert bool(torch.isfinite(r).all())
    dq, d5, d6 = to_dev(data, dev), {"db_map": tiles5.to(dev)}, {"db_map": tiles6.to(dev)}
    # ---- (a) mode 4 without exponents: the guard raises (a stream's first guarded forward reports its own batch)
    with pytest.raises(ValueError, match="map_exponents.calibrate"):
        modelq(dq, mode="q")
    with pytest.raises(ValueError, match="fp16's range"):
        modeldb(d5, mode="db")
    # ---- (b) calibrated
    eq = me.calibrate(modelq, [dq])
    edb = me.calibrate(modeldb, [d5, d6])
    assert opt.mfma_precision == 4
    assert eq == me.get_exponents(modelq) and edb == me.get_exponents(modeldb)
    _check_chosen(eq, mq, me.map_names(modelq)[0], "query")
    _check_chosen(edb, mdb, me.map_names(modeldb)[0], "db")
    assert eq["image_fe.layer1"] == 0 and eq["image_fe.layer2"] > 0 and eq["image_fe.layer2.0.conv1"] > 0 and eq["stg2.0.conv1"] > 0
    out_q = modelq(dq, mode="q")
    out_5 = modeldb(d5, mode="db")["embedding"]
    out_6 = modeldb(d6, mode="db")["embedding"]
    _assert_mm_bars(out_q, ref_q, "hot/calibrated")
    _assert_db_bars(out_5, ref_5, "hot/calibrated 5-D")
    _assert_db_bars(out_6, ref_6, "hot/calibrated 6-D")
    pq, p5 = pair.embed_pair(modelq, modeldb, dq, d5)
    _assert_mm_bars(pq, ref_q, "hot/calibrated pair")
    _assert_db_bars(p5["embedding"], ref_5, "hot/calibrated pair")
    for k in out_q:
        assert torch.equal(pq[k], out_q[k]), k                   # lock-step trunks: bit-identical to the separate forwards
    assert torch.equal(p5["embedding"], out_5)
    modelq(dq, mode="q")                                         # (eager reports come one call late)
    modeldb(d5, mode="db")
    modelq.poll_fp16_range()
    assert modelq.fp16_range_ok() and modeldb.fp16_range_ok()    # the guard is silent
    # the per-op vector path (Options.fused_vector_path = False) restores the same factors with small launches of its own
    opt.fused_vector_path = False
    _assert_mm_bars(modelq(dq, mode="q"), ref_q, "hot/calibrated per-op")
    _assert_db_bars(modeldb(d5, mode="db")["embedding"], ref_5, "hot/calibrated per-op")
    opt.fused_vector_path = True
    # cleared again: the same forward saturates again
    me.clear_exponents(modelq)
    modelq(dq, mode="q")
    assert not modelq.fp16_range_ok()
    with pytest.raises(ValueError, match="fp16's range"):
        modelq(dq, mode="q")


def test_hot_resnet50_database_network(dev, monkeypatch):
    """Bottleneck grouping: conv1 and conv2 outputs stand alone, the 4x-wide block outputs and the downsample share the group."""
    from agplace_amd import map_exponents as me
    _, modeldb, opt = _hot_pair(dev, dbfe="resnet50")
    tiles = torch.randn(2, 1, 3, 64, 64, generator=torch.Generator().manual_seed(8))
    rec = _OracleMaxima(monkeypatch)
    ref = nets.dbvanilla2d_forward_db({"db_map": tiles}, cpu_state(modeldb), opt)["embedding"]
    mdb = rec.named(rec.calls[0], "dbimage_fes.0.", "bottleneck", [3, 4, 6])
    print("MAPEXP oracle maxima resnet50", {k: f"{v:.3g}" for k, v in mdb.items()})
    assert any(_in_hot_band(mdb[f"dbimage_fes.0.layer{L}.{b}.out"]) for L, b in ((2, 3), (3, 5)))
    assert any(_in_hot_band(v) for k, v in mdb.items() if k.endswith(("conv1", "conv2")))
    assert bool(torch.isfinite(ref).all())
    d = {"db_map": tiles.to(dev)}
    with pytest.raises(ValueError, match="map_exponents.calibrate"):
        modeldb(d, mode="db")
    e = me.calibrate(modeldb, [d])
    _check_chosen(e, mdb, me.map_names(modeldb)[0], "resnet50")
    assert e["dbimage_fes.0.layer2.0.conv1"] > 0 and e["dbimage_fes.0.layer2.0.conv2"] > 0 and e["dbimage_fes.0.layer3"] > 0
    out = modeldb(d, mode="db")["embedding"]
    _assert_db_bars(out, ref, "hot resnet50")
    modeldb(d, mode="db")
    assert modeldb.fp16_range_ok()


# ------------------------------------------------------------------ 3. healthy checkpoint: nothing changes
def _healthy_pair(dev, seed=3, **kw):
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    opt = Options(mfma_precision=4, **kw)
    torch.manual_seed(seed)
    modelq = randomize_bn(MM(opt=opt)).to(dev).eval()
    modeldb = randomize_bn(DBVanilla2D("db", opt.features_dim, opt=opt), seed=1).to(dev).eval()
    return modelq, modeldb, opt


def _prep_tensors(model):
    """Every prepared scale / shift tensor of a model's image path at mode 4."""
    from agplace_amd import map_exponents as me
    out = []
    for _, owner in me._parts(model):
        if hasattr(owner, "nstages"):
            p = owner._prepared(scaled=True)
            cws = [p["stem"]] + [cw for k, v in p.items() if isinstance(k, tuple) and k != "exp" and isinstance(v, tuple)
                                 for cw in v[0] + ([v[1]] if v[1] is not None else [])]
        else:
            cws = owner._cw
        out += [t for cw in cws for t in (cw.scale, cw.shift)]
    return out


def test_healthy_checkpoint_calibrates_to_zero_and_stays_bit_equal(dev):
    from agplace_amd import map_exponents as me
    modelq, modeldb, opt = _healthy_pair(dev)
    data = to_dev(nets.synth_query(3, 64, 192, opt, seed=5), dev)
    tiles = {"db_map": torch.randn(3, 1, 3, 64, 64, generator=torch.Generator().manual_seed(6)).to(dev)}
    out0 = {k: v.clone() for k, v in modelq(data, mode="q").items()}
    db0 = modeldb(tiles, mode="db")["embedding"].clone()
    prep0 = _prep_tensors(modelq) + _prep_tensors(modeldb)
    eq, edb = me.calibrate(modelq, [data]), me.calibrate(modeldb, [tiles])
    assert not any(eq.values()) and not any(edb.values())
    prep1 = _prep_tensors(modelq) + _prep_tensors(modeldb)
    assert len(prep0) == len(prep1) and all(a is b for a, b in zip(prep0, prep1))       # not even re-folded
    out1 = modelq(data, mode="q")
    for k in out0:
        assert torch.equal(out0[k], out1[k]), k
    assert torch.equal(db0, modeldb(tiles, mode="db")["embedding"])
    # an explicit all-zero dict re-keys nothing either; the values stay the same bits
    me.set_exponents(modelq, eq)
    for a, b in zip(prep0, _prep_tensors(modelq) + _prep_tensors(modeldb)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 4. forced exponents on a healthy checkpoint
def test_forced_exponents_meet_the_bars_and_exports_keep_true_scale(dev):
    """Exponent 3 on every group and internal map of a healthy checkpoint: descriptors meet the mode-4 bars; the op-level
    ImageFE.forward export shows the true scale.  Scaling is exact except where a stored value falls into fp16's subnormal
    range (below 2^-14 * 2^3 true size), so bit equality is not demanded; the measured difference is printed."""
    from agplace_amd import map_exponents as me
    from agplace_amd import pair
    from agplace_amd.network_mm.image_fe import ImageFE
    modelq, modeldb, opt = _healthy_pair(dev)
    data = nets.synth_query(3, 64, 192, opt, seed=5)
    tiles = torch.randn(3, 1, 3, 64, 64, generator=torch.Generator().manual_seed(6))
    ref_q = nets.mm_forward_q(data, cpu_state(modelq), opt)
    ref_db = nets.dbvanilla2d_forward_db({"db_map": tiles}, cpu_state(modeldb), opt)["embedding"]
    dq, dd = to_dev(data, dev), {"db_map": tiles.to(dev)}
    out0 = {k: v.clone() for k, v in modelq(dq, mode="q").items()}
    db0 = modeldb(dd, mode="db")["embedding"].clone()
    me.set_exponents(modelq, {k: 3 for k in me.get_exponents(modelq)})
    me.set_exponents(modeldb, {k: 3 for k in me.get_exponents(modeldb)})
    out3 = modelq(dq, mode="q")
    db3 = modeldb(dd, mode="db")["embedding"]
    _assert_mm_bars(out3, ref_q, "forced 3")
    _assert_db_bars(db3, ref_db, "forced 3")
    p3, pd3 = pair.embed_pair(modelq, modeldb, dq, dd)
    for k in out3:
        assert torch.equal(p3[k], out3[k])
    assert torch.equal(pd3["embedding"], db3)
    print("MAPEXP forced-3 vs exponent-0 rel_l2:", " ".join(f"{k}:{rel_l2(out3[k], out0[k]):.2e}" for k in out0),
          f"db:{rel_l2(db3, db0):.2e}")
    # the op-level export (its default precision: the tight mode 2, which shares the fp16 maps and honours the exponents)
    torch.manual_seed(9)
    fe = randomize_bn(ImageFE("resnet18", "2_2_2")).to(dev).eval()
    x = torch.randn(2, 3, 64, 96)
    params = {k: v.double() for k, v in cpu_state(fe).items()}
    refs = oresnet.forward_resnet(x.double(), params, "resnet18", 3, prefix="fe.")
    last0, maps0 = fe(x.to(dev))
    maps0 = [m.clone() for m in maps0]
    me.set_exponents(fe, {k: 3 for k in me.get_exponents(fe)})
    stored = fe.forward_maps(x.to(dev), prec=2)
    assert all(m.exp == 3 for m in stored)
    last3, maps3 = fe(x.to(dev))
    for i, (a, b, r) in enumerate(zip(maps3, maps0, refs)):
        print(f"MAPEXP export l{i + 1}: forced-3 vs exponent-0 rel_l2 {rel_l2(a, b):.2e}; vs oracle rel_l2 {rel_l2(a, r):.2e} "
              f"rel_max {rel_max(a, r):.2e}")
        assert rel_l2(a, r) < FE_BOUND4[0] and rel_max(a, r) < FE_BOUND4[1]
        assert rel_l2(a, b) < FE_BOUND4[0] and rel_max(a, b) < FE_BOUND4[1]
    # mode 3 ignores the exponents: same bits as without
    me.clear_exponents(fe)
    a3 = [m.to_f32().clone() for m in fe.forward_maps(x.to(dev), prec=3)]
    me.set_exponents(fe, {k: 3 for k in me.get_exponents(fe)})
    b3 = fe.forward_maps(x.to(dev), prec=3)
    assert all(m.exp == 0 for m in b3) and all(torch.equal(a, b.to_f32()) for a, b in zip(a3, b3))


# ------------------------------------------------------------------ 5. GeM folding
@pytest.mark.parametrize("p", [1.0, 3.0])
@pytest.mark.parametrize("fused", [False, True])
def test_gem_with_exponent_equals_gem_without(dev, p, fused):
    """A post-ReLU map with many zeros (where the eps clamp decides) pooled at exponent 0 and -- the same true values stored times
    2^-4 -- at exponent 4, through ops.pool_map and through the conv epilogue (ops.PoolReq).
    The mean is a sum of exactly scaled terms: bit-equal, asserted.
    GeM clamps and (p = 3) cubes exactly scaled terms too, but the kernels take the p-th root as exp2(log2(s) / p) in fp32
    (csrc/pool.hip) -- and for p != 3 the power as exp2(p log2(v)) --, which is not homogeneous: storing times 2^-4 moves log2(s) by
    4 p, and the moved logarithm rounds differently.  Bit equality therefore cannot hold without changing those kernels; the bound
    below is the rounding of that root: with |log2 s| < 64 (asserted on the data) one ulp of a logarithm is at most 2^-18; the
    per-element logarithms of the p != 3 power average out in the sum and are covered by the same term; two logarithm roundings,
    one division and two exp2 roundings give a relative difference below ln 2 * 3 * 2^-18 + 2 * 2^-23 < 1.0e-5.
    A WRONG eps fold is a factor 2^4 on every all-zero channel (GeM = eps there), five orders of magnitude above the bound.
    Measured on an MI355X: 2.0e-7 (p = 3) and 3.5e-7 .. 4.0e-7 (p = 1) relative, not bit-equal; the mean bit-equal."""
    from agplace_amd import ops
    g = torch.Generator().manual_seed(5)
    n, c, h, w = 3, 64, 12, 20
    x = torch.relu(torch.randn(n, c, h, w, generator=g) - 1.0) * 8.0        # ~84 % zeros
    x[:, :8] = 0.0                                                          # all-zero channels: GeM = eps exactly
    x = (x * 64).round() / 64                                               # few mantissa bits: x and x / 16 are both exact in fp16
    pt = torch.tensor([p], device=dev)
    eps = ops.GEM_EPS
    if not fused:
        m0 = ops.pack_f32(x.to(dev), c, 1, 4)
        m4 = ops.pack_f32((x / 16).to(dev), c, 1, 4)
        m4.exp = 4
        assert torch.equal(m0.to_f32(), m4.to_f32())
        mean0, gem0 = ops.pool_map(m0, pt, eps=eps)
        mean4, gem4 = ops.pool_map(m4, pt, eps=eps)
        raw_mean4, raw_gem4 = ops.pool_map(m4, pt, eps=eps, raw=True)
        assert torch.equal(raw_mean4 * 16, mean4) and torch.equal(raw_gem4 * 16, gem4)
    else:
        # identity 3x3 conv (centre tap 1) with scale 1 / shift 0 writes the same map; its epilogue pools it
        wgt = torch.zeros(c, c, 3, 3)
        wgt[torch.arange(c), torch.arange(c), 1, 1] = 1.0
        res = []
        for e in (0, 4):
            xin = ops.pack_f32(x.to(dev), c, 1, 4)
            s, t = ops.fold_exp(torch.ones(c, device=dev), torch.zeros(c, device=dev), 0, e)
            cw = ops.ConvWeights(wgt.to(dev), s, t, 1, 1)
            out = ops.SplitMap.alloc(n, h, w, c, 1, 4, dev)
            out.exp = e
            req = ops.PoolReq(pt, eps=eps, want_mean=True, want_gem=True)
            ops.conv2d(xin, cw, out, relu=True, prec=4, pool=req)
            assert req.fused and req.exp == e
            assert torch.equal(out.to_f32(), x.to(dev))
            res.append((req.true_mean(), req.true_gem()))
        (mean0, gem0), (mean4, gem4) = res
    assert torch.equal(mean0, mean4)
    s0 = (gem0.double() ** p)
    assert float(s0.log2().abs().max()) < 64
    assert rel_max(gem0[:, :8], torch.full((n, 8), eps)) < 1e-5 and rel_max(gem4[:, :8], torch.full((n, 8), eps)) < 1e-5
    d = ((gem4.double() - gem0.double()).abs() / gem0.double()).max()
    print(f"MAPEXP gem p={p} fused={fused}: max relative difference exponent 4 vs 0 = {float(d):.2e}, bit-equal {torch.equal(gem0, gem4)}")
    assert float(d) < 1.0e-5


# ------------------------------------------------------------------ 6. captured replays, mode 3, training
def test_captured_pair_after_set_exponents_replays_the_eager_forward(dev):
    from agplace_amd import map_exponents as me
    from agplace_amd import pair
    modelq, modeldb, opt = _hot_pair(dev)
    data = to_dev(nets.synth_query(4, 64, 192, opt, seed=5), dev)
    tiles = {"db_map": torch.randn(4, 1, 3, 64, 64, generator=torch.Generator().manual_seed(6)).to(dev)}
    me.calibrate(modelq, [data])
    me.calibrate(modeldb, [tiles])
    eq, ed = pair.embed_pair(modelq, modeldb, data, tiles)
    eq, ed = {k: v.clone() for k, v in eq.items()}, ed["embedding"].clone()
    cp = pair.CapturedPair(modelq, modeldb, data, tiles)
    for _ in range(3):
        cp.replay()
    rq, rd = cp.finish()                                         # (raises if a replay saturated a map)
    for k in eq:
        assert torch.equal(rq[k], eq[k]), k
    assert torch.equal(rd["embedding"], ed)


def test_mode3_and_train_ignore_exponents(dev):
    """mfma_precision = 3 outputs and .train() outputs / gradients: bit-equal with and without exponents installed."""
    from agplace_amd import map_exponents as me
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    opt = Options(mfma_precision=3)
    data = to_dev(nets.synth_query(2, 64, 128, opt, seed=12), dev)

    def run(install):
        torch.manual_seed(21)
        model = randomize_bn(MM(opt=opt)).to(dev).eval()
        if install:
            me.set_exponents(model, {k: 3 for k in me.get_exponents(model)})
        with torch.no_grad():
            inf = {k: v.clone() for k, v in model(data, mode="q").items()}
        model.train()
        out = model(data, mode="q")
        out["embedding"].square().sum().backward()
        grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        return inf, {k: v.detach().clone() for k, v in out.items()}, grads
    inf0, tr0, g0 = run(False)
    inf1, tr1, g1 = run(True)
    assert all(torch.equal(inf0[k], inf1[k]) for k in inf0)
    assert all(torch.equal(tr0[k], tr1[k]) for k in tr0)
    assert set(g0) == set(g1) and len(g0) > 50 and all(torch.equal(g0[k], g1[k]) for k in g0)


# ------------------------------------------------------------------ 7. no new work per step
def _census(fn):
    """What one call of fn issues: the library entry points in order (each is a fixed launch sequence for given geometry) and the
    ATen operators dispatched (torch.profiler, CPU activity: no device tracing needed), metadata-only operators left out."""
    from agplace_amd import _lib
    lib = _lib.load()
    calls, saved = [], {}
    for name in _lib.SIGNATURES:
        f = getattr(lib, name)
        saved[name] = f

        def wrap(*a, _f=f, _n=name):
            calls.append(_n)
            return _f(*a)
        setattr(lib, name, wrap)
    try:
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
    finally:
        for name, f in saved.items():
            setattr(lib, name, f)
    aten = collections.Counter(e.name for e in prof.events() if e.name.startswith("aten::") and e.name not in _ATEN_METADATA)
    return calls, aten


# ATen operators that only make a new tensor OBJECT over existing memory (or return their argument): no allocation, no device
# work.  A `.to()` / `.contiguous()` that does copy dispatches aten::_to_copy / aten::clone / aten::copy_, which stay counted.
_ATEN_METADATA = {"aten::detach", "aten::to", "aten::contiguous", "aten::view", "aten::reshape", "aten::_unsafe_view", "aten::slice",
                  "aten::select", "aten::as_strided", "aten::permute", "aten::transpose", "aten::t", "aten::unsqueeze", "aten::squeeze",
                  "aten::expand", "aten::alias", "aten::set_", "aten::lift_fresh", "aten::unbind", "aten::is_pinned",
                  "aten::result_type"}


def test_exponents_add_no_launch_to_the_step(dev):
    """The paired forward (the bench step's shape of work) with exponents forced on every group issues the same library entry
    points in the same order, and the same ATen operators that allocate or launch, as without."""
    from agplace_amd import map_exponents as me
    from agplace_amd import pair
    modelq, modeldb, opt = _healthy_pair(dev)
    data = to_dev(nets.synth_query(4, 64, 192, opt, seed=5), dev)
    tiles = {"db_map": torch.randn(4, 1, 3, 64, 64, generator=torch.Generator().manual_seed(6)).to(dev)}

    def step():
        pair.embed_pair(modelq, modeldb, data, tiles)
    for _ in range(2):
        step()
    calls0, aten0 = _census(step)
    me.set_exponents(modelq, {k: 3 for k in me.get_exponents(modelq)})
    me.set_exponents(modeldb, {k: 2 for k in me.get_exponents(modeldb)})
    for _ in range(2):
        step()                                                   # (re-folds once: the prepared constants are cached again)
    calls1, aten1 = _census(step)
    print("MAPEXP census: entry-point calls per step", len(calls0), "aten ops", sum(aten0.values()))
    assert len(calls0) > 20 and ("agp_vecprog_run2" in calls0 or "agp_vecprog_run" in calls0)
    assert any(n.startswith("aten::empty") for n in aten0)              # (the census does see the forward's allocations)
    assert calls1 == calls0
    assert aten1 == aten0, {k: (aten0.get(k), aten1.get(k)) for k in set(aten0) | set(aten1) if aten0.get(k) != aten1.get(k)}
