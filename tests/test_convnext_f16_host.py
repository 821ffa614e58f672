"""Precision 4 of the ConvNeXt-tiny trunk, host side (no GPU): the fp64 emulation (tests/convnext_f16_ref.py), the option and the
prepared weight planes."""
import types

import pytest
import torch

import convnext_f16_ref as H
import convnext_ref as R
from agplace_amd import convnext as cnx
from agplace_amd.options import Options, from_reference_opt

SEED = 2


@pytest.fixture(scope="module")
def trunk_and_truth():
    m64 = R.seeded_trunk([2, 2, 2], SEED)
    x = R.seeded_input((2, 3, 64, 96), SEED, torch.float64)
    with torch.no_grad():
        return m64, x, R.forward_maps(m64, x)


def test_helper_without_rounding_is_the_restatement(trunk_and_truth):
    m64, x, want = trunk_and_truth
    got = H.forward_maps(m64, x, rnd=None)
    assert len(got) == 3
    for g, w in zip(got, want):
        assert g.dtype == torch.float64 and R.rel_l2(g, w) <= 1e-12 and R.rel_max(g, w) <= 1e-12


def test_fp16_rounding_alone_stays_inside_the_cap(trunk_and_truth):
    """The emulation's own error against the truth: between 1e-4 (the roundings are felt) and 1e-3 (the cap of the GPU tests).
    First measured at 2.5e-4 / 4.5e-4 / 5.8e-4."""
    m64, x, want = trunk_and_truth
    errs = [R.rel_l2(g, w) for g, w in zip(H.forward_maps(m64, x, rnd=H.round_f16), want)]
    print("fp16 emulation, 2_2_2 [2,3,64,96] seed 2: rel_l2 " + " / ".join(f"{e:.3g}" for e in errs))
    assert all(1e-4 <= e <= 1e-3 for e in errs), errs


def test_round_f16_is_nearest_even_saturating_and_keeps_nan():
    t = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65519.0, 1e9, -1e9, float("nan"), 2.0 ** -25, 0.1], dtype=torch.float64)
    got = H.round_f16(t)
    assert got[:5].tolist() == [1.0, 1.0 + 2.0 ** -9, 65504.0, 65504.0, -65504.0]      # ties to even; saturation
    assert bool(torch.isnan(got[5])) and float(got[6]) == 0.0 and float(got[7]) == float(torch.tensor(0.1).half())


def test_option():
    assert Options().convnext_precision == 3 and Options(convnext_precision=4).convnext_precision == 4
    for bad in (5, True, "4", 2, 4.0, None):
        with pytest.raises(ValueError, match="convnext_precision"):
            Options(convnext_precision=bad)
    assert from_reference_opt(types.SimpleNamespace(convnext_precision=4)).convnext_precision == 3
    assert Options(convnext_precision=4).copy().convnext_precision == 4


def test_set_precision_and_model_wiring():
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.network_mm.image_fe import ImageFE
    from agplace_amd.network_mm.mm import MM
    fe = cnx.ConvNeXt([1, 1, 1])
    assert fe.precision == 3 and fe.set_precision(4) is fe and fe.precision == 4 and fe.set_precision(3).precision == 3
    for bad in (5, True, "4", None):
        with pytest.raises(ValueError, match="set_precision"):
            fe.set_precision(bad)
    assert ImageFE("convnext_tiny", "1_1_1").fe.precision == 3
    assert ImageFE("convnext_tiny", "1_1_1", opt=Options(convnext_precision=4)).fe.precision == 4
    db = dict(dbimage_fe="convnext_tiny", dbimage_fe_layers="1_1_1", maptype="a_b")
    assert [e.fe.precision for e in DBVanilla2D("db", 256, opt=Options(convnext_precision=4, **db)).dbimage_fes] == [4, 4]
    assert [e.fe.precision for e in DBVanilla2D("db", 256, opt=Options(**db)).dbimage_fes] == [3, 3]
    mm = dict(mm_imgfe="convnext_tiny", mm_imgfe_layers="1_1_1", mm_imgfe_planes="96_192_384", mm_imgfe_dim=384, mm_stg2fuse_dim=384,
              mm_voxfe_planes="64_128_384", mm_voxfe_dim=384, mm_bevfe_planes="64_128_384", mm_bevfe_dim=384)
    assert MM(opt=Options(convnext_precision=4, **mm)).image_fe.fe.precision == 4
    assert MM(opt=Options(**mm)).image_fe.fe.precision == 3
    # precision 4 with the fp16 range guard: refused by name, by both models and by the op-level drop-in
    for build in (lambda o: DBVanilla2D("db", 256, opt=o.copy(**db)), lambda o: MM(opt=o.copy(**mm))):
        with pytest.raises(NotImplementedError, match="fp16_range_guard"):
            build(Options(convnext_precision=4, fp16_range_guard=True))
    guarded = ImageFE("convnext_tiny", "1_1_1", opt=Options(convnext_precision=4, fp16_range_guard=True)).eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="fp16_range_guard"):
        guarded(torch.zeros(1, 3, 32, 32))


def test_prepared_planes_are_the_fp16_rounding_of_the_mode3_fragments():
    """Element for element: the precision-4 plane is fp16(the fragment-ordered fp32 tensor that precision 3 splits into hi + lo),
    in the same order; everything that is not an MFMA operand is the same tensor in both."""
    m32 = R.seeded_trunk([1, 1, 1], SEED, torch.float32)
    for stage in (1, 3):
        blk, ds = m32.features[stage][0], m32.features[stage + 1]
        c = blk.layer_scale.shape[0]
        with torch.no_grad():
            p3, p4 = cnx.prep_block(blk), cnx.prep_block(blk, prec=4)
            d3, d4 = cnx.prep_down(*ds), cnx.prep_down(*ds, prec=4)
            frags = [(p3["w1"], p4["w1"], cnx._frag_rows(blk.block[3].weight.detach())),
                     (p3["w2"], p4["w2"], cnx._frag_acc(blk.block[5].weight.detach())),
                     (d3["w"], d4["w"], cnx._frag_rows(ds[1].weight.detach().permute(0, 2, 3, 1).reshape(2 * c, 4 * c)))]
        for planes3, planes4, frag in frags:
            assert len(planes3) == 2 and len(planes4) == 1
            hi, lo = planes3
            assert torch.equal(hi, frag.bfloat16()) and torch.equal(lo, (frag - hi.float()).bfloat16())     # the tensor 3 splits
            h = planes4[0]
            assert h.dtype == torch.float16 and h.shape == frag.shape and h.is_contiguous()
            assert torch.equal(h.double(), H.round_f16(frag))
        for k in ("dw", "dwb", "g", "b", "b1", "b2", "ls"):
            assert torch.equal(p3[k], p4[k])
    with pytest.raises(ValueError, match="precision"):
        cnx.prep_block(m32.features[1][0], prec=2)


def test_planes_saturate():
    w = torch.tensor([[1e6, -1e6, 65519.0, 1.0]])
    assert cnx._half(w).tolist() == [[65504.0, -65504.0, 65504.0, 1.0]]


def test_f16_entries_refuse_bad_arguments():
    """The precision-4 entries validate as the precision-3 ones do, before any launch: every call below has exactly one bad argument
    and must come back AGP_E_BADARG (= 1).  The pointers are never dereferenced."""
    from agplace_amd import _lib
    L = _lib.load()
    A, P, C = 4096, 40, 96                             # a 16-byte aligned stand-in address; 40 pixels pad to 64
    plane = 64 * C * 2                                 # one fp16 plane [P_pad][C]
    dw = dict(x=A, n=1, h=5, w=8, C=C, wt=A, bias=A, g=A, b=A, eps=1e-6, ws=A, nbytes=plane, stream=None)
    mlp = dict(ws=A, nbytes=plane, P=P, C=C, w1=A, b1=A, w2=A, b2=A, ls=A, resid=A, out=A, stream=None)
    ds = dict(x=A, n=1, h=5, w=8, C=C, g=A, b=A, eps=1e-6, wt=A, bias=A, out=A, stream=None)
    cases = [(L.agp_cnx_dwconv_ln_f16_fwd, dw, [("x", None), ("wt", None), ("bias", None), ("g", None), ("b", None), ("ws", None),
                                                 ("C", 100), ("n", 0), ("h", 0), ("w", 1 << 30), ("ws", A + 8), ("nbytes", plane - 1)]),
             (L.agp_cnx_mlp_f16_fwd, mlp, [("ws", None), ("w1", None), ("b1", None), ("w2", None), ("b2", None), ("ls", None),
                                           ("resid", None), ("out", None), ("C", 100), ("P", 0), ("P", (1 << 31) // 32),
                                           ("ws", A + 8), ("nbytes", plane - 1)]),
             (L.agp_cnx_downsample_f16_fwd, ds, [("x", None), ("g", None), ("b", None), ("wt", None), ("bias", None), ("out", None),
                                                 ("C", 100), ("n", 0), ("h", 1), ("w", 1)])]
    for fn, good, bads in cases:
        for key, value in bads:
            assert fn(*dict(good, **{key: value}).values()) == 1, (fn.__name__, key, value)
