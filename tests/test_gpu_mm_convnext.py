"""-m gpu tests of MM with mm_imgfe='convnext_tiny' (inference) against the fp64 reference of tests/mm_convnext_ref.py.

Set-up: layers 1_1_1 (2_1_2 once), image [2, 3, 64, 96] (maps 16x24, 8x12, 4x6), seeded weights drawn in fp32 so that the model
and the fp64 reference hold the same values.  With the dense voxel stand-ins the whole model is mode-3 or fp32 arithmetic and
is held to the project's mode-3 bar (tests/test_gpu_convnext.py): rel_l2 < 1e-4 and rel_max < 1e-4 on all seven outputs; so is
the voxel branch from `coords` at Options(mfma_precision=3).  At the default mfma_precision=4 the voxel branch is one-product
fp16 and the outputs meet the north-star bound 1e-3, as in the ResNet model's tests.
"""
import functools

import pytest
import torch

import mm_convnext_ref as ref
from oracle import nets
from gpu_util import rel_l2, rel_max, to_dev

pytestmark = pytest.mark.gpu

B, H, W = 2, 64, 96
KEYS = ("imagevec_org", "voxvec_org", "shallowvec_org", "stg2fusevec", "stg2imagevec", "stg2voxvec", "embedding")
TWO_TERMS = ["imageorg", "stg2image"]           # catadd adds the last term to the concatenation of the others


@functools.lru_cache(maxsize=None)
def _seeded(layers):
    """(fp32 state dict, the same values in fp64, fp64 trunk), shared by the tests and never modified."""
    p32, trunk = ref.seeded_params(ref.options(layers), seed=5, dtype=torch.float32)
    p64 = {k: (v.double() if v.is_floating_point() else v) for k, v in p32.items()}
    return p32, p64, trunk.double()


@functools.lru_cache(maxsize=None)
def _maps(layers, drop_image=False):
    """The fp64 trunk's maps of the test image: computed once per block-count string."""
    from convnext_ref import forward_maps
    img = _data()["query_image"].double()
    with torch.no_grad():
        return tuple(forward_maps(_seeded(layers)[2], img * 0 if drop_image else img))


@functools.lru_cache(maxsize=None)
def _data():
    return nets.synth_query(B, H, W, ref.options(), seed=9)


def _cloud(seed, n=200, extent=12):
    g = torch.Generator().manual_seed(seed)
    rows = []
    for b in range(B):
        xyz = torch.unique(torch.randint(0, extent, (n, 3), generator=g), dim=0)
        rows.append(torch.cat([torch.full((xyz.shape[0], 1), b), xyz], 1))
    c = torch.cat(rows, 0).float()
    return c, torch.ones(c.shape[0], 1)


def _model(dev, opt, layers="1_1_1", state=None):
    from agplace_amd.network_mm.mm import MM
    m = MM(opt=opt)
    m.load_state_dict(state if state is not None else _seeded(layers)[0], strict=True)     # the checkpoint round trip
    return m.to(dev).eval()


def _check(out, want, bound, what):
    for k in KEYS:
        e2, em = rel_l2(out[k], want[k]), rel_max(out[k], want[k])
        print(f"mm_convnext {what} {k}: rel_l2 {e2:.3e} rel_max {em:.3e}")
    for k in KEYS:
        assert out[k].shape == want[k].shape and out[k].dtype == torch.float32, (what, k)
        assert rel_l2(out[k], want[k]) < bound and rel_max(out[k], want[k]) < bound, (what, k, rel_l2(out[k], want[k]), rel_max(out[k], want[k]))


@pytest.mark.parametrize("l2", [True, False])
@pytest.mark.parametrize("fuse", ["add", "cat", "catadd"])
def test_dense_stand_ins_match_fp64(dev, fuse, l2):
    opt = ref.options(final_fusetype=fuse, output_l2=l2, **(dict(final_type=TWO_TERMS) if fuse == "catadd" else {}))
    m = _model(dev, opt)
    with torch.no_grad():
        out = m(to_dev(_data(), dev), mode="q")
    want = ref.forward_q(ref.cast(_data(), torch.float64), _seeded("1_1_1")[1], opt, maps=list(_maps("1_1_1")))
    assert out["embedding"].shape == (B, {"add": 384, "cat": len(opt.final_type) * 384, "catadd": 384}[fuse])
    _check(out, want, 1e-4, f"dense {fuse} l2={l2}")


def test_dense_stand_ins_match_fp64_with_more_blocks(dev):
    opt = ref.options("2_1_2")
    m = _model(dev, opt, "2_1_2")
    with torch.no_grad():
        out = m(to_dev(_data(), dev), mode="q")
    want = ref.forward_q(ref.cast(_data(), torch.float64), _seeded("2_1_2")[1], opt, maps=list(_maps("2_1_2")))
    _check(out, want, 1e-4, "dense 2_1_2")


def _cloud_data(seed):
    d = {"query_image": _data()["query_image"]}
    d["coords"], d["features"] = _cloud(seed)
    return d


@functools.lru_cache(maxsize=None)
def _cloud_ref(seed, drop=None):
    opt = ref.options()
    return ref.forward_q(ref.cast(_cloud_data(seed), torch.float64), _seeded("1_1_1")[1], opt,
                         maps=list(_maps("1_1_1", drop == "image")), drop=drop)


def test_voxel_branch_from_coords_matches_fp64_in_mode_3(dev):
    opt = ref.options(mfma_precision=3)
    m = _model(dev, opt)
    with torch.no_grad():
        out = m(to_dev(_cloud_data(21), dev), mode="q")
        other = m(to_dev(_cloud_data(22), dev), mode="q")
    assert m.voxel_coords_in_range()
    _check(out, _cloud_ref(21), 1e-4, "coords prec 3")
    for k in ("stg2voxvec", "voxvec_org"):              # the branch is live: non-trivial, and it follows the cloud
        assert float(out[k].norm()) > 0 and rel_l2(other[k], out[k]) > 1e-3, k


def test_voxel_branch_from_coords_at_the_default_precision(dev):
    opt = ref.options()
    assert opt.mfma_precision == 4
    m = _model(dev, opt)
    with torch.no_grad():
        out = m(to_dev(_cloud_data(21), dev), mode="q")
    want = _cloud_ref(21)
    for k in KEYS:
        print(f"mm_convnext coords prec 4 {k}: rel_l2 {rel_l2(out[k], want[k]):.3e}")
    for k in KEYS:
        assert rel_l2(out[k], want[k]) < 1e-3, (k, rel_l2(out[k], want[k]))


@pytest.mark.parametrize("key", ["stg2fuseblock.ffnsimg.0.conv2.weight", "fuseblocktoshallow.blocks.1.blocks.0.func.func.fc.weight"])
def test_weights_are_felt(dev, key):
    """A silently skipped branch would leave the embedding unchanged when its weights are zeroed."""
    opt = ref.options()
    data = to_dev(_data(), dev)
    state = dict(_seeded("1_1_1")[0])
    state[key] = torch.zeros_like(state[key])
    with torch.no_grad():
        base = _model(dev, opt)(data, mode="q")["embedding"]
        zeroed = _model(dev, opt, state=state)(data, mode="q")["embedding"]
    assert rel_l2(zeroed, base) > 1e-3, key


def test_drop_image_and_drop_pc(dev):
    from agplace_amd.network_mm.mm import MM
    opt = ref.options(mfma_precision=3)
    for drop in ("image", "pc"):
        m = MM(drop=drop, opt=opt)
        m.load_state_dict(_seeded("1_1_1")[0], strict=True)
        m = m.to(dev).eval()
        with torch.no_grad():
            out = m(to_dev(_cloud_data(21), dev), mode="q")
        _check(out, _cloud_ref(21, drop), 1e-4, f"drop={drop}")


def test_captured_forward_replays_bit_equal(dev):
    opt = ref.options()
    m = _model(dev, opt)
    data = to_dev(_data(), dev)
    with torch.no_grad():
        eager = {k: v.clone() for k, v in m(data, mode="q").items()}    # the warm-up: weights prepared, workspaces allocated
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m(data, mode="q")
        inputs = {t.data_ptr() for v in data.values() for t in (v if isinstance(v, list) else [v])}
        for v in out.values():
            if v.data_ptr() not in inputs:      # (with the dense stand-ins stg2voxvec IS the input tensor)
                v.zero_()
        graph.replay()
        torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(out[k], eager[k]), k


def test_refusals_name_their_case(dev):
    from agplace_amd import map_exponents, pair
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.options import Options
    opt = ref.options(query_substreams=2)
    m = _model(dev, opt)
    data = to_dev(_data(), dev)
    with pytest.raises(NotImplementedError, match="gradient"):
        m(data, mode="q")
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="train"):
            m.train()(data, mode="q")
        m.eval()
        u8 = torch.zeros(B, 1, H, W, 3, dtype=torch.uint8, device=dev)
        with pytest.raises(NotImplementedError, match="uint8"):
            m(dict(data, query_image=u8), mode="q")
        with pytest.raises(NotImplementedError, match="query_frames"):
            m({k: v for k, v in dict(data, query_frames=u8).items() if k != "query_image"}, mode="q")
        db = DBVanilla2D("db", 384, opt=Options(features_dim=384)).to(dev).eval()
        with pytest.raises(NotImplementedError, match="embed_pair"):
            pair.embed_pair(m, db, data, {"db_map": torch.zeros(B, 1, 3, 64, 64, device=dev)})
        with pytest.raises(NotImplementedError, match="calibrate"):
            map_exponents.calibrate(m, [data])
        # query_substreams = 2 with a batch it would split: the forward runs whole, and equals the plain model's
        four = {k: ([torch.cat([t, t]) for t in v] if isinstance(v, list) else torch.cat([v, v])) for k, v in data.items()}
        out = m(four, mode="q")
        want = _model(dev, ref.options())(four, mode="q")
        assert out["embedding"].shape == (2 * B, 384) and torch.equal(out["embedding"], want["embedding"])
