"""The references of tests/sparse_kernel_ref.py against the project's oracle (oracle/sparse.py) on a small real cloud, in fp64 on
the CPU: the GPU tests of the sparse kernels (tests/test_gpu_sparse_kernels.py) stand on these functions."""
import numpy as np
import pytest
import torch

import sparse_kernel_ref as R
from oracle import sparse as osp

TOL = 1e-12


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.fixture(scope="module")
def cloud():
    """3 samples (the last one EMPTY: nbatch = 3, coordinates of samples 0 and 1 only), 8 channels."""
    coords, _ = osp.synth_cloud(2, 90, extent=9, seed=5)
    g = torch.Generator().manual_seed(11)
    x = osp.from_coords(torch.randn((coords.shape[0], 8), generator=g, dtype=torch.float64), coords, nbatch=3)
    return x


def _zero_row(x):
    return torch.cat([x.feats, torch.zeros((1, x.feats.shape[1]), dtype=x.feats.dtype)], 0)


def _table(x, out_coords, offs):
    n_in = len(x.coords)
    return np.array([[x.index.get((b, cx + dx, cy + dy, cz + dz), n_in) for b, cx, cy, cz in out_coords] for dx, dy, dz in offs],
                    dtype=np.int32)


def _seg_off(x):
    b = torch.tensor([c[0] for c in x.coords], dtype=torch.long)
    return torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(b, minlength=x.nbatch).cumsum(0)])


def test_gather_table_switches():
    tab = R.gather_table(27, 700, 500, 0.5, seed=1, centre=13, lacking={0: (0, 1, 26), 3: range(9)}, single=(2, 5), absent_rows=40)
    assert tab.dtype == np.int32 and tab.shape == (27, 700) and tab.min() >= 0 and tab.max() == 500
    assert (tab[[0, 1, 26], :128] == 500).all() and (tab[:9, 384:512] == 500).all()
    assert (tab[5, 256:384] != 500).sum() >= 100 and (np.delete(tab, 5, 0)[:, 256:384] == 500).all()
    dead = (tab == 500).all(0)
    assert dead[-1] and 40 <= dead.sum() <= 45
    live = ~dead & ~((np.arange(700) >= 256) & (np.arange(700) < 384))
    assert (tab[13, live] == np.minimum(np.arange(700), 500)[live]).all()
    m = R.granule_masks(tab, 500)
    assert m.shape == (6,) and int(m[0]) & 0b11 == 0 and int(m[0]) >> 26 == 0 and int(m[3]) & 0x1ff == 0 and int(m[2]) == 1 << 5
    one = R.one_hot_table(300, 40, seed=2)
    assert ((one != 40).sum(0) == 1).all()


@pytest.mark.parametrize("ksize,stride", [(3, 1), (2, 2)])
def test_conv_ref64_equals_the_oracle_convolution(cloud, ksize, stride):
    x = cloud
    g = torch.Generator().manual_seed(ksize)
    kernel = torch.randn((ksize ** 3, 8, 16), generator=g, dtype=torch.float64)
    want = osp.conv(x, kernel, ksize, stride)
    tab = _table(x, want.coords, osp._offsets(ksize, x.stride))
    assert tab.shape == (ksize ** 3, len(want.coords)) and (tab == len(x.coords)).any() and (tab != len(x.coords)).any()
    assert _rel(R.conv_ref64(_zero_row(x), tab, kernel), want.feats) < TOL
    # the epilogue: per-channel scale and shift, a residual on the output rows, ReLU
    scale, shift = torch.rand(16, generator=g, dtype=torch.float64) + 0.5, torch.randn(16, generator=g, dtype=torch.float64)
    res = torch.randn(want.feats.shape, generator=g, dtype=torch.float64)
    assert _rel(R.conv_ref64(_zero_row(x), tab, kernel, scale, shift, res, True), torch.relu(want.feats * scale + shift + res)) < TOL


def test_conv_ref64_on_the_one_hot_table_equals_the_oracle_transposed_convolution(cloud):
    fine = cloud
    g = torch.Generator().manual_seed(3)
    coarse = osp.conv(fine, torch.randn((8, 8, 8), generator=g, dtype=torch.float64), 2, 2)
    kernel = torch.randn((8, 8, 16), generator=g, dtype=torch.float64)
    want = osp.conv_transpose(coarse, kernel, fine)
    n_in, st = len(coarse.coords), fine.stride
    tab = np.full((8, len(fine.coords)), n_in, dtype=np.int32)
    for i, (b, cx, cy, cz) in enumerate(fine.coords):
        u = (b, cx // 2 // st * 2 * st, cy // 2 // st * 2 * st, cz // 2 // st * 2 * st)
        tab[(cx - u[1]) // st + 2 * ((cy - u[2]) // st) + 4 * ((cz - u[3]) // st), i] = coarse.index[u]
    assert ((tab != n_in).sum(0) == 1).all()
    assert _rel(R.conv_ref64(_zero_row(coarse), tab, kernel), want.feats) < TOL


def test_wgrad_ref64_equals_autograd_through_the_oracle_convolution(cloud):
    x = cloud
    g = torch.Generator().manual_seed(4)
    kernel = torch.randn((27, 8, 16), generator=g, dtype=torch.float64, requires_grad=True)
    out = osp.conv(x, kernel, 3)
    gout = torch.randn(out.feats.shape, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad((out.feats * gout).sum(), kernel)
    tab = _table(x, x.coords, osp._offsets(3, 1))
    assert _rel(R.wgrad_ref64(_zero_row(x), tab, gout), want) < TOL
    assert _rel(R.wgrad_f32(_zero_row(x), tab, gout), want) < 1e-5        # (the fp32 yardstick computes the same sum)


def test_emulate_rounds_operands_and_result_to_the_storage_formats(cloud):
    x = cloud
    g = torch.Generator().manual_seed(6)
    kernel = torch.randn((27, 8, 16), generator=g, dtype=torch.float64) / 10
    tab = _table(x, x.coords, osp._offsets(3, 1))
    ref = R.conv_ref64(_zero_row(x), tab, kernel)
    for prec, err in ((4, 2.0 ** -10), (2, 2.0 ** -10), (3, 2.0 ** -15)):
        e = R.emulate(prec, _zero_row(x), tab, kernel)
        assert 0 < _rel(e, ref) < err
        assert torch.equal(R.store_round(prec)(e), e)
        # operands that are already stored values: only the result's rounding is left
        xs, ws = R.store_round(prec)(_zero_row(x)), R.weight_round(prec)(kernel)
        assert torch.equal(R.weight_round(prec)(ws), ws)
        assert torch.equal(R.emulate(prec, xs, tab, ws), R.store_round(prec)(R.conv_ref64(xs, tab, ws)))


def test_segment_references_equal_the_oracle(cloud):
    x = cloud
    seg = _seg_off(x)
    assert seg.tolist()[-2:] == [len(x.coords)] * 2                          # the empty sample
    assert _rel(R.seg_mean64(x.feats, seg), osp.global_avg(x)) < TOL
    for p in (3.0, 2.5):
        assert _rel(R.seg_gem64(x.feats, seg, p), osp.mink_gem(x, torch.tensor(p, dtype=torch.float64))) < TOL
    assert not R.seg_mean64(x.feats, seg)[2].any() and not R.seg_gem64(x.feats, seg, 3.0)[2].any()
    for k in (3, 5):
        w = torch.randn((1, 1, k), generator=torch.Generator().manual_seed(k), dtype=torch.float64)
        s = R.eca64(R.seg_mean64(x.feats, seg), w)
        assert _rel(R.seg_affine64(x.feats, R.seg_bidx(seg), scale=s), osp.eca(x, w).feats) < TOL
    g = torch.Generator().manual_seed(8)
    add, res = torch.randn((3, 8), generator=g, dtype=torch.float64), torch.randn(x.feats.shape, generator=g, dtype=torch.float64)
    assert _rel(R.seg_affine64(x.feats, R.seg_bidx(seg), add=add, res=res, relu=True),
                torch.relu(osp.broadcast_add(x, add).feats + res)) < TOL
    b = R.seg_bidx(seg)
    want = torch.stack([(x.feats[b == i] * res[b == i]).sum(0) for i in range(3)])
    assert _rel(R.seg_dot64(x.feats, res, seg), want) < TOL
    assert _rel(R.seg_dot64(x.feats, None, seg), torch.stack([x.feats[b == i].sum(0) for i in range(3)])) < TOL


@pytest.mark.parametrize("p", [3.0, 2.5])
def test_pooling_backward_reference_equals_autograd(cloud, p):
    seg = _seg_off(cloud)
    g = torch.Generator().manual_seed(9)
    x = cloud.feats.clone()
    x[::5] = x[::5].abs() * 1e-7                                              # values below eps
    x.requires_grad_(True)
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    gmean, ggem = torch.randn((3, 8), generator=g, dtype=torch.float64), torch.randn((3, 8), generator=g, dtype=torch.float64)
    base = torch.randn(x.shape, generator=g, dtype=torch.float64)
    mean, gem = R.seg_mean64(x, seg), R.seg_gem64(x, seg, pt)
    gx, gp = torch.autograd.grad((mean * gmean).sum() + (gem * ggem).sum(), (x, pt))
    out, dp = R.seg_pool_bwd64(x.detach(), seg, gmean, ggem, gem.detach(), p, base=base)
    assert _rel(out - base, gx) < TOL and abs(float(dp - gp)) < TOL * max(1.0, abs(float(gp)))
    out, dp = R.seg_pool_bwd64(x.detach(), seg, gmean=gmean)
    (gx,) = torch.autograd.grad((R.seg_mean64(x, seg) * gmean).sum(), x)
    assert dp is None and _rel(out, gx) < TOL


@pytest.mark.parametrize("k", [3, 5])
def test_eca_backward_reference_equals_autograd(cloud, k):
    seg = _seg_off(cloud)
    g = torch.Generator().manual_seed(10 + k)
    x = cloud.feats.clone().requires_grad_(True)
    w = torch.randn(k, generator=g, dtype=torch.float64, requires_grad=True)
    gs = torch.randn((3, 8), generator=g, dtype=torch.float64)
    mean = R.seg_mean64(x, seg)
    s = R.eca64(mean, w)
    gx, gw = torch.autograd.grad((s * gs).sum(), (x, w))
    add, gw_ref = R.eca_bwd64(mean.detach(), s.detach(), gs, seg, w.detach())
    assert _rel(gw_ref, gw) < TOL and not add[2].any()
    assert _rel(add[R.seg_bidx(seg)], gx) < TOL                               # dL/dmean spread over the rows


def test_granule_rel_sees_what_the_whole_map_figure_averages_away():
    g = torch.Generator().manual_seed(1)
    ref = torch.randn((2100, 128), generator=g, dtype=torch.float64)
    got = ref.clone()
    got[1280:1408, 64:] += 0.01 * torch.randn((128, 64), generator=g, dtype=torch.float64)
    worst, where, rel = R.granule_rel(got, ref)
    assert where == "rows 1280..1407 columns 64..127" and rel.shape == (17, 2)
    assert 0.008 < worst < 0.012 and _rel(got, ref) < worst / 5
    assert int((rel > 0).sum()) == 1
    # the partial last block is averaged over its own 52 rows; a block of all-zero reference rows divides by the whole rms
    got = ref.clone()
    got[2048:] += 0.01
    ref0 = ref.clone()
    ref0[:128] = 0
    assert abs(R.granule_rel(got, ref)[0] - 0.01 / float(ref.pow(2).mean().sqrt())) < 1e-9
    assert R.granule_rel(ref0, ref0)[0] == 0.0
