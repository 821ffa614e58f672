"""csrc/fblock64.hip walks the IMAGE rows of the batch column (pairs of rows aligned to the images, the rows above and below an
image taken from one zero row in LDS) and cuts its segments in those pairs: the block is still bit-identical to two conv
launches, independent of the segmentation and of an image's place in the batch, stores interior pixels only, and the range guard
covers what it covered.  Shapes: h % 4 == 2 (an image ends on a half step), ragged and one-pixel strips, walks that cross image
borders, more images than rows per segment; two problems per launch (the query / database pair)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def _signed_scale(g):
    """Folded-BN scales of both signs, magnitudes 0.5 .. 1.5."""
    return (0.5 + torch.rand(64, generator=g)) * (1.0 - 2.0 * (torch.rand(64, generator=g) < 0.5).float())


def _problem(dev, g, n, h, w):
    from agplace_amd import ops
    x = torch.relu(torch.randn(n, 64, h, w, generator=g))
    ws = [torch.randn(64, 64, 3, 3, generator=g) / (64 * 9) ** 0.5 for _ in range(2)]
    sc = [_signed_scale(g) for _ in range(2)]
    sh = [0.3 * torch.randn(64, generator=g) for _ in range(2)]
    xm = ops.pack_f32(x.to(dev), 64, 1, 4)
    cws = [ops.ConvWeights(ws[i].to(dev), sc[i].to(dev), sh[i].to(dev), 1, 1) for i in range(2)]
    assert ops.bblock64_ok(xm, cws[0], cws[1], 4)
    x64 = xm.to_f32().double().cpu()                      # the fp16-rounded input is what both paths see
    t = F.conv2d(x64, ws[0].double(), None, 1, 1) * sc[0].double().view(1, -1, 1, 1) + sh[0].double().view(1, -1, 1, 1)
    ref = F.conv2d(torch.relu(t), ws[1].double(), None, 1, 1) * sc[1].double().view(1, -1, 1, 1) + sh[1].double().view(1, -1, 1, 1)
    return xm, cws, torch.relu(ref + x64)


def _unfused(dev, xm, cws):
    from agplace_amd import ops
    mid = ops.SplitMap.alloc(xm.n, xm.h, xm.w, 64, 1, 4, dev)
    out = ops.SplitMap.alloc(xm.n, xm.h, xm.w, 64, 1, 4, dev)
    ops.conv2d(xm, cws[0], mid, relu=True, prec=4)
    ops.conv2d(mid, cws[1], out, residual=xm, relu=True, prec=4)
    return out


def _sentinel_out(dev, n, h, w):
    from agplace_amd import ops
    out = ops.SplitMap.alloc(n, h, w, 64, 1, 4, dev)
    out.hi.fill_(SENTINEL)
    return out


def _halo_is_sentinel(o):
    return all(bool((t == SENTINEL).all()) for t in (o.hi[:, 0], o.hi[:, -1], o.hi[:, :, 0], o.hi[:, :, -1]))


# (the last group: 16 pairs in 2 segments each, the cut at pair 8 is the first pair of an image -- a segment that starts with an
# image, not with the batch, and so has no seam pair in front of it)
@pytest.mark.parametrize("shapes", [[(3, 6, 30), (5, 8, 28)], [(2, 14, 57), (9, 4, 56)], [(8, 4, 56), (4, 8, 30)]])
def test_walk_over_image_rows_is_bit_identical_to_two_convs(dev, shapes):
    """The 32x32x16 form against conv2d + conv2d bit for bit, the production form against the fp64 block at the bound
    tests/test_gpu_kernels.py holds this kernel to (8e-4); the output buffers go in filled with a sentinel, halo included: every
    interior element is overwritten and no halo element is."""
    from agplace_amd import ops
    g = torch.Generator().manual_seed(shapes[0][1] * 1000 + shapes[0][2])
    probs = [_problem(dev, g, *s) for s in shapes]
    want = [_unfused(dev, xm, cws) for xm, cws, _ in probs]
    for exact in (True, False):
        outs = ops.bblock64_grouped([(xm, cws[0], cws[1], _sentinel_out(dev, xm.n, xm.h, xm.w)) for xm, cws, _ in probs], exact=exact)
        torch.cuda.synchronize()
        for s, o, wnt, (_, _, ref) in zip(shapes, outs, want, probs):
            assert _halo_is_sentinel(o), (s, exact)
            inner = o.hi[:, 1:-1, 1:-1]
            if exact:
                assert torch.equal(inner, wnt.hi[:, 1:-1, 1:-1]), s
            err = rel_l2(inner.float().permute(0, 3, 1, 2), ref)
            print("fblock64 walk", s, "exact" if exact else "production", "rel_l2 vs fp64 = %.3e" % err)
            assert err < 8e-4, (s, exact, err)


def _launcher_segs(shapes, cus):
    """The segments per strip agp_bblock64_fwd_grouped gives every problem (n, h, w) of one launch on `cus` CUs: the rule of
    csrc/fblock64.hip restated, so that the test below can choose its shapes for the device it runs on and state what it compares."""
    np_ = [n * h // 2 for n, h, w in shapes]
    st = [(w + 27) // 28 for n, h, w in shapes]
    total = sum(a * b for a, b in zip(np_, st))
    smax = [max(p // 8, 1) for p in np_]
    segs = [min(max(p * cus // total, 1), m) for p, m in zip(np_, smax)]
    rem = cus - sum(a * b for a, b in zip(segs, st))
    while True:
        best = -1
        for i in range(len(shapes)):
            if segs[i] >= smax[i] or st[i] > rem:
                continue
            if best < 0:
                best = i
                continue
            li, lb = np_[i] * segs[best], np_[best] * segs[i]
            if li > lb or (li == lb and st[i] * np_[i] > st[best] * np_[best]):
                best = i
        if best < 0:
            return segs
        segs[best] += 1
        rem -= st[best]


def test_outputs_and_pooled_means_do_not_depend_on_the_segmentation(dev):
    """The same three images cut three ways: alone (4 segments per strip: cuts at pairs 8, 16, 24 of 33, inside the images, the
    walks cross the image borders at 11 and 22), as ONE segment per strip, and as the head of a four-image batch (5 segments: cuts
    at 8, 17, 26, 35).  The release library has no switch, so the launcher's own rule makes the single segment: beside a
    one-strip companion with enough rows the problem's share of the CUs rounds down to one and the companion takes every CU that
    is left; the companion's size is chosen by the rule restated above for the CU count of the device, and the test asserts the
    segment counts it compares.  Outputs and pooled means must be the same bits."""
    from agplace_amd import ops
    g = torch.Generator().manual_seed(5)
    n, h, w = 3, 22, 30
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    xm4, cws, _ = _problem(dev, g, n + 1, h, w)
    xm = ops.SplitMap(xm4.hi[:n].contiguous(), None, n, h, w, 64, 1)
    assert _launcher_segs([(n, h, w)], cus) == [4] and _launcher_segs([(n + 1, h, w)], cus) == [5]
    comp = next((c for c in ((nc, 56, 28) for nc in range(100, 1200, 20)) if _launcher_segs([(n, h, w), c], cus)[0] == 1), None)
    assert comp is not None, "no companion makes one segment on %d CUs" % cus
    big = ops.pack_f32(torch.rand(comp[0], 64, comp[1], comp[2], device=dev), 64, 1, 4)

    def run(xmap, with_companion, exact):
        req = ops.PoolReq(want_mean=True, want_gem=False)
        jobs = [(xmap, cws[0], cws[1], ops.SplitMap.alloc(xmap.n, h, w, 64, 1, 4, dev), req)]
        if with_companion:
            jobs.append((big, cws[0], cws[1], ops.SplitMap.alloc(big.n, big.h, big.w, 64, 1, 4, dev)))
        out = ops.bblock64_grouped(jobs, exact=exact)[0]
        torch.cuda.synchronize()
        return out.hi.clone(), req.mean.clone()
    for exact in (True, False):
        o_four, m_four = run(xm, False, exact)
        o_one, m_one = run(xm, True, exact)
        o_five, m_five = run(xm4, False, exact)
        assert torch.equal(o_four, o_one) and torch.equal(m_four, m_one), exact
        assert torch.equal(o_four, o_five[:n]) and torch.equal(m_four, m_five[:n]), exact
    want = _unfused(dev, xm, cws)
    assert torch.equal(run(xm, True, True)[0], want.hi)


def test_pooled_mean_of_an_image_first_or_last_in_the_batch(dev):
    """Image i's pooled mean is the same bits whether the image is the first or the last of the batch, and within the bound of
    tests/test_gpu_kernels.py (1e-6) of the fp64 mean of the stored output.  h % 4 == 2, three strips."""
    from agplace_amd import ops
    g = torch.Generator().manual_seed(17)
    n, h, w = 5, 6, 57
    xm, cws, _ = _problem(dev, g, n, h, w)

    def run(xmap):
        req = ops.PoolReq(want_mean=True, want_gem=False)
        out = ops.SplitMap.alloc(xmap.n, h, w, 64, 1, 4, dev)
        ops.bblock64_grouped([(xmap, cws[0], cws[1], out, req)])
        torch.cuda.synchronize()
        return out, req.mean
    out, mean = run(xm)
    err = rel_l2(mean, out.to_f32().double().mean((2, 3)))
    print("fblock64 walk pooled mean rel_l2 vs fp64 = %.3e" % err)
    assert err < 1e-6
    perm = torch.tensor([4, 1, 2, 3, 0], device=dev)
    out_p, mean_p = run(ops.SplitMap(xm.hi[perm].contiguous(), None, n, h, w, 64, 1))
    assert torch.equal(out_p.hi, out.hi[perm]) and torch.equal(mean_p, mean[perm])
    out_1, mean_1 = run(ops.SplitMap(xm.hi[4:5].contiguous(), None, 1, h, w, 64, 1))
    assert torch.equal(out_1.hi, out.hi[4:5]) and torch.equal(mean_1, mean[4:5])


@pytest.mark.parametrize("exact", [True, False])
def test_range_guard_counts_interior_intermediate_values_only(dev, exact):
    """conv1 with its left tap only (intermediate[y][x] = s1 * mean_c in[y][x - 1] + t1): ONE large input value makes ONE
    intermediate position saturate -- reported where that position is inside the image (here in the last row of image 0, the
    pair that reads the zero row below it), not reported where it is the padding column right of the image (a dead column of
    the ragged second strip: stored as zero, read by no stored output).  The block's output stays in range either way."""
    from agplace_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(23)
    n, h, w = 2, 6, 30
    x = torch.relu(torch.randn(n, 64, h, w, generator=g))
    w1 = torch.zeros(64, 64, 3, 3)
    w1[:, :, 1, 0] = 1.0 / 64
    w2 = torch.randn(64, 64, 3, 3, generator=g) / (64 * 9) ** 0.5
    cws = [ops.ConvWeights(w1.to(dev), torch.full((64,), 200.0, device=dev), torch.zeros(64, device=dev), 1, 1),
           ops.ConvWeights(w2.to(dev), torch.full((64,), 1e-6, device=dev), torch.zeros(64, device=dev), 1, 1)]

    def run(plant_col):
        xm = ops.pack_f32(x.to(dev), 64, 1, 4)
        if plant_col is not None:
            xm.hi[0, h, 1 + plant_col, 9] = 30000.0            # padded coordinates: image 0, its last row
        out = ops.SplitMap.alloc(n, h, w, 64, 1, 4, dev)
        word = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        prev = lib.agp_range_flag_set(word.data_ptr())
        try:
            ops.bblock64_grouped([(xm, cws[0], cws[1], out)], exact=exact)
        finally:
            lib.agp_range_flag_set(prev)
        torch.cuda.synchronize()
        assert float(out.hi.float().abs().max()) < 4e4         # the block's OUTPUT is in range
        return int(word.item())
    assert run(None) == 0
    assert run(5) == 1                                         # intermediate column 6: interior
    assert run(w - 1) == 0                                     # intermediate column w: conv2's padding
