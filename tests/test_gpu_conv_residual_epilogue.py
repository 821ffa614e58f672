"""-m gpu: igemm_kxrw's epilogue -- the residual through LDS-DMA into the wave's swizzled strip, the pooled sweep -- against an fp64
conv of the fp16-rounded operands, in each tile schedule (full tiles only, half tiles only, a mixed grouped launch), with and
without a residual, and with pooling off, GeM p = 3, GeM p = 2.5 and the sum-of-squares statistic.

All problems are 128 -> 128 channels: K = 1152 gives 12 macro-steps, so the last one (which carries tile row 0's residual pieces)
is distinct from the first.  Shapes, each asserted through ops.conv_tile_plan:
  full  : 62 images of 17 x 30 -- the launcher runs a launch of <= 128 tiles as half tiles, so "full tiles only" needs more
          than 128 row tiles: 62 x 17 x 32 = 33728 raster rows = 131.75 tiles (pooled: 62 x 576 rows = 139.5 tiles); M is no
          multiple of 256, every image has halo columns, and the pooled raster has rows past the image
  half  : the first 3 of those images (6.4 tiles -> 13 half tiles, the last one partial)
  mixed : conv_sched_util.GROUPS["boundary_exactly_at_MT_full"], two problems of different sizes in one grouped launch

The residual lies inside a larger NaN-filled buffer and its halo is NaN as well: a residual piece fetched from a wrong address, or
a not-stored pixel that is not zeroed, puts a NaN into the map or into the pooled sums.
Bars: conv_sched_util.BARS[4] = 6e-4 on the whole map and the worst 64 x 128 block, 1e-6 for pooled values against fp64 pooling of
the stored map (tests/test_gpu_conv_schedules.py's, same precision mode)."""
import pytest
import torch

from conv_sched_util import BARS, GROUPS, GUARD, GUARD_BITS, _f16, images, ref64, regime, weights, worst_block
from gpu_util import rel_l2

pytestmark = pytest.mark.gpu

SHAPES = {"full": [(62, 17, 30)], "half": [(3, 17, 30)], "mixed": GROUPS["boundary_exactly_at_MT_full"]}
WANT = {"full": "full-only", "half": "all-half", "mixed": "mixed"}
POOLS = ["none", "gem3", "gem2.5", "sq"]
NAN16 = GUARD_BITS            # an fp16 NaN


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


_REF = {}


def _problem(i, n, h, w):
    """Problem i of a launch, on the CPU: operands, and the fp64 conv of the fp16-rounded operands WITHOUT residual and ReLU
    (the cases add them); computed once.  "half" is the head of "full"."""
    key = (i, h, w)
    if key not in _REF or _REF[key]["x"].shape[0] < n:
        nmax = max(s[i][0] for s in SHAPES.values() if len(s) > i and s[i][1:] == (h, w))
        x, res = images(128, h, w, nmax, 11 + i), images(128, h, w, nmax, 61 + i)
        wt, scale, shift = weights(128, 128, 5 + i)
        _REF[key] = dict(x=x, res=res, wt=wt, scale=scale, shift=shift, y=ref64(_f16(x), _f16(wt), scale, shift, None, False))
    q = _REF[key]
    return dict(q, x=q["x"][:n], res=q["res"][:n], y=q["y"][:n])


def _nan_guarded_residual(res, dev):
    """The packed fp16 residual in the middle of a NaN-filled buffer, its halo NaN too."""
    from agplace_amd import ops
    n, c, h, w = res.shape
    packed = ops.pack_f32(res.to(dev), c, 1, 4)
    numel = n * (h + 2) * (w + 2) * c
    buf = torch.full((GUARD + numel + GUARD,), NAN16, dtype=torch.int16, device=dev)
    m = buf[GUARD:GUARD + numel].view(n, h + 2, w + 2, c)
    m[:, 1:-1, 1:-1] = packed.hi.view(torch.int16)[:, 1:-1, 1:-1]
    return ops.SplitMap(m.view(torch.float16), None, n, h, w, c, 1), buf


def _request(pool, dev):
    from agplace_amd import ops
    if pool == "none":
        return None
    if pool == "sq":
        return ops.SqStatReq()
    return ops.PoolReq(torch.tensor([float(pool[3:])], device=dev), want_mean=True, want_gem=True)


def _check_pooled(req, pool, stored, what):
    """The request's values against fp64 pooling of the STORED map [n, c, h, w]."""
    assert req.fused, what
    d = stored.double()
    if pool == "sq":
        n, c = d.shape[:2]
        part = req.partial.view(-1, 2, c)[:req.blocks].double().cpu().view(n, req.blocks // n, 2, c).sum(1)
        e0, e1 = rel_l2(part[:, 0], d.sum((2, 3))), rel_l2(part[:, 1], (d * d).sum((2, 3)))
        print("%s: sum %.3g squares %.3g (bar 1e-6)" % (what, e0, e1))
        assert e0 < 1e-6 and e1 < 1e-6, (what, e0, e1)
    else:
        pw = float(pool[3:])
        e0 = rel_l2(req.mean.cpu(), d.mean((2, 3)))
        e1 = rel_l2(req.gem.cpu(), d.clamp(min=1e-6).pow(pw).mean((2, 3)).pow(1 / pw))
        print("%s: mean %.3g gem %.3g (bar 1e-6)" % (what, e0, e1))
        assert e0 < 1e-6 and e1 < 1e-6, (what, e0, e1)


@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("use_res", [True, False], ids=["res", "plain"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_residual_and_pooling_epilogue(dev, shape, use_res, pool):
    from agplace_amd import ops
    probs = [_problem(i, *s) for i, s in enumerate(SHAPES[shape])]
    jobs, outs, rbufs, reqs = [], [], [], []
    for q, (n, h, w) in zip(probs, SHAPES[shape]):
        xm = ops.pack_f32(q["x"].to(dev), 128, 1, 4)
        cw = ops.ConvWeights(q["wt"].to(dev), q["scale"].to(dev), q["shift"].to(dev), 1, 1)
        out = ops.SplitMap.alloc(n, h, w, 128, 1, 4, dev)
        rm, rbuf = _nan_guarded_residual(q["res"], dev) if use_res else (None, None)
        req = _request(pool, dev)
        jobs.append((xm, cw, out, rm, True) + (() if req is None else (req,)))
        outs.append(out); rbufs.append(rbuf); reqs.append(req)
    p = ops.conv_tile_plan(jobs, 4)
    assert p["kernel"] == "kxrw" and regime(p) == WANT[shape], p
    if shape == "full":
        assert SHAPES["full"][0][0] * 17 * 32 % 256 != 0
    if len(jobs) == 1:
        ops.conv2d(jobs[0][0], jobs[0][1], jobs[0][2], residual=jobs[0][3], relu=True, prec=4, pool=reqs[0])
    else:
        ops.conv2d_grouped(jobs, 4)
    torch.cuda.synchronize()
    for i, (q, out, rbuf, req) in enumerate(zip(probs, outs, rbufs, reqs)):
        what = "%s %s %s problem %d" % (shape, "res" if use_res else "plain", pool, i)
        ref = torch.relu(q["y"] + _f16(q["res"])) if use_res else torch.relu(q["y"])
        got = out.to_f32().cpu()
        assert bool(torch.isfinite(got).all()), what
        whole = rel_l2(got, ref)
        worst, where = worst_block(got, ref, bm=256, cols=128)
        print("%s: whole map %.3g worst block %.3g (bar %.3g) at %s" % (what, whole, worst, BARS[4], where))
        assert whole < BARS[4] and worst < BARS[4], (what, whole, worst, where)
        bits = out.hi.view(torch.int16)
        assert not bool(bits[:, 0].any() | bits[:, -1].any()) and not bool(bits[:, :, 0].any() | bits[:, :, -1].any()), "halo written"
        if rbuf is not None:
            assert bool((rbuf[:GUARD] == NAN16).all()) and bool((rbuf[-GUARD:] == NAN16).all())
        if req is not None:
            _check_pooled(req, pool, got, what)


@pytest.mark.parametrize("pool", POOLS[1:])
@pytest.mark.parametrize("use_res", [True, False], ids=["res", "plain"])
def test_pooled_values_equal_in_the_full_and_the_half_tile_schedule(dev, use_res, pool):
    """The same images as ONE full-tiles-only launch and as all-half launches of a few images each: stored maps and pooled values
    torch.equal (a 64-row block is (rows 0..31) + (rows 32..63), pixels ascending, in both tile shapes)."""
    from agplace_amd import ops
    (n, h, w), = SHAPES["full"]
    q = _problem(0, n, h, w)
    xm = ops.pack_f32(q["x"].to(dev), 128, 1, 4)
    cw = ops.ConvWeights(q["wt"].to(dev), q["scale"].to(dev), q["shift"].to(dev), 1, 1)
    rm = _nan_guarded_residual(q["res"], dev)[0] if use_res else None
    out, req = ops.SplitMap.alloc(n, h, w, 128, 1, 4, dev), _request(pool, dev)
    assert regime(ops.conv_tile_plan([(xm, cw, out, rm, True, req)], 4)) == "full-only"
    ops.conv2d(xm, cw, out, residual=rm, relu=True, prec=4, pool=req)
    k = 7
    for a in list(range(0, n - k, k)) + [n - k]:
        oc, rc = ops.SplitMap.alloc(k, h, w, 128, 1, 4, dev), _request(pool, dev)
        job = (ops.slice_map(xm, a, a + k), cw, oc, None if rm is None else ops.slice_map(rm, a, a + k), True, rc)
        assert regime(ops.conv_tile_plan([job], 4)) == "all-half"
        ops.conv2d(job[0], cw, oc, residual=job[3], relu=True, prec=4, pool=rc)
        assert rc.fused and torch.equal(oc.hi, out.hi[a:a + k]), (pool, a)
        if pool == "sq":
            bpi = req.blocks // n
            full = req.partial.view(-1, 2, 128)[:req.blocks]
            assert torch.equal(rc.partial.view(-1, 2, 128)[:rc.blocks], full[a * bpi:(a + k) * bpi]), (pool, a)
        else:
            assert torch.equal(rc.mean, req.mean[a:a + k]) and torch.equal(rc.gem, req.gem[a:a + k]), (pool, a)
