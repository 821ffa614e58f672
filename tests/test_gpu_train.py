"""-m gpu parity tests of the training path (train-mode BatchNorm, conv dgrad/wgrad, pooling backward)
against autograd through the fp64 CPU oracle.  Bar: 1e-3 relative (north star)."""
import time

import pytest
import torch
import torch.nn.functional as F

from oracle import nets, resnet
from gpu_util import rel_l2, randomize_bn, cpu_state

pytestmark = pytest.mark.gpu
TOL = 1e-3


def test_bn_stats_matches_torch_batchnorm(dev):
    from agplace_amd import ops, train_graph
    torch.manual_seed(0)
    bn = torch.nn.BatchNorm2d(64).to(dev)
    bn.weight.data.uniform_(0.5, 1.5); bn.bias.data.normal_(0, 0.2)
    bn.running_mean.normal_(0, 0.3); bn.running_var.uniform_(0.5, 2.0)
    ref = torch.nn.BatchNorm2d(64)
    ref.load_state_dict({k: v.cpu() for k, v in bn.state_dict().items()})
    x = torch.randn(3, 64, 9, 11) * 2 + 0.5
    z = ops.pack_f32(x.to(dev), 64, 1, 3)
    mean, rstd, scale, shift = train_graph.bn_stats(z, bn)
    y = ops.SplitMap.alloc(3, 9, 11, 64, 1, 3, dev)
    train_graph.map_affine(z, scale, shift, y, relu=True)
    yr = torch.relu(ref.train()(x))
    assert rel_l2(y.to_f32(), yr) < 1e-5
    assert rel_l2(bn.running_mean, ref.running_mean) < 1e-5 and rel_l2(bn.running_var, ref.running_var) < 1e-5
    assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("cin,cout,k,stride,hw", [(64, 64, 3, 1, (10, 14)), (64, 128, 3, 2, (12, 16)), (64, 128, 1, 2, (12, 16)),
                                                   (128, 256, 3, 1, (7, 9)), (256, 64, 1, 1, (6, 6))])
def test_conv_bn_unit_backward(dev, cin, cout, k, stride, hw):
    from agplace_amd import ops, train_graph
    torch.manual_seed(cin + cout + k)
    conv = torch.nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, bias=(k == 3 and stride == 1)).to(dev)
    bn = torch.nn.BatchNorm2d(cout).to(dev)
    bn.weight.data.uniform_(0.5, 1.5); bn.bias.data.normal_(0, 0.2)
    x = torch.randn(2, cin, *hw)
    ho, wo = ops.conv_out_size(hw[0], k, stride, (k - 1) // 2), ops.conv_out_size(hw[1], k, stride, (k - 1) // 2)
    res = torch.randn(2, cout, ho, wo)
    G = torch.randn(2, cout, ho, wo)
    unit = train_graph.ConvBNUnit(conv, bn, "u", ops.Workspace())
    xm = ops.pack_f32(x.to(dev), cin, 1, 3)
    rm = ops.pack_f32(res.to(dev), cout, 1, 3)
    y = unit.forward(xm, residual=rm, relu=True)
    gy = ops.pack_f32(G.to(dev), cout, 1, 3)
    gx, gres, _ = unit.backward(gy)
    # oracle
    W = conv.weight.detach().cpu().double().requires_grad_(True)
    B = None if conv.bias is None else conv.bias.detach().cpu().double().requires_grad_(True)
    gam = bn.weight.detach().cpu().double().requires_grad_(True)
    bet = bn.bias.detach().cpu().double().requires_grad_(True)
    xr = x.double().requires_grad_(True)
    rr = res.double().requires_grad_(True)
    zr = F.conv2d(xr, W, B, stride, (k - 1) // 2)
    yr = torch.relu(F.batch_norm(zr, None, None, gam, bet, True, 0.0, bn.eps) + rr)
    (yr * G.double()).sum().backward()
    assert rel_l2(y.to_f32(), yr) < 1e-4
    assert rel_l2(gx.to_f32(), xr.grad) < TOL
    assert rel_l2(gres.to_f32(), rr.grad) < TOL
    assert rel_l2(conv.weight.grad, W.grad) < TOL
    assert rel_l2(bn.weight.grad, gam.grad) < TOL and rel_l2(bn.bias.grad, bet.grad) < TOL
    if B is not None:
        # d/dbias through BatchNorm is analytically zero; both sides must be tiny
        assert float(conv.bias.grad.abs().max()) < 1e-3 * float(conv.weight.grad.abs().max())


@pytest.mark.parametrize("cin,cout,hw,n,gscale,k,stride", [
    (64, 64, (10, 14), 2, 1.0, 3, 1), (64, 128, (37, 29), 3, 3e-7, 3, 1), (128, 256, (7, 9), 2, 1.0, 3, 1),
    (256, 256, (14, 84), 4, 1e4, 3, 1), (64, 64, (64, 64), 24, 1e-3, 3, 1),
    # the gather shapes (wgrad_gather_f16_kernel): stage entries and their 1x1 downsamples, odd and even map sizes
    (64, 128, (56, 84), 3, 1.0, 3, 2), (128, 256, (29, 37), 2, 3e-7, 3, 2), (64, 128, (56, 84), 3, 1e4, 1, 2),
    (128, 256, (28, 42), 4, 1.0, 1, 2), (256, 512, (13, 21), 2, 1e-3, 1, 2)])
def test_one_pass_fp16_weight_gradient(dev, cin, cout, hw, n, gscale, k, stride, monkeypatch):
    """agp_conv_desc::in_h16 / out_absmax (csrc/wgrad_tr.hip: wgrad_f16_kernel, wgrad_gather_f16_kernel): the weight gradient of
    a 3x3 stride-1 / stride-2 or 1x1 stride-2 conv as ONE fp16 product -- x from the fp16 operand plane its producer wrote (agp_map_affine's o_h16), g scaled per channel by the
    power of two that the BatchNorm backward's exact max |gz| (agp_bn_bwd's gz_absmax) puts at 2^13..2^14 -- stays inside the
    1e-3 bar against fp64 whatever the gradient's magnitude (3e-7 .. 1e4: fp16's own range would fail both ends), really runs
    (its error is fp16-sized, not the 1e-5 of the three-product kernel), leaves every other gradient untouched and re-zeroes
    the maxima."""
    from agplace_amd import ops, train_graph
    torch.manual_seed(cin + cout + n)
    conv = torch.nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, bias=False).to(dev)
    bn = torch.nn.BatchNorm2d(cout).to(dev)
    bn.weight.data.uniform_(0.5, 1.5); bn.bias.data.normal_(0, 0.2)
    x = torch.randn(n, cin, *hw).relu_()
    ohw = tuple((v + 2 * ((k - 1) // 2) - k) // stride + 1 for v in hw)
    G = torch.randn(n, cout, *ohw) * gscale
    G[:, : cout // 4] *= 1e-3                       # channels of very different magnitude: the operand scale is per channel
    ws = ops.Workspace()
    unit = train_graph.ConvBNUnit(conv, bn, "u", ws)
    x0 = ops.pack_f32(x.to(dev), cin, 1, 3)
    xm = ops.SplitMap.alloc(n, hw[0], hw[1], cin, 1, 3, dev).with_h16()
    train_graph.map_affine(x0, None, None, xm)       # the producer pass writes the pair AND the fp16 plane
    assert rel_l2(xm.to_f32(), x) < 1e-5 and float(xm.h16.float().abs().max()) > 0
    assert rel_l2(xm.h16[:, 1:-1, 1:-1].float().permute(0, 3, 1, 2), x) < 4e-4

    def run(one_pass):
        monkeypatch.setattr(train_graph, "WGRAD_F16", one_pass)
        conv.weight.grad = None; bn.weight.grad = None; bn.bias.grad = None
        unit.forward(xm, relu=False)                 # (no ReLU behind the unit: no kink whose flips would blur the comparison)
        gx, _, _ = unit.backward(ops.pack_f32(G.to(dev), cout, 1, 3))
        return conv.weight.grad.clone(), gx.to_f32().clone(), bn.weight.grad.clone()
    gw3, gx3, gg3 = run(False)
    gw1, gx1, gg1 = run(True)
    am = ws.tensor("u.gabsmax", (cout,), torch.int32, dev)
    assert int(am.abs().max()) == 0                  # consumed and zeroed for the next step
    W = conv.weight.detach().cpu().double().requires_grad_(True)
    gam = bn.weight.detach().cpu().double().requires_grad_(True)
    bet = bn.bias.detach().cpu().double().requires_grad_(True)
    xr = x.double().requires_grad_(True)
    yr = F.batch_norm(F.conv2d(xr, W, None, stride, (k - 1) // 2), None, None, gam, bet, True, 0.0, bn.eps)
    (yr * G.double()).sum().backward()
    e3, e1 = rel_l2(gw3, W.grad), rel_l2(gw1, W.grad)
    assert e3 < 1e-4 and 3e-5 < e1 < TOL, (e3, e1)
    # per output channel too (the small channels must not drown in the large ones' scale)
    per = ((gw1.cpu().double() - W.grad) ** 2).sum((1, 2, 3)).sqrt() / (W.grad ** 2).sum((1, 2, 3)).sqrt()
    assert float(per.max()) < 2e-3, float(per.max())
    assert torch.equal(gx1, gx3) and torch.equal(gg1, gg3)
    # a second backward (the maxima were re-zeroed, the planes are reused) gives the same bits
    gw1b, _, _ = run(True)
    assert torch.equal(gw1b, gw1)


def test_conv_bn_unit_backward_on_frozen_statistics(dev):
    """Eval-mode BatchNorm inside the gradient graph: running statistics used and NOT updated, held constant by the backward
    (the conv bias then has an ordinary gradient)."""
    from agplace_amd import ops, train_graph
    torch.manual_seed(5)
    cin, cout, hw = 64, 128, (9, 12)
    conv = torch.nn.Conv2d(cin, cout, 3, 1, 1, bias=True).to(dev)
    bn = torch.nn.BatchNorm2d(cout).to(dev).eval()
    bn.weight.data.uniform_(0.5, 1.5); bn.bias.data.normal_(0, 0.2)
    bn.running_mean.normal_(0, 0.3); bn.running_var.uniform_(0.5, 2.0)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    x, res, G = torch.randn(2, cin, *hw), torch.randn(2, cout, *hw), torch.randn(2, cout, *hw)
    unit = train_graph.ConvBNUnit(conv, bn, "u", ops.Workspace())
    y = unit.forward(ops.pack_f32(x.to(dev), cin, 1, 3), residual=ops.pack_f32(res.to(dev), cout, 1, 3), relu=True)
    gx, gres, _ = unit.backward(ops.pack_f32(G.to(dev), cout, 1, 3))
    assert torch.equal(rm0, bn.running_mean) and torch.equal(rv0, bn.running_var) and int(bn.num_batches_tracked) == 0
    W = conv.weight.detach().cpu().double().requires_grad_(True)
    B = conv.bias.detach().cpu().double().requires_grad_(True)
    gam = bn.weight.detach().cpu().double().requires_grad_(True)
    bet = bn.bias.detach().cpu().double().requires_grad_(True)
    xr, rr = x.double().requires_grad_(True), res.double().requires_grad_(True)
    zr = F.conv2d(xr, W, B, 1, 1)
    yr = torch.relu(F.batch_norm(zr, rm0.cpu().double(), rv0.cpu().double(), gam, bet, False, 0.0, bn.eps) + rr)
    (yr * G.double()).sum().backward()
    assert rel_l2(y.to_f32(), yr) < 1e-4
    assert rel_l2(gx.to_f32(), xr.grad) < TOL and rel_l2(gres.to_f32(), rr.grad) < TOL
    assert rel_l2(conv.weight.grad, W.grad) < TOL and rel_l2(conv.bias.grad, B.grad) < TOL
    assert rel_l2(bn.weight.grad, gam.grad) < TOL and rel_l2(bn.bias.grad, bet.grad) < TOL


def test_stem_one_pass_weight_gradient_really_runs(dev, monkeypatch):
    """Round 5: the packed 7x7 stem's weight gradient as one fp16 product -- the packing pass writes the input's fp16 plane
    (agp_pack_f32_to_nhwc4_h16: equal to half(x), zero halo), the pooled BatchNorm backward folds max |gz| per channel
    (agp_maxpool_bn_bwd's gz_absmax, re-zeroed by the weight gradient), and conv1.weight.grad differs from the three-product
    kernel's by an fp16-sized amount, not at all for every other parameter."""
    from agplace_amd import ops, train_graph
    from agplace_amd.network.image_fe import ImageFE
    torch.manual_seed(3)
    fe = randomize_bn(ImageFE("resnet18", "2_2_2")).to(dev).train()
    x = (torch.randn(3, 3, 64, 96) * 1.5).to(dev)

    def run(stem16):
        monkeypatch.setattr(train_graph, "WGRAD_F16_STEM", stem16)
        for q in fe.parameters():
            q.grad = None
        maps = fe.fe.forward_maps_train(x)
        grads = []
        g = torch.Generator().manual_seed(1)
        for m in maps:
            gm = ops.SplitMap.alloc(m.n, m.h, m.w, m.c, 1, 3, dev)
            train_graph.pool_bwd(m, gm, gmean=torch.randn(m.n, m.c, generator=g).to(dev))
            grads.append(gm)
        fe.fe.backward_maps(grads)
        return {k: v.grad.clone() for k, v in fe.fe.named_parameters() if v.grad is not None}
    g3 = run(False)
    xin3 = fe.fe._ws.map("t.in", 3, 64, 96, 4, 3, 3, dev)
    g1 = run(True)
    xin = fe.fe._ws.map("t.in", 3, 64, 96, 4, 3, 3, dev)
    assert xin.h16 is not None and xin3 is xin
    h = xin.h16.float()
    assert torch.equal(h[:, 3:-3, 3:-3, :3].permute(0, 3, 1, 2), x.half().float())
    assert float(h[:, :3].abs().max()) == 0 and float(h[:, :, :3].abs().max()) == 0 and float(h[..., 3].abs().max()) == 0
    am = fe.fe._ws.tensor("t.stem.gabsmax", (64,), torch.int32, dev)
    assert int(am.abs().max()) == 0
    e = rel_l2(g1["conv1.weight"], g3["conv1.weight"])
    assert 3e-5 < e < 1e-3, e
    for k in g3:
        if k != "conv1.weight":
            assert torch.equal(g1[k], g3[k]), k


@pytest.mark.parametrize("fe_type,hw,fast", [("resnet18", (64, 96), False), ("resnet50", (96, 96), False),
                                             pytest.param("resnet18", (64, 96), True, id="fast"),
                                             pytest.param("resnet18", (64, 96), "dgrad1", id="dgrad1")])
def test_resnet_trunk_training_gradients(dev, fe_type, hw, fast, monkeypatch):
    """fast: Options.train_precision = 16 (train_graph.FWD_F16) -- the forward of the 3x3 stride-1 convs as ONE fp16 x fp16 product;
    "dgrad1": that plus Options.train_dgrad_products = 1 (train_graph.DGRAD_HI_ONLY) -- the 3x3 data gradients as ONE bf16 product.
    The tight mode holds every parameter gradient to max(1e-3, 3 x the oracle's own response to a 1e-5 input perturbation); the fast
    mode's error and cosine against the same fp64 autograd are MEASURED here (printed: FASTGRAD) and held to the looser bars below
    (tools/grad_prec_emul.py prices this plan at 4.0-4.4 x the tight bar: train-mode BatchNorm amplifies the forward's rounding)."""
    from agplace_amd import ops, train_graph
    from agplace_amd.network.image_fe import ImageFE
    monkeypatch.setattr(train_graph, "FWD_F16", bool(fast))
    monkeypatch.setattr(train_graph, "DGRAD_HI_ONLY", fast == "dgrad1")
    torch.manual_seed(7)
    layers = "2_2_2" if fe_type == "resnet18" else "3_4_6"
    fe = randomize_bn(ImageFE(fe_type, layers)).to(dev).train()
    nb = 3 if fe_type == "resnet18" else 4
    x = torch.randn(nb, 3, *hw)
    maps = fe.fe.forward_maps_train(x.to(dev))
    if fast:      # the one-product path was taken: the 3x3 stride-1 units behind the first keep an fp16 z
        z16 = [n for n, u in fe.fe._units.items() if u.saved[1].lo is None]
        assert len(z16) >= 6, z16
        # ... and the conv1 -> conv2 maps inside the blocks are ONE fp16 plane (train_graph.Y16_ONLY)
        y16 = [n for n, u in fe.fe._units.items() if u.saved[2] is not None and u.saved[2].lo is None]
        assert len(y16) == 6 and all(n.endswith(".c0") for n in y16), y16
    p = torch.tensor([3.0], device=dev)
    g = torch.Generator().manual_seed(1)
    Gm = [torch.randn(nb, m.c, generator=g) for m in maps]
    Gg = torch.randn(nb, maps[-1].c, generator=g)
    mean3, gem3 = ops.pool_map(maps[-1], p)
    grads = []
    for i, m in enumerate(maps):
        gm = ops.SplitMap.alloc(m.n, m.h, m.w, m.c, 1, 3, dev)
        last = i == len(maps) - 1
        train_graph.pool_bwd(m, gm, gmean=Gm[i].to(dev), ggem=Gg.to(dev) if last else None,
                             gem_y=gem3 if last else None, p=p if last else None)
        grads.append(gm)
    fe.fe.backward_maps(grads)
    # oracle: same loss through autograd, train-mode BN
    params = {k: (v.double() if v.is_floating_point() else v) for k, v in cpu_state(fe.fe).items()}
    for k, v in params.items():
        if v.is_floating_point() and "running_" not in k:
            v.requires_grad_(True)
    # Impose the product's activation pattern (ReLU masks, max-pool argmax) on the oracle: a
    # pre-activation within ~1e-5 of zero may legitimately land on the other side of the kink in the
    # two arithmetics, and one such flip moves a layer's gradient by ~sqrt(1/numel) >> 1e-3 (fp32
    # torch autograd differs from fp64 torch by 5e-3 on this very net for that reason).  The forward
    # maps themselves are compared against the unconstrained oracle below.
    pattern = {"relu": (fe.fe._units["t.stem"].output_map().to_f32() > 0).cpu()}
    s_prod = fe.fe._units["t.stem"].output_map().to_f32().cpu()
    pattern["maxpool_idx"] = torch.nn.functional.max_pool2d(s_prod, 3, 2, 1, return_indices=True)[1]
    for name, u in fe.fe._units.items():
        name = name[2:]                                   # keys carry the slot prefix "t."
        if name == "stem" or name.endswith(".ds"):
            continue
        li, bi, ci = name[1:].split(".")
        pattern[f"layer{int(li) + 1}.{bi}.relu{int(ci[1:]) + 1}"] = (u.output_map().to_f32() > 0).cpu()
    def oracle_run(xin):
        for v in params.values():
            v.grad = None
        free = resnet.forward_resnet(xin, params, fe_type, 3, training=True)
        outs = resnet.forward_resnet(xin, params, fe_type, 3, training=True, pattern=pattern)
        loss = sum((o.mean((2, 3)) * Gm[i].double()).sum() for i, o in enumerate(outs))
        loss = loss + (nets.gem(outs[-1], torch.tensor([3.0], dtype=torch.float64)).flatten(1) * Gg.double()).sum()
        loss.backward()
        return [o.detach() for o in free], {k: v.grad.clone() for k, v in params.items() if v.grad is not None}

    free, ref_grads = oracle_run(x.double())
    # Conditioning: a randomly initialised train-mode-BN trunk amplifies perturbations layer by layer
    # (resnet50: a 1e-5 relative input perturbation moves l3 by ~5e-4).  The product stores every
    # activation as hi+lo bf16 (2^-17 relative), i.e. it injects ~4e-6 at each of its ~50 layers, so
    # its error is bounded by a small multiple of the oracle's own response to a 1e-5 perturbation.
    gp = torch.Generator().manual_seed(11)
    free_p, grads_p = oracle_run(x.double() * (1 + 1e-5 * torch.randn(x.shape, generator=gp, dtype=torch.float64)))
    for o, op, m in zip(free, free_p, maps):
        if fast:
            print(f"FASTFWD map rel_l2 {rel_l2(m.to_f32(), o):.2e}")
            assert rel_l2(m.to_f32(), o) < 3e-3
        else:
            assert rel_l2(m.to_f32(), o) < max(1e-4, 3 * rel_l2(op, o))
    # The activation pattern the gradients were computed under is the product's own (see above): check it INDEPENDENTLY
    # against the unconstrained oracle.  The ReLU mask of every stage output may differ only where the oracle's value is
    # at the kink (a handful of elements), never systematically.
    for i, (o, m) in enumerate(zip(free, maps)):
        prod_mask = (m.to_f32() > 0).cpu()
        ref_mask = o > 0
        flips = prod_mask != ref_mask
        frac = float(flips.float().mean())
        assert frac < (2e-3 if fast else 2e-4), (i, frac)
        if flips.any():      # every flipped element is tiny on both sides
            scale = float(o.abs().max())
            lim = (1e-2 if fast else 1e-3) * scale
            assert float(o[flips].abs().max()) < lim and float(m.to_f32().cpu()[flips].abs().max()) < lim
    checked, bad, errs, coss = 0, [], [], []
    for name, prm in fe.fe.named_parameters():
        if name.startswith("fc."):
            continue
        ref = ref_grads[name]
        assert prm.grad is not None, name
        err = rel_l2(prm.grad, ref)
        tol = max(TOL, 3 * rel_l2(grads_p[name], ref))
        if fast:
            g1, g2 = prm.grad.detach().double().cpu().flatten(), ref.double().flatten()
            cos = float((g1 @ g2) / (g1.norm() * g2.norm()).clamp_min(1e-300))
            errs.append((err, name)); coss.append((cos, name))
            tol = 1e-2            # the fast mode's bar: a gradient within 1 % of fp64 autograd, cosine >= 0.9999
            #                       (measured, ResNet18 trunk 3 x 64 x 96: median 3.1e-3, worst 4.4e-3, cosine >= 0.99999)
            if fast == "dgrad1":
                tol = 2e-2        # one-product data gradients on top: within 2 %, cosine >= 0.9998 (measured: see the FASTGRAD line)
            if not cos > (0.9998 if fast == "dgrad1" else 0.9999):
                bad.append((name, 1 - cos, 1e-4))         # (cosine)
        if not err < tol:
            bad.append((name, err, tol))
        checked += 1
    if fast:
        errs.sort(); coss.sort()
        print(f"FASTGRAD rel_l2 median {errs[len(errs) // 2][0]:.2e} worst {errs[-1][0]:.2e} ({errs[-1][1]}); "
              f"cosine worst {coss[0][0]:.6f} ({coss[0][1]}) over {checked} parameter tensors")
    print('GRADERR ' + ' '.join(f'{n}:{e:.1e}/{t:.1e}' for n, e, t in bad))
    assert not bad, bad[:5]
    assert checked > 40


@pytest.mark.parametrize("c,stride2,relu1", [(64, False, True), (128, False, True), (64, True, True), (64, False, False)])
def test_dgrad_epilogue_reduces_the_consumers_bn_backward_sums(dev, c, stride2, relu1, monkeypatch):
    """agp_conv_desc::bstat_* + agp_bn_bwd_from_partial: in a chain unit1 -> unit2 the data-gradient conv of unit2 adds the other
    branch's gradient in its epilogue and reduces unit1's BatchNorm-backward channel sums there (sum g*[y>0], sum g*[y>0]*zhat):
    every gradient equals the fp64 oracle's, and equals the unfused path (reduction pass + map_add) to rounding."""
    from agplace_amd import ops, train_graph
    torch.manual_seed(c + stride2)
    c2, s2 = (2 * c, 2) if stride2 else (c, 1)
    conv1 = torch.nn.Conv2d(c, c, 3, 1, 1, bias=False).to(dev)
    conv2 = torch.nn.Conv2d(c, c2, 3, s2, 1, bias=False).to(dev)
    bn1, bn2 = torch.nn.BatchNorm2d(c).to(dev), torch.nn.BatchNorm2d(c2).to(dev)
    for bn in (bn1, bn2):
        bn.weight.data.uniform_(0.5, 1.5); bn.bias.data.normal_(0, 0.2)
    n, h, w = 3, 12, 18
    x = torch.randn(n, c, h, w)
    ho, wo = ops.conv_out_size(h, 3, s2, 1), ops.conv_out_size(w, 3, s2, 1)
    G = torch.randn(n, c2, ho, wo)
    A = torch.randn(n, c, h, w)                       # the "other branch" gradient at unit1's output

    def run(fuse):
        monkeypatch.setattr(train_graph, "FUSE_BN_BWD", fuse)
        for m in (conv1, conv2, bn1, bn2):
            for q in m.parameters():
                q.grad = None
        ws = ops.Workspace()
        u1, u2 = train_graph.ConvBNUnit(conv1, bn1, "a", ws), train_graph.ConvBNUnit(conv2, bn2, "b", ws)
        y1 = u1.forward(ops.pack_f32(x.to(dev), c, 1, 3), relu=relu1)
        u2.forward(y1, relu=True)
        am = ops.pack_f32(A.to(dev), c, 1, 3)
        g1, _, (added, part) = u2.backward(ops.pack_f32(G.to(dev), c2, 1, 3), add=am, stats_for=u1)
        assert added == fuse and (part is not None) == fuse
        if not added:
            g1 = train_graph.map_add(g1, am, ops.SplitMap.alloc(n, h, w, c, 1, 3, dev))
        gx, _, _ = u1.backward(g1, partial=part)
        return [gx.to_f32().cpu()] + [q.grad.detach().cpu().clone() for m in (conv1, bn1, conv2, bn2) for q in m.parameters()]
    fused, plain = run(True), run(False)
    for a, b in zip(fused, plain):
        assert rel_l2(a, b) < 2e-5
    # fp64 oracle
    P = [q.detach().cpu().double().requires_grad_(True) for m in (conv1, bn1, conv2, bn2) for q in m.parameters()]
    xr = x.double().requires_grad_(True)
    t = F.batch_norm(F.conv2d(xr, P[0], None, 1, 1), None, None, P[1], P[2], True, 0.0, bn1.eps)
    y1 = torch.relu(t) if relu1 else t
    y2 = torch.relu(F.batch_norm(F.conv2d(y1, P[3], None, s2, 1), None, None, P[4], P[5], True, 0.0, bn2.eps))
    ((y2 * G.double()).sum() + (y1 * A.double()).sum()).backward()
    for a, r in zip(fused, [xr.grad] + [q.grad for q in P]):
        assert rel_l2(a, r) < TOL


@pytest.mark.parametrize("hw,bn_eval", [((22, 30), False), ((17, 23), False), ((22, 30), True)])
def test_stem_backward_through_the_maxpool_without_a_gradient_map(dev, hw, bn_eval, monkeypatch):
    """agp_maxpool_bn_bwd: conv -> BN -> ReLU -> MaxPool(3, 2, 1) backward from the POOLED gradient: BatchNorm / conv gradients
    equal the fp64 oracle's and the separate calls' (max-pool backward into a map, then the unit's backward)."""
    from agplace_amd import ops, train_graph
    torch.manual_seed(hw[0])
    c = 64
    conv = torch.nn.Conv2d(c, c, 3, 1, 1, bias=False).to(dev)
    bn = torch.nn.BatchNorm2d(c).to(dev)
    bn.weight.data.uniform_(0.5, 1.5); bn.bias.data.normal_(0, 0.2)
    bn.running_mean.normal_(0, 0.1); bn.running_var.uniform_(0.5, 1.5)
    if bn_eval:
        bn.eval()
    n = 3
    x = torch.randn(n, c, *hw)
    h2, w2 = ops.conv_out_size(hw[0], 3, 2, 1), ops.conv_out_size(hw[1], 3, 2, 1)
    G = torch.randn(n, c, h2, w2)

    def run(fuse, use_pooled=True):
        monkeypatch.setattr(train_graph, "FUSE_BN_BWD", fuse)
        for q in list(conv.parameters()) + list(bn.parameters()):
            q.grad = None
        ws = ops.Workspace()
        u = train_graph.ConvBNUnit(conv, bn, "s", ws)
        pooled = ops.SplitMap.alloc(n, h2, w2, c, 1, 3, dev)
        argmax = torch.empty((n, h2, w2, c), dtype=torch.uint8, device=dev)
        # fused: BatchNorm apply + ReLU + pool in one pass, the full-size output not stored (saved y is None) and recomputable
        out = u.forward(ops.pack_f32(x.to(dev), c, 1, 3), relu=True, pool=(pooled, argmax))
        assert out is pooled and (u.saved[2] is None) == fuse
        assert u.output_map().h == hw[0]
        gx, _, _ = u.backward(ops.pack_f32(G.to(dev), c, 1, 3), pool_argmax=argmax, pooled=pooled if use_pooled else None)
        return pooled.to_f32().cpu(), [gx.to_f32().cpu()] + [q.grad.detach().cpu().clone() for q in list(conv.parameters()) + list(bn.parameters())]
    pooled, fused = run(True)
    _, plain = run(False)
    _, gathered = run(True, use_pooled=False)          # the channel sums by the gather instead of over the pooled elements
    for a, b, g_ in zip(fused, plain, gathered):
        assert rel_l2(a, b) < 2e-5 and rel_l2(g_, b) < 2e-5
    # channels whose gamma is too small to recover zhat from the pooled value read z at the argmax: the same gradients as the
    # gather over the same forward (the separately stored activation breaks the near-ties of such channels differently: not compared)
    keep = bn.weight.data.clone()
    bn.weight.data[::3] = 1e-6
    bn.weight.data[1::7] *= -1
    _, f2 = run(True)
    _, g2 = run(True, use_pooled=False)
    for a, b in zip(f2, g2):
        assert rel_l2(a, b) < 2e-5
    bn.weight.data.copy_(keep)
    W = conv.weight.detach().cpu().double().requires_grad_(True)
    gam, bet = bn.weight.detach().cpu().double().requires_grad_(True), bn.bias.detach().cpu().double().requires_grad_(True)
    xr = x.double().requires_grad_(True)
    zr = F.conv2d(xr, W, None, 1, 1)
    if bn_eval:
        yr = torch.relu(F.batch_norm(zr, bn.running_mean.cpu().double(), bn.running_var.cpu().double(), gam, bet, False, 0.0, bn.eps))
    else:
        yr = torch.relu(F.batch_norm(zr, None, None, gam, bet, True, 0.0, bn.eps))
    pr = F.max_pool2d(yr, 3, 2, 1)
    (pr * G.double()).sum().backward()
    assert rel_l2(pooled, pr) < 1e-4
    # One ReLU-kink or pool-tie decision taken differently by the two arithmetics moves these small maps' gradients by
    # ~1 / sqrt(elements) (see test_resnet_trunk_training_gradients); the geometry of the gather at odd sizes is pinned by the
    # comparison with the separate calls above, the arithmetic by the even-size cases at the usual tolerance.
    tol = TOL if hw[0] % 2 == 0 else 1e-2
    for a, r in zip(fused, [xr.grad, W.grad, gam.grad, bet.grad]):
        assert rel_l2(a, r) < tol


# ------------------------------------------------------------------ end-to-end model training
def _unit_mask(u):
    return (u.output_map().to_f32() > 0).cpu()


def trunk_pattern(trunk, slot=0):
    """Activation pattern (ReLU masks, max-pool argmax) of a ResNet's last training forward (of `slot`), keyed
    as oracle.resnet.forward_resnet(pattern=...) expects."""
    pre = "t." if slot == 0 else f"t{slot}."
    pat = {"relu": _unit_mask(trunk._units[pre + "stem"])}
    s_prod = trunk._units[pre + "stem"].output_map().to_f32().cpu()
    pat["maxpool_idx"] = F.max_pool2d(s_prod, 3, 2, 1, return_indices=True)[1]
    for name, u in trunk._units.items():
        if not name.startswith(pre):
            continue
        name = name[len(pre):]
        if name == "stem" or name.endswith(".ds"):
            continue
        li, bi, ci = name[1:].split(".")
        pat[f"layer{int(li) + 1}.{bi}.relu{int(ci[1:]) + 1}"] = _unit_mask(u)
    return pat


# the training modes, as Options fields (the public switch: MM.forward_q / DBVanilla2D.forward_db enter train_graph.training_mode)
MODES = {"tight": {}, "fast": dict(train_precision=16), "dgrad1": dict(train_precision=16, train_dgrad_products=1)}
# fast modes: (rel-L2 bar, cosine bar) of every parameter gradient against fp64 autograd -- test_resnet_trunk_training_gradients'
FAST_BARS = {"fast": (1e-2, 0.9999), "dgrad1": (2e-2, 0.9998)}
# ... except for the parameters whose gradient is ONE cancelling sum over the batch and the channels: the GeM exponents (".p":
# the gradient of (mean x^p)^(1/p) in p is a covariance of log x under the weights x^p) and the fusion ODE's fc biases: the
# forward's fp16 rounding of the last maps (3e-3, FASTFWD) reaches them amplified by that cancellation.  Their bars are 2 x the
# trunk's; measured (MI355X), the same in "fast" and "dgrad1" (so from the forward, not from the data gradients; the tight mode,
# same kernels outside the convs, holds them at 1e-3): dbimage_pools.0.p 1.77e-2 (satellite), fuseblocktoshallow.blocks.2.blocks.0.
# func.func.fc.bias / .weight 1.62e-2, cosine 0.99987 (next to the voxel branch: level 3 of the fusion over 3 queries)
CANCELLING = (".p", "func.func.fc.bias", "func.func.fc.weight")
FAST_BARS_CANCELLING = {"fast": (2e-2, 0.9998), "dgrad1": (4e-2, 0.9996)}
# model outputs against the unconstrained fp64 oracle
OUT_BARS = {"tight": 1e-3, "fast": 3e-3, "dgrad1": 3e-3}


def _compare_grads(model, params, run_oracle, perturb, min_checked, skip=(), must=(), batch_stats=True, mode="tight"):
    """Product .grad vs fp64 oracle autograd.  mode "tight": tolerance max(TOL, 3x the oracle's own response to a 1e-5
    relative input perturbation) -- see test_resnet_trunk_training_gradients.  mode "fast" / "dgrad1" (Options.train_precision
    = 16, and train_dgrad_products = 1): every parameter gradient within FAST_BARS[mode] of fp64 autograd in rel-L2 AND in
    cosine -- the trunk test's bars; one FASTGRAD line (median and worst rel-L2, worst cosine) is printed."""
    def grads(pert):
        for v in params.values():
            v.grad = None
        run_oracle(pert).backward()
        return {k: v.grad.clone() for k, v in params.items() if v.grad is not None}
    fast = mode != "tight"
    ref = grads(False)
    refp = None if fast else grads(True)             # (the fast bars are fixed: no perturbed oracle run)
    bad, checked, seen, errs, coss = [], 0, set(), [], []
    for name, prm in model.named_parameters():
        if name not in ref or name.startswith(skip) or not prm.requires_grad:
            continue
        if float(ref[name].abs().max()) == 0:
            continue
        assert prm.grad is not None, name
        seen.add(name)
        if batch_stats and name.endswith(("conv1.bias", "conv2.bias")):
            # a conv bias in front of batch-statistics BatchNorm has an analytically zero gradient: both sides tiny
            # (frozen statistics, batch_stats=False: it is an ordinary gradient and is compared below)
            wg = dict(model.named_parameters())[name[:-4] + "weight"].grad
            assert float(prm.grad.abs().max()) < 1e-3 * float(wg.abs().max()), name
            continue
        r = ref[name].reshape(prm.grad.shape)
        err = rel_l2(prm.grad, r)
        if fast:
            tol, cbar = (FAST_BARS_CANCELLING if name.endswith(CANCELLING) else FAST_BARS)[mode]
            g1, g2 = prm.grad.detach().double().cpu().flatten(), r.double().flatten()
            cos = float((g1 @ g2) / (g1.norm() * g2.norm()).clamp_min(1e-300))
            errs.append((err, name)); coss.append((cos, name))
            if not cos >= cbar:
                bad.append((name + " (1 - cosine)", 1 - cos, 1 - cbar))
        else:
            tol = max(TOL, 3 * rel_l2(refp[name].reshape(r.shape), r))
        if not err < tol:
            bad.append((name, err, tol))
        checked += 1
    if fast:
        errs.sort(); coss.sort()
        print(f"FASTGRAD [{mode}] rel_l2 median {errs[len(errs) // 2][0]:.2e} ({errs[len(errs) // 2][1]}) worst {errs[-1][0]:.2e} "
              f"({errs[-1][1]}); cosine worst {coss[0][0]:.6f} ({coss[0][1]}) over {checked} parameter tensors")
    print("GRADERR " + " ".join(f"{n}:{e:.1e}/{t:.1e}" for n, e, t in bad))
    assert not bad, bad[:6]
    assert checked >= min_checked, checked
    assert not [m for m in must if m not in seen], [m for m in must if m not in seen]


# Path census of the fast modes, derived once from the rules of ConvBNUnit.forward / reads_f16_plane_only: a unit's forward is ONE
# fp16 product (its z one fp16 plane, saved[1].lo is None) when it is not the stem, is a 3x3 stride-1 conv or a stage entry (3x3
# stride 2, 1x1 stride-2 downsample), has in and out channels divisible by 64 and its input map keeps an fp16 plane; a unit's output
# is ONE fp16 plane (saved[2].lo is None) when its only reader is such a 3x3 stride-1 unit (a block's conv1 -> conv2).
# ResNet18 "2_2_2" (64_128_256): every unit but the stem (the max-pooled stem output keeps the plane for l0.0.c0; every block output
# keeps it for the next block's entries) ...
TRUNK18_Z16 = frozenset(f"l{li}.{bi}.c{ci}" for li in range(3) for bi in range(2) for ci in range(2)) | {"l1.0.ds", "l2.0.ds"}
TRUNK18_Y16 = frozenset(f"l{li}.{bi}.c0" for li in range(3) for bi in range(2))
# ... the stage-2 BasicBlock (stage2fuse_blockadd.py, forward_map_train): its input is the trunk map plus the broadcast vector
# (ops.bcast_add writes no fp16 plane), so its conv1 keeps three products; conv2 reads conv1's output, stored as one fp16 plane
STG2_Z16 = frozenset({"t.c2"})
STG2_Y16 = frozenset({"t.c1"})


def _single_plane(units):
    z16 = {n for n, u in units.items() if u.saved[1].lo is None}
    y16 = {n for n, u in units.items() if u.saved[2] is not None and u.saved[2].lo is None}
    return z16, y16


def _fast_path_census(mode, trunks=(), blocks=()):
    """trunks: (label, resnet trunk, slot prefix); blocks: (label, stage-2 BasicBlock).  In a fast mode exactly the expected units
    ran in one-product form (a silent fall-back to three products fails); in the tight mode none.  Every 3x3 unit carries
    the data-gradient mode of its forward (_dgrad_hi_only) -- set in "dgrad1" only."""
    fast = mode != "tight"
    units = []
    for label, trunk, pre in trunks:
        us = {n[len(pre):]: u for n, u in trunk._units.items() if n.startswith(pre)}
        assert len(us) == 15, (label, sorted(us))
        z16, y16 = _single_plane(us)
        print(f"CENSUS [{mode}] {label} one-product z: {sorted(z16)}; one-plane outputs: {sorted(y16)}")
        assert z16 == (TRUNK18_Z16 if fast else set()), (label, sorted(z16 ^ TRUNK18_Z16))
        assert y16 == (TRUNK18_Y16 if fast else set()), (label, sorted(y16 ^ TRUNK18_Y16))
        units += us.values()
    for label, blk in blocks:
        us = {u.tag: u for u in blk._units}
        z16, y16 = _single_plane(us)
        print(f"CENSUS [{mode}] {label} one-product z: {sorted(z16)}; one-plane outputs: {sorted(y16)}")
        assert z16 == (STG2_Z16 if fast else set()) and y16 == (STG2_Y16 if fast else set()), (label, z16, y16)
        units += us.values()
    for u in units:       # (the switch as it stood at the unit's forward; its backward applies it to the 3x3 data gradients)
        assert u._dgrad_hi_only == (mode == "dgrad1"), (u.tag, u._dgrad_hi_only)


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _assert_dgrad1_ran(grads, fast_grads, names):
    """dgrad1 only: the same state and input in the "fast" mode (three-product data gradients) give conv weight gradients that
    are NOT bit-equal -- the one-product data gradient ran.  `names`: the conv weights whose gradient passes a 3x3 data gradient."""
    same = [n for n in names if torch.equal(grads[n], fast_grads[n])]
    assert not same and len(names) > 0, same


def _conv_weights(model, prefix, exclude=()):
    return [n for n, p in model.named_parameters() if n.startswith(prefix) and p.dim() == 4 and n not in exclude]


_MM_CASES = [pytest.param("tight", 1, "train", 4, (64, 128), id="1-train"), pytest.param("tight", 2, "train", 4, (64, 128), id="2-train"),
             pytest.param("tight", 1, "eval", 4, (64, 128), id="1-eval")]
_MM_CASES += [pytest.param(m, nl, bm, 4, (64, 128), id=f"{m}-{nl}-{bm}") for m in ("fast", "dgrad1")
              for nl, bm in ((1, "train"), (2, "train"), (1, "eval"))]
# the bench's query batch shape (two of its 224 x 1344 panoramas: layer 3 at 14 x 84, the stage-2 block there)
_MM_CASES += [pytest.param("dgrad1", 1, "train", 2, (224, 1344), id="dgrad1-bench-2x224x1344")]


@pytest.mark.parametrize("mode,nlayers,bn_mode,nq,hw", _MM_CASES)
def test_mm_end_to_end_training_gradients(dev, mode, nlayers, bn_mode, nq, hw):
    """.train() MM: loss on the embedding and two auxiliary outputs -> every parameter's gradient
    (ResNet convs/BNs, GeM exponents, fusion path, stage-2 conv block and projections).  nlayers = 2: opt.stg2nlayers
    stacked stage-2 layers (reference stage2fuse_blockadd.py:190, layer i+1 reads layer i's map).
    bn_mode "eval": .eval() with gradients enabled -- fine-tuning on frozen BatchNorm statistics (F.batch_norm with
    training=False under autograd): running statistics used and left untouched, constants of the backward.
    mode "fast" / "dgrad1": the model built with Options(train_precision=16[, train_dgrad_products=1]) -- the step bench.py times
    as train.fast_mode: every gradient at the trunk test's fast bars (_compare_grads), exactly the expected units in one-product
    form (_fast_path_census), and under dgrad1 conv weight gradients that differ from the fast mode's on the same state and input."""
    t0 = time.perf_counter()
    training = bn_mode == "train"
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    from gpu_util import to_dev
    opt = Options(stg2nlayers=nlayers, **MODES[mode])
    torch.manual_seed(21)
    model = randomize_bn(MM(opt=opt)).to(dev).train(training)
    state0 = {k: v.clone() for k, v in model.state_dict().items()}
    data = nets.synth_query(nq, hw[0], hw[1], opt, seed=5)
    ddev = to_dev(data, dev)
    g = torch.Generator().manual_seed(2)
    G = [torch.randn(nq, 256, generator=g) for _ in range(4)]

    def step(m):
        out = m(ddev, mode="q")
        loss = (out["embedding"] * G[0].to(dev)).sum() + (out["stg2imagevec"] * G[1].to(dev)).sum() \
            + (out["imagevec_org"] * G[2].to(dev)).sum() + (out["stg2fusevec"] * G[3].to(dev)).sum()
        loss.backward()
        return out
    before = model.image_fe.fe.bn1.running_mean.clone()
    out = step(model)
    assert torch.equal(before, model.image_fe.fe.bn1.running_mean) != training     # running stats updated in .train() only
    _fast_path_census(mode, [("image_fe", model.image_fe.fe, "t.")],
                      [(f"stg2fuseblock.ffnsimg.{li}", model.stg2fuseblock.ffnsimg[li]) for li in range(nlayers)])
    if mode == "dgrad1":
        twin = MM(opt=opt.copy(train_dgrad_products=3)).to(dev).train(training)
        twin.load_state_dict(state0)
        step(twin)
        _assert_dgrad1_ran(_grads(model), _grads(twin), _conv_weights(model, "image_fe.fe.")
                           + [f"stg2fuseblock.ffnsimg.{li}.conv1.weight" for li in range(nlayers)])
    params = {k: (v.double() if v.is_floating_point() else v) for k, v in cpu_state(model).items()}
    for k, v in params.items():
        if v.is_floating_point() and "running_" not in k and not k.endswith("_weight"):
            v.requires_grad_(True)
    pattern = trunk_pattern(model.image_fe.fe)
    for li in range(nlayers):
        u1, u2 = model.stg2fuseblock.ffnsimg[li]._units
        pattern[f"stg2fuseblock.ffnsimg.{li}.relu1"] = _unit_mask(u1)
        pattern[f"stg2fuseblock.ffnsimg.{li}.relu2"] = _unit_mask(u2)
    d64 = {k: ([t.double() for t in v] if isinstance(v, list) else v.double()) for k, v in data.items()}
    gp = torch.Generator().manual_seed(3)
    noise = 1 + 1e-5 * torch.randn(d64["query_image"].shape, generator=gp, dtype=torch.float64)

    def run_oracle(pert):
        d = dict(d64)
        if pert:
            d["query_image"] = d64["query_image"] * noise
        ref = nets.mm_forward_q(d, params, opt, training=training, pattern=pattern)
        return (ref["embedding"] * G[0].double()).sum() + (ref["stg2imagevec"] * G[1].double()).sum() \
            + (ref["imagevec_org"] * G[2].double()).sum() + (ref["stg2fusevec"] * G[3].double()).sum()

    free = nets.mm_forward_q(d64, params, opt, training=training)
    for k in ("embedding", "stg2imagevec", "imagevec_org", "shallowvec_org", "stg2fusevec"):
        assert rel_l2(out[k], free[k]) < OUT_BARS[mode], (k, rel_l2(out[k], free[k]))
    must = ["image_fe.fe.conv1.weight", "image_fe.fe.layer3.1.bn2.weight", "image_pool.p",
            "stg2fuseblock.poolimage.p", "stg2fuseblock.projsfuseimg.0.0.weight",
            "stg2fuseblock.ffnsimg.0.conv1.weight", "stg2fuseblock.ffnsimg.0.bn2.bias",
            "stg2fuseblock.projsimgfuse.0.0.weight", "fuseblocktoshallow.updimsimg.0.weight",
            "fuseblocktoshallow.blocks.0.blocks.0.func.func.fc.weight", "stg2fusefc.weight"]
    if nlayers == 2:
        must += ["stg2fuseblock.ffnsimg.1.conv2.weight", "stg2fuseblock.projsfuseimg.1.0.weight",
                 "stg2fuseblock.projsimgfuse.1.0.weight", "stg2fuseblock.ffnsfuse.1.ffns.0.fc1.weight"]
    if not training:
        must += ["stg2fuseblock.ffnsimg.0.conv1.bias"]
    _compare_grads(model, params, run_oracle, noise, min_checked=65, skip=("image_fe.fe.fc.",), must=tuple(must),
                   batch_stats=training, mode=mode)
    print(f"WALL mm [{mode}-{nlayers}-{bn_mode} {nq}x{hw[0]}x{hw[1]}] {time.perf_counter() - t0:.1f} s")


_DB_CASES = [pytest.param("tight", dict(), "train", (2, 3, 64), id="variant0-train"),
             pytest.param("tight", dict(maptype="satellite_roadmap"), "train", (2, 3, 64), id="variant1-train"),
             pytest.param("tight", dict(maptype="satellite_roadmap", share_dbfe=True), "train", (2, 3, 64), id="variant2-train"),
             pytest.param("tight", dict(maptype="satellite_roadmap", share_dbfe=True), "eval", (2, 3, 64), id="variant3-eval")]
_DB_CASES += [pytest.param(m, v, "train", (2, 3, 64), id=f"{m}-{vid}-train") for m in ("fast", "dgrad1")
              for vid, v in (("satellite", dict()), ("shared-roadmap", dict(maptype="satellite_roadmap", share_dbfe=True)))]
# the bench's database batch shape: [2, 2, 1, 3, 256, 256] aerial tiles (layer 3 at 16 x 16)
_DB_CASES += [pytest.param("dgrad1", dict(), "train", (2, 2, 256), id="dgrad1-bench-2x2x1x256")]


@pytest.mark.parametrize("mode,variant,bn_mode,shape", _DB_CASES)
def test_dbvanilla2d_end_to_end_training_gradients(dev, mode, variant, bn_mode, shape):
    """share_dbfe: ONE trunk over both map types (reference models_baseline/dbvanilla2d.py:69-72); its gradients are the
    sum over the two applications.  bn_mode "eval": gradients through eval-mode (frozen-statistics) BatchNorm.
    mode "fast" / "dgrad1": Options(train_precision=16[, train_dgrad_products=1]) as in test_mm_end_to_end_training_gradients;
    the census covers each trunk, or both slots ("t.", "t1.") of the shared one."""
    t0 = time.perf_counter()
    training = bn_mode == "train"
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.options import Options
    opt = Options(**variant, **MODES[mode])
    torch.manual_seed(22)
    model = randomize_bn(DBVanilla2D(mode="db", dim=256, opt=opt)).to(dev).train(training)
    state0 = {k: v.clone() for k, v in model.state_dict().items()}
    nmap = len(opt.maptype.split("_"))
    b, ndb, hw = shape
    db_map = torch.randn(b, ndb, nmap, 3, hw, hw)
    G = torch.randn(b, ndb, 256)

    def step(m):
        out = m({"db_map": db_map.to(dev)}, mode="db")["embedding"]
        (out * G.to(dev)).sum().backward()
        return out
    out = step(model)
    shared = opt.share_dbfe is True
    if shared:
        trunks = [("dbimage_fes.0 slot 0", model.dbimage_fes[0].fe, "t."), ("dbimage_fes.0 slot 1", model.dbimage_fes[0].fe, "t1.")]
    else:
        trunks = [(f"dbimage_fes.{i}", model.dbimage_fes[i].fe, "t.") for i in range(nmap)]
    _fast_path_census(mode, trunks)
    if mode == "dgrad1":
        twin = DBVanilla2D(mode="db", dim=256, opt=opt.copy(train_dgrad_products=3)).to(dev).train(training)
        twin.load_state_dict(state0)
        step(twin)
        # (the last conv's weight gradient comes from the pooling alone: no data gradient in front of it)
        _assert_dgrad1_ran(_grads(model), _grads(twin), [n for i in range(1 if shared else nmap) for n in _conv_weights(
            model, f"dbimage_fes.{i}.fe.", exclude=(f"dbimage_fes.{i}.fe.layer3.1.conv2.weight",))])
    params = {k: (v.double() if v.is_floating_point() else v) for k, v in cpu_state(model).items()}
    for k, v in params.items():
        if v.is_floating_point() and "running_" not in k:
            v.requires_grad_(True)
    patterns = [trunk_pattern(model.dbimage_fes[0 if shared else i].fe, slot=i if shared else 0) for i in range(nmap)]
    gp = torch.Generator().manual_seed(3)
    noise = 1 + 1e-5 * torch.randn(db_map.shape, generator=gp, dtype=torch.float64)

    def run_oracle(pert):
        x = db_map.double() * noise if pert else db_map.double()
        ref = nets.dbvanilla2d_forward_db({"db_map": x}, params, opt, training=training, patterns=patterns)
        return (ref["embedding"] * G.double()).sum()

    free = nets.dbvanilla2d_forward_db({"db_map": db_map.double()}, params, opt, training=training)["embedding"]
    assert rel_l2(out, free) < OUT_BARS[mode], rel_l2(out, free)
    nfe = len(model.dbimage_fes)
    _compare_grads(model, params, run_oracle, noise, min_checked=48, skip=tuple(f"dbimage_fes.{i}.fe.fc." for i in range(nfe)),
                   must=("dbimage_fes.0.fe.conv1.weight", "dbimage_pools.0.p", "dbimage_mlps.0.seq.0.weight"), batch_stats=training,
                   mode=mode)
    print(f"WALL db [{mode}-{bn_mode} {b}x{ndb}x{nmap}x{hw}x{hw}] {time.perf_counter() - t0:.1f} s")


def test_training_gradients_are_bit_repeatable(dev):
    """Round 5 (tools/repeat_stress.py): forward + backward of MM and DBVanilla2D from the same state give the SAME bits every
    time -- every parameter gradient, the GeM exponents' and the LayerNorm gains / biases included (those were summed with one
    atomicAdd per wave / per element and differed by ~1e-5 relative from run to run; now a fixed-order sum over the grid)."""
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    from gpu_util import to_dev
    opt = Options()
    torch.manual_seed(4)
    mq = randomize_bn(MM(opt=opt)).to(dev).train()
    mdb = randomize_bn(DBVanilla2D("db", opt.features_dim, opt=opt)).to(dev).train()
    data = to_dev(nets.synth_query(3, 64, 128, opt, seed=8), dev)
    nmap = len(opt.maptype.split("_"))
    db = {"db_map": torch.randn(3, 2, nmap, 3, 64, 64, generator=torch.Generator().manual_seed(9)).to(dev)}
    g = torch.Generator().manual_seed(2)
    Gq, Gd = torch.randn(3, 256, generator=g).to(dev), torch.randn(3, 2, 256, generator=g).to(dev)
    named = [("q." + n, p) for n, p in mq.named_parameters()] + [("db." + n, p) for n, p in mdb.named_parameters()]

    def grads():
        for _, p in named:
            p.grad = None
        fq, fd = mq(data, mode="q"), mdb(db, mode="db")
        ((fq["embedding"] * Gq).sum() + (fq["stg2imagevec"] * Gq).sum() + (fd["embedding"] * Gd).sum()).backward()
        return {n: p.grad.clone() for n, p in named if p.grad is not None}
    g0 = grads()
    assert any(n.endswith(".p") for n in g0) and len(g0) > 100
    for _ in range(4):
        g1 = grads()
        diff = [n for n in g0 if not torch.equal(g0[n], g1[n])]
        assert not diff, diff[:8]


def test_adam_steps_reduce_a_matching_loss(dev):
    """Three optimizer steps on a fixed batch, query and database networks together (train.py:337-341
    shape of use): the loss goes down and every trainable parameter moves."""
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.options import Options
    from gpu_util import to_dev
    opt = Options()
    torch.manual_seed(23)
    mq = MM(opt=opt).to(dev).train()
    mdb = DBVanilla2D(mode="db", dim=256, opt=opt).to(dev).train()
    data = to_dev(nets.synth_query(2, 64, 128, opt, seed=6), dev)
    nmap = len(opt.maptype.split("_"))
    db = {"db_map": torch.randn(2, 2, nmap, 3, 64, 64).to(dev)}
    prm = [p for p in list(mq.parameters()) + list(mdb.parameters()) if p.requires_grad]
    optim = torch.optim.Adam(prm, lr=1e-4)
    w0 = mq.image_fe.fe.layer2[0].conv1.weight.detach().clone()
    losses = []
    for _ in range(3):
        optim.zero_grad(set_to_none=True)
        q = mq(data, mode="q")["embedding"]
        d = mdb(db, mode="db")["embedding"]
        loss = ((q[:, None, :] - d) ** 2).sum(-1).mean()
        loss.backward()
        optim.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0], losses
    assert not torch.equal(w0, mq.image_fe.fe.layer2[0].conv1.weight)


def _imagefe_step(fe, x, dev):
    """One standalone training step of an ImageFE trunk (whatever mode the process-wide switches hold): its gradients."""
    from agplace_amd import ops, train_graph
    for q in fe.parameters():
        q.grad = None
    maps = fe.fe.forward_maps_train(x)
    g = torch.Generator().manual_seed(1)
    grads = []
    for m in maps:
        gm = ops.SplitMap.alloc(m.n, m.h, m.w, m.c, 1, 3, dev)
        train_graph.pool_bwd(m, gm, gmean=torch.randn(m.n, m.c, generator=g).to(dev))
        grads.append(gm)
    fe.fe.backward_maps(grads)
    return _grads(fe)


def test_training_mode_is_per_model(dev):
    """The training mode belongs to the model whose Options select it, not to the process: MM.forward_q / DBVanilla2D.forward_db
    set train_graph's switches for their own forward only (train_graph.training_mode).  (a) a dgrad1 MM next to a tight
    DBVanilla2D and (b) the modes swapped: forward q, forward db, one joint backward -- each model's gradients are bit-equal to
    its gradients when it runs alone from the same state.  After a fast MM training forward the switches hold what they held
    before, and a standalone ImageFE trunk step (which relies on them) gives the same bits as before that forward."""
    from agplace_amd import train_graph
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.network.image_fe import ImageFE
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    from gpu_util import to_dev
    base = Options()
    torch.manual_seed(61)
    sq = {k: v.clone() for k, v in randomize_bn(MM(opt=base)).state_dict().items()}
    sd = {k: v.clone() for k, v in randomize_bn(DBVanilla2D("db", base.features_dim, opt=base), seed=1).state_dict().items()}

    def build(cls, state, mode):
        m = cls(opt=base.copy(**MODES[mode])) if cls is MM else cls("db", base.features_dim, opt=base.copy(**MODES[mode]))
        m.load_state_dict(state)
        return m.to(dev).train()
    mq = {m: build(MM, sq, m) for m in ("tight", "dgrad1")}
    mdb = {m: build(DBVanilla2D, sd, m) for m in ("tight", "dgrad1")}
    data = to_dev(nets.synth_query(2, 64, 128, base, seed=8), dev)
    db = {"db_map": torch.randn(2, 2, 1, 3, 64, 64, generator=torch.Generator().manual_seed(9)).to(dev)}
    g = torch.Generator().manual_seed(2)
    Gq, Gd = torch.randn(2, 256, generator=g).to(dev), torch.randn(2, 2, 256, generator=g).to(dev)

    def run(q=None, d=None):
        """forward q, then forward db, then ONE backward; every model reset to the same state first (parameters, running
        statistics, num_batches_tracked)"""
        for m, st in ((q, sq), (d, sd)):
            if m is not None:
                m.load_state_dict(st)
                for p_ in m.parameters():
                    p_.grad = None
        loss = 0
        if q is not None:
            fq = q(data, mode="q")
            loss = loss + (fq["embedding"] * Gq).sum() + (fq["stg2imagevec"] * Gq).sum()
        if d is not None:
            loss = loss + (d(db, mode="db")["embedding"] * Gd).sum()
        loss.backward()
        return _grads(q) if q is not None else None, _grads(d) if d is not None else None

    for qm, dm in (("dgrad1", "tight"), ("tight", "dgrad1")):
        jq, jd = run(mq[qm], mdb[dm])
        aq, _ = run(q=mq[qm])
        _, ad = run(d=mdb[dm])
        assert len(jq) > 60 and jq.keys() == aq.keys() and jd.keys() == ad.keys()
        diff = [n for n in jq if not torch.equal(jq[n], aq[n])] + [n for n in jd if not torch.equal(jd[n], ad[n])]
        assert not diff, (qm, dm, diff[:8])
    # the process-wide switches are left as they were; a trunk that relies on them runs in the same mode as before
    torch.manual_seed(62)
    fe = randomize_bn(ImageFE("resnet18", "2_2_2")).to(dev).train()
    fe_state = {k: v.clone() for k, v in fe.state_dict().items()}
    x = (torch.randn(3, 3, 64, 96, generator=torch.Generator().manual_seed(63)) * 1.5).to(dev)
    switches = (train_graph.FWD_F16, train_graph.DGRAD_HI_ONLY)
    g0 = _imagefe_step(fe, x, dev)
    for m, inp, kind in ((mq["dgrad1"], data, "q"), (mdb["dgrad1"], db, "db")):
        m(inp, mode=kind)
        assert (train_graph.FWD_F16, train_graph.DGRAD_HI_ONLY) == switches, type(m).__name__
        fe.load_state_dict(fe_state)
        g1 = _imagefe_step(fe, x, dev)
        diff = [n for n in g0 if not torch.equal(g0[n], g1[n])]
        assert g0.keys() == g1.keys() and not diff, (type(m).__name__, diff[:8])


# ------------------------------------------------------------------ Adam trajectory against the fp64 oracle
TRAJ_STEPS, TRAJ_LR = 20, 1e-4


@pytest.fixture(scope="module")
def adam_oracle():
    """The problem (2 queries at 64 x 128, database [2, 2, 1, 3, 64, 64], triplet loss with margin 1.5 so that the hinges stay
    open over the run) and TRAJ_STEPS Adam steps of it through the oracle (oracle.nets + oracle.losses, plain autograd) in fp64 and
    in fp32 -- the fp32 run is the drift of an ordinary fp32 PyTorch implementation, the control the product is measured against."""
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    from oracle import losses as olosses
    opt = Options(train_batch_size=2, negs_num_per_query=2, margin=1.5)
    torch.manual_seed(51)
    mq, mdb = randomize_bn(MM(opt=opt)), randomize_bn(DBVanilla2D("db", opt.features_dim, opt=opt), seed=1)
    pb = dict(opt=opt, sq=cpu_state(mq), sd=cpu_state(mdb),
              names=[("q", n) for n, p_ in mq.named_parameters() if p_.requires_grad]
              + [("db", n) for n, p_ in mdb.named_parameters() if p_.requires_grad],
              data=nets.synth_query(2, 64, 128, opt, seed=52),
              db=torch.randn(2, 2, len(opt.maptype.split("_")), 3, 64, 64, generator=torch.Generator().manual_seed(53)),
              # rows: queries 0, 1, then the database tiles [query, tile] 2 = (0, 0), 3 = (0, 1), 4 = (1, 0), 5 = (1, 1)
              trip=torch.tensor([[0, 2, 3], [0, 2, 4], [1, 4, 5], [1, 4, 2]]))

    def run(dtype):
        st = {w: {k: (v.to(dtype) if v.is_floating_point() else v).clone() for k, v in pb["s" + w[0]].items()} for w in ("q", "db")}
        prm = [st[w][n].requires_grad_(True) for w, n in pb["names"]]
        th0 = [p_.detach().clone() for p_ in prm]
        d = {k: ([t.to(dtype) for t in v] if isinstance(v, list) else (v.to(dtype) if v.is_floating_point() else v))
             for k, v in pb["data"].items()}
        x = pb["db"].to(dtype)
        optim = torch.optim.Adam(prm, lr=TRAJ_LR)
        losses = []
        for _ in range(TRAJ_STEPS):
            optim.zero_grad(set_to_none=True)
            q = nets.mm_forward_q(d, st["q"], opt, training=True)["embedding"]
            e = nets.dbvanilla2d_forward_db({"db_map": x}, st["db"], opt, training=True)["embedding"]
            loss = olosses.compute_loss(pb["trip"], torch.cat([q, e.reshape(-1, e.shape[-1])]), 2, 2, opt.margin)
            loss.backward()
            optim.step()
            losses.append(float(loss.detach()))
        return losses, {w + "." + n: (p_.detach() - t0).double() for (w, n), p_, t0 in zip(pb["names"], prm, th0)}
    return pb, run(torch.float64), run(torch.float32)


def _trajectory_error(losses, upd, ref):
    """(largest relative loss deviation over the steps, median and worst per-tensor relative error of theta_20 - theta_0) against
    the fp64 run `ref`.  Left out: the conv biases in front of batch-statistics BatchNorm (an analytically zero gradient, on
    which Adam's normalised step follows rounding noise; BatchNorm removes them exactly) and tensors no gradient reaches."""
    l64, u64 = ref
    dev_ = max(abs(a - b) / abs(b) for a, b in zip(losses, l64))
    errs = sorted((rel_l2(upd[n], u64[n]), n) for n in u64
                  if not n.endswith(("conv1.bias", "conv2.bias")) and float(u64[n].abs().max()) > 0)
    return dev_, errs[len(errs) // 2][0], errs[-1]


# the fast modes' bars (loss deviation, update median, update worst): 1.5 x the values measured on an MI355X (the test's docstring)
TRAJ_FAST_BARS = {"fast": (1.2e-3, 2.2e-1, 4.3e-1), "dgrad1": (2.3e-3, 2.2e-1, 4.9e-1)}


@pytest.mark.parametrize("mode", ["tight", "fast", "dgrad1"])
def test_adam_trajectory_matches_fp64_oracle(dev, mode, adam_oracle):
    """TRAJ_STEPS Adam steps of query and database networks on one fixed batch (losses.compute_loss, triplet) against the same
    steps through the fp64 oracle: the largest relative loss deviation over the steps and the per-tensor relative error of
    the whole update theta_20 - theta_0 (median, worst).  A ReLU kink cannot be pinned over 20 steps, so the bars are relative
    to an fp32 run of the oracle: the tight mode within 3 x that control; the fast modes within 1.5 x what they measured
    (TRAJ_FAST_BARS).  The loss goes down in every mode.  Measured (MI355X): fp32 control 1.33e-3 / 4.23e-2 / 1.21e-1 (loss
    deviation / update median / worst); tight 1.55e-3 / 8.76e-2 / 2.12e-1; fast 8.12e-4 / 1.48e-1 / 2.87e-1; dgrad1 1.55e-3 /
    1.48e-1 / 3.25e-1.  Adam normalises each tensor's step, so a constant error factor on one gradient is invisible here: the
    end-to-end gradient tests are the ones that catch it."""
    from agplace_amd import losses as plosses
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.network_mm.mm import MM
    from gpu_util import to_dev
    t0 = time.perf_counter()
    pb, ref, ctl = adam_oracle
    opt = pb["opt"].copy(**MODES[mode])
    mq, mdb = MM(opt=opt), DBVanilla2D("db", opt.features_dim, opt=opt)
    mq.load_state_dict(pb["sq"]); mdb.load_state_dict(pb["sd"])
    mq, mdb = mq.to(dev).train(), mdb.to(dev).train()
    own = {"q": dict(mq.named_parameters()), "db": dict(mdb.named_parameters())}
    prm = [own[w][n] for w, n in pb["names"]]
    th0 = [p_.detach().clone() for p_ in prm]
    data, db, trip = to_dev(pb["data"], dev), {"db_map": pb["db"].to(dev)}, pb["trip"].to(dev)
    optim = torch.optim.Adam(prm, lr=TRAJ_LR)
    losses = []
    for _ in range(TRAJ_STEPS):
        optim.zero_grad(set_to_none=True)
        q = mq(data, mode="q")["embedding"]
        e = mdb(db, mode="db")["embedding"]
        loss = plosses.compute_loss(opt, None, trip, torch.cat([q, e.reshape(-1, e.shape[-1])]))
        loss.backward()
        optim.step()
        losses.append(float(loss.detach()))
    upd = {w + "." + n: (p_.detach() - t).double().cpu() for (w, n), p_, t in zip(pb["names"], prm, th0)}
    got, fp32 = _trajectory_error(losses, upd, ref), _trajectory_error(*ctl, ref)
    print(f"TRAJECTORY [{mode}] loss {losses[0]:.4f} -> {losses[-1]:.4f} (fp64 {ref[0][0]:.4f} -> {ref[0][-1]:.4f}); "
          f"loss deviation {got[0]:.2e} (fp32 control {fp32[0]:.2e}); update rel-L2 median {got[1]:.2e} (control {fp32[1]:.2e}), "
          f"worst {got[2][0]:.2e} {got[2][1]} (control {fp32[2][0]:.2e} {fp32[2][1]}); {time.perf_counter() - t0:.1f} s")
    assert losses[-1] < losses[0] and ref[0][-1] < ref[0][0], losses
    if mode == "tight":
        bars = (3 * fp32[0], 3 * fp32[1], 3 * fp32[2][0])
    else:
        bars = TRAJ_FAST_BARS[mode]
    for name, v, bar in zip(("loss deviation", "update median", "update worst"), (got[0], got[1], got[2][0]), bars):
        assert bar is None or v <= bar, (name, v, bar)


@pytest.mark.parametrize("mode,bn_mode,ntd", [pytest.param("tight", "train", 0, id="train-0"), pytest.param("tight", "eval", 0, id="eval-0"),
                                              pytest.param("tight", "train", 1, id="train-1"),
                                              pytest.param("fast", "train", 0, id="fast-train-0"),
                                              pytest.param("dgrad1", "train", 0, id="dgrad1-train-0")])
def test_mm_end_to_end_training_with_sparse_voxel_branch(dev, mode, bn_mode, ntd):
    """bn_mode "eval": the same through eval-mode (frozen-statistics) BatchNorm / MinkowskiBatchNorm.
    .train() MM from query_image + coords/features: gradients of every parameter -- image trunk, MinkFPN
    (sparse convs, MinkowskiBatchNorm, ECA), both GeM/MinkGeM exponents, fusion path, stage-2 image AND sparse
    side -- against fp64 autograd through the oracle.  mode "fast" / "dgrad1": the image side in a fast training mode
    (Options(train_precision=16[, train_dgrad_products=1])) next to the voxel branch, at the fast bars (_compare_grads)."""
    t0 = time.perf_counter()
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    from gpu_util import to_dev
    from oracle import sparse as osp
    # ntd = 1: the voxel FPN's top-down path inside MM (equal voxel planes, see test_gpu_models.py)
    opt = Options(**MODES[mode]) if ntd == 0 else Options(mm_voxfe_ntd=ntd, mm_voxfe_planes="256_256_256", **MODES[mode])
    torch.manual_seed(31)
    model = MM(opt=opt)
    params0 = nets.init_mm_params(opt, seed=21)
    model.load_reference_state_dict(params0)
    training = bn_mode == "train"
    model = model.to(dev).train(training)
    state0 = {k: v.clone() for k, v in model.state_dict().items()}
    data = nets.synth_query(3, 64, 128, opt, seed=15)
    for k in ("vox_levels", "voxfeatvec", "stg2voxvec", "voxvec_fuse"):
        data.pop(k)
    coords, feats = osp.synth_cloud(3, 350, extent=28, seed=16)
    data["coords"], data["features"] = coords, feats
    g = torch.Generator().manual_seed(2)
    keys = ("embedding", "stg2imagevec", "stg2voxvec", "voxvec_org", "stg2fusevec")
    G = {k: torch.randn(3, 256, generator=g) for k in keys}

    def step(m):
        out = m(to_dev(data, dev), mode="q")
        loss = sum((out[k] * G[k].to(dev)).sum() for k in keys)
        loss.backward()
        return out
    out = step(model)
    _fast_path_census(mode, [("image_fe", model.image_fe.fe, "t.")], [("stg2fuseblock.ffnsimg.0", model.stg2fuseblock.ffnsimg[0])])
    if mode == "dgrad1":
        twin = MM(opt=opt.copy(train_dgrad_products=3))
        twin.load_reference_state_dict(params0)
        twin = twin.to(dev).train(training)
        twin.load_state_dict(state0)
        step(twin)
        _assert_dgrad1_ran(_grads(model), _grads(twin), _conv_weights(model, "image_fe.fe.") + ["stg2fuseblock.ffnsimg.0.conv1.weight"])
    params = {k: (v.double() if v.is_floating_point() else v) for k, v in cpu_state(model).items()}
    for k, v in params.items():
        if v.is_floating_point() and "running_" not in k and not k.endswith("_weight"):
            v.requires_grad_(True)
    # activation pattern of the conv parts: image trunk, stage-2 image block, MinkFPN, stage-2 sparse block
    pattern = trunk_pattern(model.image_fe.fe)
    u1, u2 = model.stg2fuseblock.ffnsimg[0]._units
    pattern["stg2fuseblock.ffnsimg.0.relu1"] = _unit_mask(u1)
    pattern["stg2fuseblock.ffnsimg.0.relu2"] = _unit_mask(u2)

    def fmask(sp):
        return ((sp.hi[:sp.n].float() + sp.lo[:sp.n].float()) > 0).float().cpu()
    tr = model.vox_fe._train_obj
    pattern["vox_fe.relu0"] = fmask(tr.u0.saved[3])
    for i in range(3):
        pattern[f"vox_fe.relus.{i}"] = fmask(tr.down[i].saved[3])
        pattern[f"vox_fe.blocks.{i}.0.relu1"] = fmask(tr.blocks[i][0].u1.saved[3])
        pattern[f"vox_fe.blocks.{i}.0.relu2"] = fmask(tr.blocks[i][0].saved[5])
    bt = model.stg2fuseblock.ffnsvox[0]._train_obj
    pattern["stg2fuseblock.ffnsvox.0.relu1"] = fmask(bt.u1.saved[3])
    pattern["stg2fuseblock.ffnsvox.0.relu2"] = fmask(bt.saved[5])
    d64 = {k: ([t.double() for t in v] if isinstance(v, list) else (v.double() if v.is_floating_point() else v))
           for k, v in data.items()}
    gp = torch.Generator().manual_seed(3)
    noise = 1 + 1e-5 * torch.randn(d64["query_image"].shape, generator=gp, dtype=torch.float64)
    fnoise = 1 + 1e-5 * torch.randn(feats.shape, generator=gp, dtype=torch.float64)

    def run_oracle(pert):
        d = dict(d64)
        if pert:
            d["query_image"] = d64["query_image"] * noise
            d["features"] = d64["features"] * fnoise
        ref = nets.mm_forward_q(d, params, opt, training=training, pattern=pattern)
        return sum((ref[k] * G[k].double()).sum() for k in keys)

    free = nets.mm_forward_q(d64, params, opt, training=training)
    for k in keys:
        assert rel_l2(out[k], free[k]) < OUT_BARS[mode], (k, rel_l2(out[k], free[k]))
    _compare_grads(model, params, run_oracle, noise, min_checked=125, skip=("image_fe.fe.fc.",),
                   must=("image_fe.fe.conv1.weight", "vox_fe.conv0.kernel", "vox_fe.blocks.2.0.conv2.kernel",
                         "vox_fe.blocks.1.0.eca.conv.weight", "vox_fe.bns.0.bn.weight", "vox_pool.p",
                         *(("vox_fe.tconvs.0.kernel", "vox_fe.conv1x1s.1.kernel") if ntd else ()),
                         "stg2fuseblock.ffnsvox.0.conv1.kernel", "stg2fuseblock.ffnsvox.0.eca.conv.weight",
                         "stg2fuseblock.projsvoxfuse.0.0.kernel", "stg2fuseblock.projsfusevox.0.0.weight",
                         "stg2fuseblock.poolvox.p", "fuseblocktoshallow.updimsvox.0.weight"), batch_stats=training, mode=mode)
    print(f"WALL mm+vox [{mode}-{bn_mode}-{ntd}] {time.perf_counter() - t0:.1f} s")


def test_two_stream_training_step_gives_the_same_gradients(dev):
    """The database network's forward (and so its backward) on a second HIP stream, as bench.py runs the
    training step: identical parameter gradients (module workspaces are keyed by the launching stream)."""
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.options import Options
    from gpu_util import to_dev
    opt = Options()
    torch.manual_seed(41)
    mq = MM(opt=opt).to(dev).train()
    mdb = DBVanilla2D(mode="db", dim=256, opt=opt).to(dev).train()
    data = to_dev(nets.synth_query(2, 64, 128, opt, seed=7), dev)
    nmap = len(opt.maptype.split("_"))
    db = {"db_map": torch.randn(2, 3, nmap, 3, 64, 64).to(dev)}
    names = [(n, p) for n, p in list(mq.named_parameters()) + list(mdb.named_parameters()) if p.requires_grad]

    def grads(two_streams):
        for _, p in names:
            p.grad = None
        if two_streams:
            side = torch.cuda.Stream(device=dev)
            cur = torch.cuda.current_stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                d = mdb(db, mode="db")["embedding"]
            q = mq(data, mode="q")["embedding"]
            cur.wait_stream(side)
        else:
            q = mq(data, mode="q")["embedding"]
            d = mdb(db, mode="db")["embedding"]
        ((q[:, None, :] - d) ** 2).sum(-1).mean().backward()
        torch.cuda.synchronize()
        return {n: p.grad.clone() for n, p in names if p.grad is not None}
    a, b = grads(False), grads(True)
    assert a.keys() == b.keys() and len(a) > 100
    for n in a:
        assert rel_l2(b[n], a[n]) < 1e-5, n


@pytest.mark.parametrize("cin,cout,h,w,n", [(64, 64, 12, 20, 3), (64, 128, 9, 7, 5), (128, 256, 14, 10, 2), (64, 192, 33, 31, 2)])
def test_conv_epilogue_channel_statistics_equal_reduction_pass(dev, cin, cout, h, w, n):
    """agp_conv_desc.stat_partial (3x3 stride-1 kernel, bf16-pair maps): BatchNorm's batch statistics from the conv
    kernel's per-tile sums equal those of the separate reduction pass over the stored conv output."""
    from agplace_amd import ops, train_graph
    g = torch.Generator().manual_seed(cin + cout + h)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    bias = torch.randn(cout, generator=g)
    xm = ops.pack_f32(x.to(dev), cin, 1, 3)
    cw = ops.ConvWeights(wt.to(dev), None, bias.to(dev), 1, 1)
    z = ops.SplitMap.alloc(n, h, w, cout, 1, 3, dev)
    tiles = ops.conv_stat_tiles(xm, cw, z, 3)
    assert tiles > 0
    part = torch.full((tiles, 2, cout), float("nan"), device=dev)
    ops.conv2d(xm, cw, z, relu=False, prec=3, stat_partial=part)
    bn_a = torch.nn.BatchNorm2d(cout).to(dev).train()
    bn_b = torch.nn.BatchNorm2d(cout).to(dev).train()
    with torch.no_grad():
        for bn in (bn_a, bn_b):
            bn.weight.copy_(torch.linspace(0.5, 1.5, cout))
            bn.bias.copy_(torch.linspace(-0.3, 0.3, cout))
    ref = train_graph.bn_stats(z, bn_a)
    got = train_graph.bn_stats_from_partial(part, tiles, z, bn_b)
    for a, b, name in zip(got, ref, ("mean", "rstd", "scale", "shift")):
        assert float((a - b).abs().max()) <= 2e-6 * float(b.abs().max()) + 1e-7, name
    assert torch.allclose(bn_a.running_var, bn_b.running_var, rtol=1e-5, atol=1e-7)
    # the stride-2 form and the 1x1 / stride-2 downsample run on the generic kernel, which reports its own tiles
    for (wt2, st, pd) in ((wt, 2, 1), (torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5, 2, 0)):
        cw2 = ops.ConvWeights(wt2.to(dev), None, None, st, pd)
        k2 = wt2.shape[-1]
        ho, wo = ops.conv_out_size(h, k2, st, pd), ops.conv_out_size(w, k2, st, pd)
        z2 = ops.SplitMap.alloc(n, ho, wo, cout, 1, 3, dev)
        t2 = ops.conv_stat_tiles(xm, cw2, z2, 3)
        assert t2 == (n * ho * wo + (127 if cout % 128 == 0 else 255)) // (128 if cout % 128 == 0 else 256)
        part2 = torch.full((t2, 2, cout), float("nan"), device=dev)
        ops.conv2d(xm, cw2, z2, relu=False, prec=3, stat_partial=part2)
        assert rel_l2(z2.to_f32(), F.conv2d(x.double(), wt2.double(), None, st, pd)) < 1e-4
        ref2 = train_graph.bn_stats(z2, bn_a)
        got2 = train_graph.bn_stats_from_partial(part2, t2, z2, bn_b)
        for a, b, name in zip(got2, ref2, ("mean", "rstd", "scale", "shift")):
            # (the epilogue sums the values before their 2^-17 storage rounding, the pass after it: 5e-7 of a unit-variance map)
            assert float((a - b).abs().max()) <= 5e-6 * float(b.abs().max()) + 1e-6, (name, st, k2)


@pytest.mark.parametrize("n,h,w", [(3, 64, 96), (2, 50, 38), (5, 32, 32)])
def test_stem_conv_epilogue_channel_statistics_equal_reduction_pass(dev, n, h, w):
    """The same for the packed 7x7/2 stem conv (igemm_d16, 256-row tiles of the plain raster, a ragged last tile)."""
    from agplace_amd import ops, train_graph
    g = torch.Generator().manual_seed(n + h)
    x = torch.randn(n, 3, h, w, generator=g)
    wt = torch.randn(64, 3, 7, 7, generator=g) / (3 * 49) ** 0.5
    xin = ops.pack_f32(x.to(dev), 4, 3, 3)
    cw = ops.ConvWeights(wt.to(dev), None, None, 2, 3, stem=True)
    ho, wo = ops.conv_out_size(h, 7, 2, 3), ops.conv_out_size(w, 7, 2, 3)
    z = ops.SplitMap.alloc(n, ho, wo, 64, 1, 3, dev)
    tiles = ops.conv_stat_tiles(xin, cw, z, 3)
    assert tiles == (n * ho * wo + 255) // 256
    part = torch.full((tiles, 2, 64), float("nan"), device=dev)
    ops.conv2d(xin, cw, z, relu=False, prec=3, stat_partial=part)
    ref_z = F.conv2d(x.double(), wt.double(), None, 2, 3)
    assert rel_l2(z.to_f32(), ref_z) < 1e-4
    bn_a, bn_b = torch.nn.BatchNorm2d(64).to(dev).train(), torch.nn.BatchNorm2d(64).to(dev).train()
    ref = train_graph.bn_stats(z, bn_a)
    got = train_graph.bn_stats_from_partial(part, tiles, z, bn_b)
    for a, b, name in zip(got, ref, ("mean", "rstd", "scale", "shift")):
        assert float((a - b).abs().max()) <= 2e-6 * float(b.abs().max()) + 1e-7, name


def test_frozen_stem_still_trains_the_deeper_layers_and_cumulative_bn_momentum(dev):
    """the autograd anchor of a trunk is any parameter that requires grad -- with conv1 / bn1 frozen the
    deeper layers still receive their gradients; BatchNorm(momentum=None) updates its running statistics with the
    cumulative average 1 / num_batches_tracked like torch."""
    from agplace_amd import ops, train_graph
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.options import Options
    torch.manual_seed(5)
    model = randomize_bn(DBVanilla2D(mode="db", dim=256, opt=Options())).to(dev).train()
    fe = model.dbimage_fes[0].fe
    fe.conv1.weight.requires_grad_(False)
    for p_ in fe.bn1.parameters():
        p_.requires_grad_(False)
    x = torch.randn(2, 3, 1, 3, 64, 64, generator=torch.Generator().manual_seed(2)).to(dev)
    out = model({"db_map": x}, mode="db")["embedding"]
    out.sum().backward()
    assert fe.conv1.weight.grad is None
    assert fe.layer2[0].conv1.weight.grad is not None and float(fe.layer2[0].conv1.weight.grad.abs().max()) > 0
    # momentum=None on the statistics kernel against torch's BatchNorm, two steps from a non-trivial state
    g = torch.Generator().manual_seed(3)
    bn = randomize_bn(torch.nn.BatchNorm2d(64, momentum=None)).to(dev).train()
    ref = torch.nn.BatchNorm2d(64, momentum=None).to(dev).train()
    ref.load_state_dict(bn.state_dict())
    for step in range(2):
        z = (torch.randn(3, 64, 5, 7, generator=g) * (1.0 + step) + 0.5 * step).to(dev)
        train_graph.bn_stats(ops.pack_f32(z, 64, 1, 3), bn)
        ref(z)
    assert int(bn.num_batches_tracked) == 2 == int(ref.num_batches_tracked)
    assert rel_l2(bn.running_mean, ref.running_mean) < 1e-5 and rel_l2(bn.running_var, ref.running_var) < 1e-5


def test_per_rank_batchnorm_differs_from_whole_batch_statistics(dev):
    """Data-parallel training keeps BatchNorm statistics per rank like the reference's default (train.py wraps nothing in
    SyncBN).  This quantifies what that means at the bench's per-rank batch: the same 8 aerial tiles as ONE batch against
    two ranks' worth (4 + 4 tiles, gradients averaged).  Measured (round 2, randomly initialised ResNet18 trunk, 64 x 64
    tiles): embeddings differ by 8e-2, parameter gradients by 0.7 (median) in relative L2 -- a property of the recipe (the
    reference's multi-GPU mode, nn.DataParallel at train.py:253-256, normalises per replica in the same way), not of this
    implementation: each half on its own matches the oracle (test_dbvanilla2d_end_to_end_training_gradients)."""
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.options import Options
    torch.manual_seed(8)
    model = randomize_bn(DBVanilla2D(mode="db", dim=256, opt=Options())).to(dev).train()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.randn(8, 1, 1, 3, 64, 64, generator=torch.Generator().manual_seed(4)).to(dev)
    G = torch.randn(8, 1, 256, generator=torch.Generator().manual_seed(5)).to(dev)

    def run(parts):
        model.load_state_dict(state)
        for p_ in model.parameters():
            p_.grad = None
        outs = []
        for lo, hi in parts:
            o = model({"db_map": x[lo:hi]}, mode="db")["embedding"]
            ((o * G[lo:hi]).sum() / len(parts)).backward()
            outs.append(o.detach())
        return torch.cat(outs), {n: p_.grad.clone() for n, p_ in model.named_parameters() if p_.grad is not None}

    o1, g1 = run([(0, 8)])
    o2, g2 = run([(0, 4), (4, 8)])
    do = rel_l2(o2, o1)
    dg = {n: rel_l2(g2[n], g1[n] / 1.0) for n in g1 if n in g2 and float(g1[n].abs().max()) > 0}
    worst = max(dg.values())
    print(f"PERRANKBN outputs {do:.2e}, gradients median {sorted(dg.values())[len(dg) // 2]:.2e} worst {worst:.2e}")
    assert 1e-4 < do < 1.0 and all(v == v for v in dg.values())          # different, finite, same order of magnitude
