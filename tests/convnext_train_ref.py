"""Reference code of the ConvNeXt training tests (tests/test_convnext_train_host.py, tests/test_gpu_convnext_bwd.py): the
stochastic-depth block restated on tests/convnext_ref.py, closed forms of GELU' and the LayerNorm backward, and the fp64 / fp32
autograd truths the kernel tests compare with.  Everything runs on the CPU.

torchvision is not a dependency.  Its StochasticDepth(p, "row") multiplies each image's branch by bernoulli(1 - p) / (1 - p) in
training and is the identity in eval; CNBlock.forward is `x + stochastic_depth(layer_scale * block(x))`.  With the factor as an
input that is `x + scale[:, None, None, None] * blk.branch(x)`.
"""
import math

import torch

import convnext_ref as R

STAGE_FIRST_BLOCK = (0, 3, 6)


def sd_probs(layers, prob=0.1):
    """p_k of the kept blocks: torchvision assigns prob * k / (18 - 1) over the FULL network before the reference truncates."""
    return [[prob * (STAGE_FIRST_BLOCK[s] + b) / 17.0 for b in range(min(layers[s], R.DEPTHS[s]))] for s in range(3)]


def scaled_block(blk, x, scale):
    return blk(x) if scale is None else x + scale[:, None, None, None] * blk.branch(x)


def forward_maps_scaled(model, x, scales):
    """R.forward_maps with one scale ([n] tensor or None) per block, stage by stage."""
    out, k = [], 0
    for i, layer in enumerate(model.features.children()):
        if i in (1, 3, 5):
            for blk in layer:
                x = scaled_block(blk, x, None if scales is None else scales[k])
                k += 1
            out.append(x)
        else:
            x = layer(x)
    return out


def gelu_grad(x):
    """d/dx GELU(x) = Phi(x) + x phi(x)."""
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def layernorm_bwd(z, gamma, gxn, eps=R.LN_EPS):
    """Closed form the kernels use, over the last dimension: returns (gz, g_gamma, g_beta)."""
    mean = z.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((z - mean) ** 2).mean(-1, keepdim=True) + eps)
    xhat = (z - mean) * rstd
    gxh = gxn * gamma
    gz = rstd * (gxh - gxh.mean(-1, keepdim=True) - xhat * (gxh * xhat).mean(-1, keepdim=True))
    flat = lambda t: t.reshape(-1, t.shape[-1])
    return gz, (flat(gxn) * flat(xhat)).sum(0), flat(gxn).sum(0)


def leaf_params(module, dtype):
    """name -> detached copy of every parameter in `dtype` that requires a gradient."""
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in module.named_parameters()}


def mlp_truth(blk, xn, gy, pix_scale, dtype):
    """Gradients of sum(gy * pix_scale * layer_scale * MLP(xn)) in `dtype`: dict with gxn, w1, b1, w2, b2, ls.  xn, gy: [P, C]."""
    C = xn.shape[1]
    xn = xn.to(dtype).clone().requires_grad_(True)
    w1, b1 = (t.detach().to(dtype).clone().requires_grad_(True) for t in (blk.block[3].weight, blk.block[3].bias))
    w2, b2 = (t.detach().to(dtype).clone().requires_grad_(True) for t in (blk.block[5].weight, blk.block[5].bias))
    ls = blk.layer_scale.detach().to(dtype).reshape(C).clone().requires_grad_(True)
    m = R.gelu_exact(xn @ w1.t() + b1) @ w2.t() + b2
    out = ls * m if pix_scale is None else pix_scale.to(dtype)[:, None] * (ls * m)
    g = torch.autograd.grad((out * gy.to(dtype)).sum(), [xn, w1, b1, w2, b2, ls])
    return dict(zip(("gxn", "w1", "b1", "w2", "b2", "ls"), g))


def dwln_truth(blk, x, gxn, gy, dtype):
    """Gradients of sum(gxn * LN(dwconv(x))) + sum(gy * x): dict with gx, dw, dwb, g, b.  x, gy: [n,C,h,w]; gxn: [n,h,w,C]."""
    x = x.to(dtype).clone().requires_grad_(True)
    dw, ln = blk.block[0], blk.block[2]
    ps = [t.detach().to(dtype).clone().requires_grad_(True) for t in (dw.weight, dw.bias, ln.weight, ln.bias)]
    z = torch.nn.functional.conv2d(x, ps[0], ps[1], padding=3, groups=x.shape[1]).permute(0, 2, 3, 1)
    mean = z.mean(-1, keepdim=True)
    xn = (z - mean) / torch.sqrt(((z - mean) ** 2).mean(-1, keepdim=True) + R.LN_EPS) * ps[2] + ps[3]
    g = torch.autograd.grad((xn * gxn.to(dtype)).sum() + (x * gy.to(dtype)).sum(), [x] + ps)
    return dict(zip(("gx", "dw", "dwb", "g", "b"), g))


def module_truth(mod, x, gout, dtype, want_gx=True):
    """Gradients of sum(gout * mod(x)) for a Sequential of the restatement (downsample, stem): (gx or None, {name: grad})."""
    import copy
    mod = copy.deepcopy(mod).to(dtype)
    x = x.to(dtype).clone().requires_grad_(want_gx)
    names, ps = zip(*mod.named_parameters())
    g = torch.autograd.grad((mod(x) * gout.to(dtype)).sum(), ([x] if want_gx else []) + list(ps))
    return (g[0] if want_gx else None), dict(zip(names, g[1 if want_gx else 0:]))
