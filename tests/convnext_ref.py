"""Torch-CPU restatement of torchvision's convnext_tiny (torchvision is not a dependency), the reference's truncation of it
(network_mm/image_fe.py:59-88,118-150), and seeded non-trivial weights.  Run in fp64 for the truth and in fp32 for the error
floor.  Module and parameter names are torchvision's, so state_dict keys match `agplace_amd.convnext.ConvNeXt`.
"""
import math

import numpy as np
import torch
import torch.nn as nn

DIMS = (96, 192, 384, 768)
DEPTHS = (3, 3, 9, 3)
LN_EPS = 1e-6


def gelu_exact(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


class LayerNorm2d(nn.LayerNorm):
    """LayerNorm over the channels of an NCHW map (biased variance)."""

    def forward(self, x):
        x = x.permute(0, 2, 3, 1)
        mean = x.mean(-1, keepdim=True)
        var = ((x - mean) ** 2).mean(-1, keepdim=True)
        x = (x - mean) / torch.sqrt(var + self.eps) * self.weight + self.bias
        return x.permute(0, 3, 1, 2)


class _GELU(nn.Module):
    def forward(self, x):
        return gelu_exact(x)


class _Permute(nn.Module):
    def __init__(self, dims):
        super().__init__()
        self.dims = dims

    def forward(self, x):
        return x.permute(*self.dims)


class CNBlock(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.block = nn.Sequential(
            nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim, bias=True),
            _Permute([0, 2, 3, 1]),
            nn.LayerNorm(dim, eps=LN_EPS),
            nn.Linear(dim, 4 * dim),
            _GELU(),
            nn.Linear(4 * dim, dim),
            _Permute([0, 3, 1, 2]),
        )
        self.layer_scale = nn.Parameter(torch.ones(dim, 1, 1) * 1e-6)

    def branch(self, x):
        return self.layer_scale * self.block(x)

    def forward(self, x):
        return x + self.branch(x)         # stochastic depth is the identity in eval


class ConvNeXtTiny(nn.Module):
    """features / avgpool / classifier as torchvision registers them; 28 589 128 parameters, 182 state_dict keys."""

    def __init__(self):
        super().__init__()
        layers = [nn.Sequential(nn.Conv2d(3, DIMS[0], kernel_size=4, stride=4, bias=True), LayerNorm2d(DIMS[0], eps=LN_EPS))]
        for i, (c, d) in enumerate(zip(DIMS, DEPTHS)):
            layers.append(nn.Sequential(*[CNBlock(c) for _ in range(d)]))
            if i < 3:
                layers.append(nn.Sequential(LayerNorm2d(c, eps=LN_EPS), nn.Conv2d(c, DIMS[i + 1], kernel_size=2, stride=2, bias=True)))
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(LayerNorm2d(DIMS[3], eps=LN_EPS), nn.Flatten(1), nn.Linear(DIMS[3], 1000))
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def forward(self, x):
        return self.classifier(self.avgpool(self.features(x)))


def truncate(model, layers):
    """The reference's in-place surgery for three `layers` entries: features[6:] dropped, stage i keeps its first layers[i]
    blocks.  Returns the model."""
    assert len(layers) == 3
    lst = list(model.features.children())[:-2]
    for k, i in enumerate((1, 3, 5)):
        lst[i] = lst[i][:layers[k]]
    model.features = nn.Sequential(*lst)
    return model


def trunk(layers):
    return truncate(ConvNeXtTiny(), layers)


def forward_maps(model, x):
    """Outputs of features[1], [3], [5] (the reference's forward_convnext taps)."""
    out = []
    for i, layer in enumerate(model.features.children()):
        x = layer(x)
        if i in (1, 3, 5):
            out.append(x)
    return out


def randomize_convnext(module, seed):
    """Weights under which every block moves its input and GELU sees both signs (the default initialisation makes every block
    the identity to 1e-6).  Drawn from numpy's default_rng in module order, so a fixture is reproducible."""
    rng = np.random.default_rng(seed)

    def put(p, a):
        with torch.no_grad():
            p.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(p.dtype).reshape(p.shape))

    def normal(p, std):
        put(p, rng.standard_normal(tuple(p.shape)) * std)

    for m in module.modules():
        if isinstance(m, CNBlock):
            c = m.layer_scale.shape[0]
            put(m.layer_scale, rng.uniform(0.3, 1.2, (c, 1, 1)) * rng.choice([-1.0, 1.0], (c, 1, 1)))
            normal(m.block[0].weight, 1.0 / 7.0)
            normal(m.block[3].weight, 1.0 / math.sqrt(c))
            normal(m.block[5].weight, 1.0 / math.sqrt(4 * c))
            for k in (0, 3, 5):
                normal(m.block[k].bias, 0.2)
        elif isinstance(m, nn.LayerNorm):            # LayerNorm2d included
            put(m.weight, 0.5 + rng.uniform(0.0, 1.0, tuple(m.weight.shape)))
            normal(m.bias, 0.2)
    for m in module.modules():                       # stem / downsample convs: variance-preserving weights
        if isinstance(m, nn.Conv2d) and m.groups == 1:
            normal(m.weight, 1.0 / math.sqrt(m.in_channels * m.kernel_size[0] * m.kernel_size[1]))
            normal(m.bias, 0.2)
    return module


def seeded_trunk(layers, seed, dtype=torch.float64):
    """The FULL model randomised, then truncated (the order the reference applies: pretrained weights, then surgery)."""
    return truncate(randomize_convnext(ConvNeXtTiny(), seed), layers).to(dtype).eval()


def seeded_input(shape, seed, dtype=torch.float32):
    """Standard-normal values that are exact in fp32, from numpy's default_rng."""
    return torch.from_numpy(np.random.default_rng(100 + seed).standard_normal(shape).astype(np.float32)).to(dtype)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def rel_max(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


@torch.no_grad()
def check_weights_are_felt(model, x):
    """The precondition of every parity test, on the reference alone (fp64): every block moves its input by rel_l2 >= 0.3 and
    between 20 % and 80 % of each block's GELU inputs are negative."""
    x = x.double()
    for layer in model.features.children():
        if isinstance(layer[0], CNBlock):
            for blk in layer:
                pre = blk.block[3](blk.block[2](blk.block[1](blk.block[0](x))))
                neg = float((pre < 0).double().mean())
                assert 0.2 <= neg <= 0.8, f"GELU inputs negative: {neg:.3f}"
                y = blk(x)
                assert rel_l2(y, x) >= 0.3, f"a block moves its input by only {rel_l2(y, x):.3g}"
                x = y
        else:
            x = layer(x)
