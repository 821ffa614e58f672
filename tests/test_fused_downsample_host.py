"""Host side of the stage entry without a stored downsample map: the eligibility refusals of agp_conv2d_s2_fwd and
agp_conv2d_fwd_grouped2 (every refusal comes before a launch, so none of this needs a GPU), the folded chunk-major downsample
plane against a numpy restatement, the not-fusable decision, and the ABI of the second-stream block."""
import ctypes

import numpy as np
import torch

from agplace_amd import _lib, ops, resnet
from conv_sched_util import desc_conv

E_UNSUPPORTED = 3


def _s2(n=2, cin=64, cout=128, **k):
    return desc_conv(cin, cout, 13, 27, n, k=3, stride=2, relu=True, **k)


def _call_s2(descs):
    arr = (_lib.ConvDesc * len(descs))(*descs)
    return _lib.load().agp_conv2d_s2_fwd(arr, len(descs), None)


def test_s2_entry_refuses_ineligible_input():
    assert _call_s2([]) == E_UNSUPPORTED                                   # n = 0
    assert _call_s2([_s2(), _s2(), _s2()]) == E_UNSUPPORTED                # more than two trunks
    assert _call_s2([desc_conv(64, 128, 13, 27, 2, k=3, stride=1)]) == E_UNSUPPORTED
    assert _call_s2([desc_conv(64, 128, 13, 27, 2, k=1, stride=2)]) == E_UNSUPPORTED
    assert _call_s2([_s2(prec=2)]) == E_UNSUPPORTED
    assert _call_s2([_s2(res=True)]) == E_UNSUPPORTED
    assert _call_s2([_s2(), _s2(cout=256)]) == E_UNSUPPORTED               # the trunks share one channel shape
    d = _s2()
    d.pout = 0
    assert _call_s2([d]) == E_UNSUPPORTED


def _k3(cin=128, cout=128, h=7, w=14, n=2, **k):
    return desc_conv(cin, cout, h, w, n, k=3, stride=1, relu=True, **k)


def _stream(n=2, hin=13, win=27, cin=64):
    t = _lib.ConvStream2()
    t.in_hi = t.w_cm = 1
    t.n, t.hin, t.win, t.cin = n, hin, win, cin
    return t


def _call_g2(descs, streams):
    arr = (_lib.ConvDesc * len(descs))(*descs)
    st = (_lib.ConvStream2 * len(descs))(*streams)
    return _lib.load().agp_conv2d_fwd_grouped2(arr, st, len(descs), None)


def test_grouped2_entry_refuses_ineligible_input():
    assert _call_g2([_k3()] * 5, [_stream()] * 5) == E_UNSUPPORTED        # more than four problems
    assert _call_g2([_k3(cout=64)], [_stream()]) == E_UNSUPPORTED         # cout % 128
    assert _call_g2([_k3(prec=2)], [_stream()]) == E_UNSUPPORTED
    assert _call_g2([desc_conv(128, 128, 7, 14, 2, k=1)], [_stream()]) == E_UNSUPPORTED
    assert _call_g2([_k3(res=True)], [_stream()]) == E_UNSUPPORTED        # a stored residual AND a computed one
    d = _k3()
    d.pool_partial = 1
    assert _call_g2([d], [_stream()]) == E_UNSUPPORTED                    # the pooling epilogue with the stream
    assert _call_g2([_k3()], [_stream(cin=48)]) == E_UNSUPPORTED          # cin2 % 32
    assert _call_g2([_k3()], [_stream(n=3)]) == E_UNSUPPORTED             # another batch
    assert _call_g2([_k3()], [_stream(hin=15)]) == E_UNSUPPORTED          # (15 - 1) / 2 + 1 = 8 rows, the conv has 7
    assert _call_g2([_k3()], [_stream(win=29)]) == E_UNSUPPORTED
    t = _stream()
    t.w_cm = None
    assert _call_g2([_k3()], [t]) == E_UNSUPPORTED
    assert _call_g2([_k3(), _k3(cin=256)], [_stream(), _stream()]) == E_UNSUPPORTED


def test_folded_plane_layout_and_values():
    g = torch.Generator().manual_seed(3)
    cout, cin = 128, 96
    w = torch.randn(cout, cin, 1, 1, generator=g)
    s = torch.randn(cout, generator=g)
    s[3], s[7] = 0.0, -2.5
    t = torch.randn(cout, generator=g)
    sw = ops.Stream2Weights(w, s, t)
    assert sw.fusable and sw.plane.dtype == torch.float16 and tuple(sw.plane.shape) == (cin // 32, cout, 32)
    wn, sn = w.numpy().reshape(cout, cin), s.numpy()
    want = np.empty((cin // 32, cout, 32), np.float16)
    for c in range(cin // 32):
        for n in range(cout):
            want[c, n] = (wn[n, 32 * c:32 * c + 32] * sn[n]).astype(np.float32).astype(np.float16)      # one rounding, from fp32
    assert np.array_equal(sw.plane.numpy().view(np.uint16), want.view(np.uint16))
    assert np.array_equal(sw.shift.numpy(), t.numpy())


def test_not_fusable_decision():
    w = torch.ones(128, 64, 1, 1)
    t = torch.zeros(128)
    assert ops.Stream2Weights(w, torch.full((128,), 65503.0), t).fusable
    for bad in (65504.0, -7.0e4, float("inf"), float("nan")):
        s = torch.ones(128)
        s[5] = bad
        sw = ops.Stream2Weights(w, s, t)
        assert not sw.fusable and sw.plane is None, bad


def test_trunk_preparation_marks_blocks():
    net = resnet.ResNet("resnet18", nstages=3).eval()
    prep, fuse = net._prepared(scaled=True), net._prepared_fuse(scaled=True)
    assert fuse[(0, 0)] is None and fuse[(1, 1)] is None        # no downsample
    for li in (1, 2):
        sw, c2f = fuse[(li, 0)]
        cws, dsw = prep[(li, 0)]
        assert sw.fusable and sw.cin == cws[0].cin and sw.cout == cws[1].cout
        assert torch.equal(c2f.shift, cws[1].shift + dsw.shift) and c2f.scale is cws[1].scale and c2f._planes is cws[1]._planes
    net.layer2[0].downsample[1].weight.data.mul_(1.0e7)
    net.layer2[0].downsample[1].weight._version    # (in-place edits through .data do not move it: drop the cache by hand)
    net._prep_key = None
    fuse = net._prepared_fuse(scaled=True)
    assert fuse[(1, 0)] is None and fuse[(2, 0)] is not None
    # 50-layer trunks (Bottleneck blocks) are untouched
    assert all(v is None for v in resnet.ResNet("resnet50", nstages=2)._prepared_fuse().values())


def test_stream2_abi():
    assert ctypes.sizeof(_lib.ConvStream2) == 2 * 8 + 4 * 4
    assert (_lib.ConvStream2.in_hi.offset, _lib.ConvStream2.w_cm.offset, _lib.ConvStream2.n.offset, _lib.ConvStream2.cin.offset) == (0, 8, 16, 28)
    import os, subprocess, tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "l.c")
        open(src, "w").write('#include <stddef.h>\n#include <stdio.h>\n#include "agplace_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n",'
                             'sizeof(agp_conv_stream2),offsetof(agp_conv_stream2,w_cm),offsetof(agp_conv_stream2,n),'
                             'offsetof(agp_conv_stream2,cin),sizeof(agp_conv_desc));return 0;}\n')
        exe = os.path.join(td, "l")
        subprocess.run(["gcc", "-I", os.path.join(root, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [32, 8, 16, 28, ctypes.sizeof(_lib.ConvDesc)]
