"""Host-side tests (no GPU) of the 384-column adaptive solver's interface: the size functions of include/agplace_hip.h and the
fragment-order planes of W^T the backward reads."""
import pytest
import torch


@pytest.fixture(scope="module")
def L():
    from agplace_amd import _lib
    return _lib.load()


def test_ring_floats_are_what_the_header_documents(L):
    for b in (1, 5, 16, 37, 64):
        for cap in (1, 2, 64):
            assert L.agp_fcode_adaptive_wide_ring_floats(b, 384, cap, 1) == (cap + 1) * 8 * b * 384
            assert L.agp_fcode_adaptive_wide_ring_floats(b, 384, cap, 0) == 2 * 8 * b * 384
    for b, cap in ((0, 64), (-3, 64), (16, 0), (16, -1)):
        assert L.agp_fcode_adaptive_wide_ring_floats(b, 384, cap, 1) == 0
        assert L.agp_fcode_adaptive_wide_ring_floats(b, 384, cap, 0) == 0
    assert L.agp_fcode_adaptive_wide_ring_floats(16, 256, 64, 1) == 0        # the one width
    # the control block is shared with the 256-column solver
    assert L.agp_fcode_adaptive_ctrl_bytes(64) == 32 + 3 * 64 * 8


def test_workspace_bytes_are_what_the_header_documents(L):
    for b in (1, 5, 16, 17, 37, 64):
        bp = (b + 15) // 16 * 16
        for cap in (1, 2, 64):
            assert L.agp_fcode_adaptive_wide_bwd_workspace_bytes(b, 384, cap) == 2 * (6 * cap + 1) * bp * 384 * 4
    for b, cap in ((0, 64), (-3, 64), (16, 0), (16, -1)):
        assert L.agp_fcode_adaptive_wide_bwd_workspace_bytes(b, 384, cap) == 0
    assert L.agp_fcode_adaptive_wide_bwd_workspace_bytes(16, 256, 64) == 0


def _host_weights(w):
    """A LinearWeights with CPU planes (its constructor splits on the GPU): hi = bf16(w), lo = bf16(w - hi), padded to 512 rows."""
    from agplace_amd import ops
    hi = w.bfloat16()
    lo = (w - hi.float()).bfloat16()
    lw = object.__new__(ops.LinearWeights)
    pad = torch.zeros(128, w.shape[1], dtype=torch.bfloat16)
    lw.w_hi, lw.w_lo = torch.cat([hi, pad]), torch.cat([lo, pad])
    lw.n, lw.k, lw.npad = w.shape[0], w.shape[1], 512
    lw.wt_hi = lw.wt_lo = lw.bias = lw._frag = lw._frag_t = None
    return lw


def test_transposed_planes_are_the_planes_of_the_transpose():
    from agplace_amd import ops
    g = torch.Generator().manual_seed(7)
    w = torch.randn(384, 384, generator=g) / 19
    lw, lwt = _host_weights(w), _host_weights(w.t().contiguous())
    got, want = ops.fcode_wide_planes_t(lw), ops.fcode_wide_planes(lwt)
    assert not torch.equal(got[0], ops.fcode_wide_planes(lw)[0])
    for p, q in zip(got, want):
        assert p.shape == q.shape == (8, 12, 3, 4, 16, 8) and p.dtype == q.dtype == torch.bfloat16 and p.is_contiguous()
        assert torch.equal(p.view(torch.int16), q.view(torch.int16))
    assert ops.fcode_wide_planes_t(lw) is got                               # cached
    # the documented entry: [wave][ks][tile][q][row][8] = W[32 ks + 8 q .. + 7][48 wave + 16 tile + row]
    for plane, src in zip(got, (lw.w_hi, lw.w_lo)):
        for wave, ks, tile, q, row in ((0, 0, 0, 0, 0), (7, 11, 2, 3, 15), (3, 5, 1, 2, 9)):
            col = src[32 * ks + 8 * q:32 * ks + 8 * q + 8, 48 * wave + 16 * tile + row].contiguous()
            assert torch.equal(plane[wave, ks, tile, q, row].view(torch.int16), col.view(torch.int16))
    with pytest.raises(NotImplementedError):
        ops.fcode_wide_planes_t(_host_weights(torch.zeros(256, 256)))
