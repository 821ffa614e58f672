"""-m gpu test: the adaptive dopri5 solver at 256 and 384 columns (csrc/fusion_adaptive.hip) gives, bit for bit, what the
build before the two forward kernels became one driver gave (tests/golden/fcode_adaptive_parent.npz, dumped on an MI355X from
that build by `python tests/test_gpu_dopri5_parity.py --dump`, which runs every case twice and refuses to write a file if the
two runs differ, or if a width has no case with a rejected step).

Cases, per width (256, 384) and activation (relu, tanh, sigmoid, id: four kernel instantiations each way): the input law at
b = 37 (three row tiles, the last one padded) and gain 4.0, add1, tol 1e-4, cap 64, with trajectory, then the backward of a
randn cotangent (seed 3).  Per width one failed solve: relu, b = 16, gain 1, tol 1e-3, cap 2 -- status 1, NaN outputs.
Stored: y, gx, gb and the control block in full, gw as the SHA-256 of its bytes (y, gx and the control block for the failed
solves).  Only ops.fcode_adaptive(..., want_traj=True) and ops.fcode_adaptive_bwd are called.

The step sequences of the dump (accepted / rejected); a case with a rejected step exercises the reject path:
    256: relu 8 / 0, tanh 4 / 0, sigmoid 3 / 0, id 7 / 1, failed 2 / 0 (status 1)
    384: relu 8 / 0, tanh 4 / 0, sigmoid 3 / 0, id 7 / 1, failed 2 / 0 (status 1)
(relu at this gain rejects a step at b = 16, seed 11 -- the LONG tables of the two dopri5 modules -- but not at b = 37; id does.)
The control block is compared by its decoded accepted and rejected counts first, then by its bytes: a failure says whether a
decision changed or only the arithmetic."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

import dopri5_ref as R
import test_gpu_dopri5_wide as wide

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fcode_adaptive_parent.npz")
INPUT_LAW = {256: R.input_law, 384: wide.input_law}
# (width, act, b, gain, tol, cap, failed)
CASES = [(d, act, 37, 4.0, 1e-4, 64, False) for d in (256, 384) for act in ("relu", "tanh", "sigmoid", "id")]
CASES += [(d, "relu", 16, 1.0, 1e-3, 2, True) for d in (256, 384)]


def _tag(case):
    return f"{case[0]}_{case[1]}" + ("_failed" if case[6] else "")


def _run(case):
    """The arrays of one case as numpy, and the solve's statistics."""
    from agplace_amd import ops
    d, act, b, gain, tol, cap, failed = case
    dev = torch.device("cuda:0")
    x, a1, w, bias = INPUT_LAW[d](b, gain)
    G = torch.randn(b, d, generator=torch.Generator().manual_seed(3)).to(dev)
    lw = ops.LinearWeights(w.to(dev), bias.to(dev), with_transpose=True)
    y, ctrl, traj = ops.fcode_adaptive(x.to(dev), lw, act, "dopri5", tol, cap, add1=a1.to(dev), want_traj=True)
    gx, gw, gb = ops.fcode_adaptive_bwd(traj, ctrl, G, lw, act, "dopri5", cap)
    out = {"y": y.cpu().numpy(), "gx": gx.cpu().numpy(), "ctrl": ctrl.cpu().numpy()}
    if not failed:
        out["gb"] = gb.cpu().numpy()
        out["gw_sha256"] = np.frombuffer(hashlib.sha256(gw.cpu().numpy().tobytes()).digest(), dtype=np.uint8)
    return out, ops.ode_stats(ctrl)


def _counts(ctrl):
    """(status, accepted, rejected) of a control block's bytes."""
    return tuple(int(v) for v in np.ascontiguousarray(ctrl[:12]).view(np.int32))


@pytest.fixture(scope="module")
def parent():
    return np.load(FIXTURE)


@pytest.mark.parametrize("case", CASES, ids=_tag)
def test_bits_equal_the_parent_build(dev, parent, case):
    got, st = _run(case)
    tag, failed = _tag(case), case[6]
    print(f"DOPRI5 PARITY {tag}: status {st['status']} accepted {st['accepted']} rejected {st['rejected']}")
    want_ctrl = parent[f"{tag}/ctrl"]
    assert _counts(got["ctrl"]) == _counts(want_ctrl), (tag, "a step decision changed", st)
    assert st["status"] == (1 if failed else 0)
    if failed:
        assert np.isnan(got["y"]).all() and np.isnan(got["gx"]).all(), tag
    assert set(got) == {k.split("/")[1] for k in parent.files if k.startswith(tag + "/")}
    for name in ("ctrl", "y", "gx", "gb", "gw_sha256"):
        if name in got:
            want = parent[f"{tag}/{name}"]
            assert got[name].dtype == want.dtype, (tag, name)
            assert np.array_equal(got[name], want, equal_nan=failed), (tag, name)      # (the same NaN by its bits below)
            assert got[name].tobytes() == want.tobytes(), (tag, name)


def _dump():
    arrays, rejecting = {}, {256: [], 384: []}
    for case in CASES:
        first, st = _run(case)
        second, _ = _run(case)
        for name in first:
            if first[name].tobytes() != second[name].tobytes():
                sys.exit(f"{_tag(case)}: two runs differ in {name}; no file written")
            arrays[f"{_tag(case)}/{name}"] = first[name]
        print(f"{_tag(case)}: status {st['status']} accepted {st['accepted']} rejected {st['rejected']}")
        if st["rejected"] and not case[6]:
            rejecting[case[0]].append(case[1])
    for d, acts in rejecting.items():
        if not acts:
            sys.exit(f"no case with a rejected step at {d} columns; no file written")
    np.savez_compressed(FIXTURE, **arrays)
    print(f"wrote {FIXTURE}: {os.path.getsize(FIXTURE)} bytes")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] != ["--dump"]:
        sys.exit("usage: test_gpu_dopri5_parity.py --dump")
    _dump()
