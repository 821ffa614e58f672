"""`python3 bench.py --gpus N` starts its own ranks: the launcher's environment, line relay and exit
code, on CPU with a gloo stand-in rank program; bench.py's strict WORLD_SIZE check."""
import io
import json
import os
import subprocess
import sys

from agplace_amd import launcher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "tests", "helpers", "rank_script.py")


def test_launcher_relays_rank0_line_and_returns_zero():
    out = io.StringIO()
    rc = launcher.launch_ranks(SCRIPT, ["--gpus", "2"], 2, out=out)
    assert rc == 0
    # (gloo announces its connections on stdout; RCCL does not)
    lines = [ln for ln in out.getvalue().splitlines() if ln.strip() and not ln.startswith("[Gloo]")]
    assert len(lines) == 1, lines                       # only rank 0's stdout is relayed
    rec = json.loads(lines[0])
    assert rec == {"world": 2, "allreduce_ones": 2.0, "local": 0}


def test_launcher_returns_worst_child_exit_code():
    out = io.StringIO()
    rc = launcher.launch_ranks(SCRIPT, ["--gpus", "2", "--fail-rank", "1", "--rc", "7"], 2, out=out)
    assert rc == 7
    assert json.loads([ln for ln in out.getvalue().splitlines() if ln.startswith("{")][0])["world"] == 2   # rank 0's line got out


def test_launcher_terminates_survivors_of_a_dead_rank():
    # rank 1 dies before the rendezvous (bad argument): rank 0 would wait for it forever; the launcher ends it
    out = io.StringIO()
    env = dict(os.environ)
    rc = launcher.launch_ranks(SCRIPT, ["--gpus", "3"], 2, env=env, out=out, grace_s=2.0)   # world 2 != --gpus 3: assertion
    assert rc != 0


def test_bench_refuses_a_world_size_that_differs_from_gpus():
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 2, (p.returncode, p.stderr[-500:])
    assert "WORLD_SIZE=3" in p.stderr and p.stdout.strip() == ""


def test_bench_parent_of_a_multi_rank_run_never_initialises_the_gpu():
    """No GPU here: the child ranks fail their `needs a GPU` assertion; the parent must come back with their failure
    code instead of hanging, and must not print a line of its own."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["AGP_DIST_BACKEND"] = "gloo"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env,
                       capture_output=True, text=True, timeout=600)
    import torch
    if not torch.cuda.is_available():
        assert p.returncode not in (0, 2), (p.returncode, p.stderr[-800:])
        assert "needs a GPU" in p.stderr
        assert not any(ln.startswith("{") for ln in p.stdout.splitlines())


def test_bench_plain_run_is_one_window_and_dumps_float32_within_the_limit(tmp_path, monkeypatch):
    """A plain line times exactly --steps steps (one window; --full keeps five); --dump-outputs writes float32 .npy files and, above
    the limit, the same seeded rows of every array."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7"])
    a = bench.parse()
    assert (a.steps, a.windows, a.full, a.dump_outputs) == (7, 1, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", str(tmp_path)])
    assert bench.parse().windows == 5
    q, d = torch.randn(64, 8).half(), torch.randn(64, 8)
    bench.dump_outputs(str(tmp_path / "all"), {"q": q, "d": d})
    got = np.load(tmp_path / "all" / "q.npy")
    assert got.dtype == np.float32 and np.array_equal(got, q.float().numpy())
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 * 8 * 4)          # room for half of the rows
    for run in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / run), {"q": d, "d": d})
    s = [np.load(tmp_path / run / f"{n}.npy") for run in ("s1", "s2") for n in ("q", "d")]
    assert s[0].shape == (32, 8) and all(np.array_equal(s[0], x) for x in s[1:])
    assert all(any(np.array_equal(r, x) for x in d.numpy()) for r in s[0])
