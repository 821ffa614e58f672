"""The host-side conv dispatch (csrc/conv_dispatch.hip) against the answers recorded from the build before it was gathered there
(tests/golden/conv_dispatch_table.npz, written by tests/golden/make_conv_dispatch_table.py): every route, return code, plan and
size query of a fixed sweep of descriptors and groups, compared exactly.  Host-only: nothing is launched.  No GPU needed."""
import importlib.util
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_conv_dispatch_table", os.path.join(GOLDEN, "make_conv_dispatch_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded(gen):
    fx = np.load(os.path.join(GOLDEN, "conv_dispatch_table.npz"))
    assert tuple(fx["cols"]) == gen.COLS and len(str(fx["commit"])) == 40
    return fx["table"], fx["crc"]


@pytest.fixture(scope="module")
def rows(gen):
    return gen.sweep()


def test_recorded_table_covers_the_dispatch(gen, recorded, rows):
    """Every kernel and return code, statistics on each kernel that has them (igemm_kxr at both tile heights) and none for the
    3x3 conv the generic kernel runs, pooling granted and refused; and where the parent sized a statistics buffer, it was the
    plan's MT."""
    table, crc = recorded
    assert len(rows) == len(table) == len(crc)
    gen.check_coverage(table, [name for name, _ in rows])


def test_dispatch_answers_what_the_recorded_build_answered(gen, recorded, rows):
    from agplace_amd import _lib
    table, crc = recorded
    got, got_crc = gen.evaluate(_lib.load(), rows)
    assert np.array_equal(got_crc, crc), "the sweep no longer builds the recorded descriptors: record again"
    differ = np.nonzero((got != table).any(axis=1))[0]
    report = ["%s: %s, recorded %s" % (rows[i][0], dict(zip(gen.COLS, got[i].tolist())), dict(zip(gen.COLS, table[i].tolist())))
              for i in differ[:10]]
    assert differ.size == 0, "%d of %d rows differ\n%s" % (differ.size, len(rows), "\n".join(report))
