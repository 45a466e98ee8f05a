"""FEM map --xa: its usage line and its refusals, each before anything is loaded; the two functions in the header and the binding.
No GPU."""
import pytest

from tests import cases
from tests.harness import run_fem

BASE = ("map", "--ref", "a", "--index", "b", "--read1", "c", "-o", "d")


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def test_usage_lists_the_switch():
    r = run_fem("map", "-h")
    assert r.returncode == 0 and b"--xa" in r.stderr and b"XA:Z" in r.stderr


@pytest.mark.parametrize("arg", ["--xa=0", "--xa=x", "--xa=1000001", "--xa=-3", "--xa=12x"])
def test_refused_value(arg):
    r = run_fem(*(BASE + (arg,)))
    assert r.returncode == 1 and b"Wrong number of --xa entries (1-1000000)." in r.stderr and b"Loaded index" not in r.stderr


@pytest.mark.parametrize("arg", ["--xa", "--xa=1", "--xa=1000000"])
def test_accepted_value(arg):
    r = run_fem(*(BASE + (arg,)))  # (the run then ends at the reference file that is not there)
    assert b"--xa" not in r.stderr.split(b"Usage")[0] and b"Usage" not in r.stderr


@pytest.mark.parametrize("var", ["FEM_HOST_TAIL", "FEM_HOST_FORMAT"])
def test_refused_with_host_text(var):
    r = run_fem(*(BASE + ("--xa",)), env={var: "1"})
    assert r.returncode == 1 and (b"--xa is not supported with %s=1" % var.encode()) in r.stderr
    assert b"Loaded index" not in r.stderr
    # without the switch the variable is none of its business
    r = run_fem(*BASE, env={var: "1"})
    assert b"--xa" not in r.stderr.split(b"Usage")[0]


def test_served_with_the_qualities_on_the_host():
    r = run_fem(*(BASE + ("--xa",)), env={"FEM_HOST_QUALS": "1"})
    assert b"--xa" not in r.stderr.split(b"Usage")[0] and b"not supported" not in r.stderr


def test_the_functions_are_declared_and_bound():
    from fem_amd.device import ABI_SYMBOLS
    for name in ("fem_dev_set_xa", "fem_dev_xa_count"):
        assert name in cases.declared_symbols() and name in ABI_SYMBOLS
