"""FEM map --mate-tags: its usage line and its four refusals, each before anything is loaded.  No GPU."""
import pytest

from tests.harness import run_fem

BASE = ("map", "--ref", "a", "--index", "b", "--read1", "c", "-o", "d")


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def test_usage_lists_the_switch():
    r = run_fem("map", "-h")
    assert r.returncode == 0 and b"--mate-tags" in r.stderr and b"MC:Z, MQ:i and ms:i" in r.stderr


def test_refused_without_read2():
    r = run_fem(*(BASE + ("--mate-tags",)))
    assert r.returncode == 1 and b"--mate-tags needs --read2" in r.stderr and b"Loaded index" not in r.stderr


@pytest.mark.parametrize("var", ["FEM_HOST_TAIL", "FEM_HOST_FORMAT", "FEM_HOST_QUALS"])
def test_refused_with_host_text_or_host_qualities(var):
    r = run_fem(*(BASE + ("--read2", "c2", "--mate-tags")), env={var: "1"})
    assert r.returncode == 1 and (b"--mate-tags is not supported with %s=1" % var.encode()) in r.stderr
    assert b"Loaded index" not in r.stderr
    # without the switch the variable is none of its business (the run then ends at the reference file that is not there)
    r = run_fem(*(BASE + ("--read2", "c2")), env={var: "1"})
    assert b"--mate-tags" not in r.stderr.split(b"Usage")[0]
