"""FEM map --trim5 / --trim3 / --trim-qual on the host: the usage lines, every refusal of the command line (before anything is
loaded), and the symbols the library exports.  No GPU."""
import ctypes

import pytest

from fem_amd import device
from tests.harness import run_fem


def _map(*extra, env=None):
    return run_fem("map", "-e", "3", "--ref", "a.fa", "--index", "a.idx", "--read1", "r.fq", "-o", "o.sam", *extra, env=env, text=True)


def test_usage_lists_the_three_switches():
    err = run_fem("map", "-h", text=True).stderr
    assert "--trim5 INT" in err and "--trim3 INT" in err and "--trim-qual INT" in err
    assert "(0-1024)" in err and "(1-93)" in err and "keeping 35 bases at the least" in err and "soft clips" in err


@pytest.mark.parametrize("extra,msg", [
    (["--trim5", "1025"], "Wrong number of bases to trim (0-1024)."),
    (["--trim5", "-1"], "Wrong number of bases to trim (0-1024)."),
    (["--trim3", "1025"], "Wrong number of bases to trim (0-1024)."),
    (["--trim3", "x"], "Wrong number of bases to trim (0-1024)."),
    (["--trim5", "3", "--trim3", "7x"], "Wrong number of bases to trim (0-1024)."),
    (["--trim-qual", "0"], "Wrong trimming quality (1-93)."),
    (["--trim-qual", "94"], "Wrong trimming quality (1-93)."),
    (["--trim-qual", "-3"], "Wrong trimming quality (1-93)."),
    (["--trim-qual", "q"], "Wrong trimming quality (1-93)."),
])
def test_values_out_of_range_are_refused(extra, msg):
    r = _map(*extra)
    assert r.returncode == 1 and r.stderr.splitlines()[0] == msg and "Loaded index" not in r.stderr


@pytest.mark.parametrize("switch", [("--trim5", "1"), ("--trim3", "2"), ("--trim-qual", "20"), ("--trim5", "0")])
@pytest.mark.parametrize("var", ["FEM_HOST_QUALS", "FEM_HOST_TAIL", "FEM_HOST_FORMAT"])
def test_host_side_output_is_refused_before_anything_is_loaded(var, switch):
    r = _map(*switch, env={var: "1"})
    assert r.returncode == 1
    assert r.stderr.splitlines()[0].startswith("--trim5, --trim3 and --trim-qual are not supported with %s=1" % var)
    assert "Loaded index" not in r.stderr and "sequence" not in r.stderr


def test_values_in_range_pass_the_argument_check():
    r = _map("--trim5", "1024", "--trim3", "0", "--trim-qual", "93")  # the next thing to fail is the reference file
    assert r.returncode != 0 and "Wrong" not in r.stderr and "not supported" not in r.stderr


def test_the_library_exports_the_three_calls():
    lib = ctypes.CDLL(device.hip_library_path())
    for name in ("fem_dev_set_trim", "fem_dev_fetch_trim", "fem_dev_trim_count"):
        assert name in device.ABI_SYMBOLS and hasattr(lib, name)
    assert all(hasattr(device.Device, f) for f in ("set_trim", "fetch_trim", "trim_count"))
    assert ctypes.sizeof(device._TrimParams) == 12
