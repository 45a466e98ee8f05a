"""FEM map --adapter / --adapter2 / --adapter-overlap / --adapter-err on the host: the usage lines, every refusal of the command
line (before anything is loaded), and the symbols the library exports.  No GPU."""
import ctypes

import pytest

from fem_amd import device
from tests.harness import run_fem

A1 = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"


def _map(*extra, env=None, read2=False):
    pair = ("--read2", "r2.fq") if read2 else ()
    return run_fem("map", "-e", "3", "--ref", "a.fa", "--index", "a.idx", "--read1", "r.fq", *pair, "-o", "o.sam", *extra, env=env, text=True)


def test_usage_lists_the_four_switches():
    err = run_fem("map", "-h", text=True).stderr
    assert "--adapter STR" in err and "--adapter2 STR" in err and "--adapter-overlap INT" in err and "--adapter-err INT" in err
    assert "(4-64 letters of ACGT)" in err and "(0-30) [10]" in err and "[5]" in err and "soft clips" in err


SEQ, OVERLAP, ERR = "Wrong adapter sequence (4-64 letters of ACGT).", "Wrong adapter overlap (1 to the adapter's length).", "Wrong adapter error percentage (0-30)."


@pytest.mark.parametrize("extra,read2,msg", [
    (["--adapter", "ACG"], False, SEQ),
    (["--adapter", "A" * 65], False, SEQ),
    (["--adapter", "ACGTN"], False, SEQ),
    (["--adapter", "ACGU"], False, SEQ),
    (["--adapter", ""], False, SEQ),
    (["--adapter", A1, "--adapter2", "ACGTRY"], True, SEQ),
    (["--adapter", A1, "--adapter2", "AC"], True, SEQ),
    (["--adapter", A1, "--adapter-overlap", "0"], False, OVERLAP),
    (["--adapter", A1, "--adapter-overlap", "34"], False, OVERLAP),
    (["--adapter", A1, "--adapter-overlap", "x"], False, OVERLAP),
    (["--adapter", A1, "--adapter2", "ACGTAC", "--adapter-overlap", "7"], True, OVERLAP),  # the shorter of the two
    (["--adapter", A1, "--adapter-err", "31"], False, ERR),
    (["--adapter", A1, "--adapter-err", "-1"], False, ERR),
    (["--adapter", A1, "--adapter-err", "5%"], False, ERR),
    (["--adapter2", A1], True, "--adapter2, --adapter-overlap and --adapter-err need --adapter."),
    (["--adapter-overlap", "5"], False, "--adapter2, --adapter-overlap and --adapter-err need --adapter."),
    (["--adapter-err", "10"], False, "--adapter2, --adapter-overlap and --adapter-err need --adapter."),
    (["--adapter", A1, "--adapter2", A1], False, "--adapter2 needs --read2."),
])
def test_values_out_of_range_are_refused(extra, read2, msg):
    r = _map(*extra, read2=read2)
    assert r.returncode == 1 and r.stderr.splitlines()[0] == msg and "Loaded index" not in r.stderr


@pytest.mark.parametrize("var", ["FEM_HOST_QUALS", "FEM_HOST_TAIL", "FEM_HOST_FORMAT"])
def test_host_side_output_is_refused_before_anything_is_loaded(var):
    r = _map("--adapter", A1, env={var: "1"})
    assert r.returncode == 1
    assert r.stderr.splitlines()[0].startswith("--adapter is not supported with %s=1" % var)
    assert "Loaded index" not in r.stderr and "sequence" not in r.stderr


@pytest.mark.parametrize("extra,read2", [
    (["--adapter", A1], False),
    (["--adapter", A1.lower(), "--adapter-overlap", "33", "--adapter-err", "30"], False),
    (["--adapter", "ACGT", "--adapter-overlap", "4", "--adapter-err", "0"], False),
    (["--adapter", "A" * 64, "--adapter2", "ACGTAC", "--adapter-overlap", "6"], True),
    (["--adapter", A1, "--trim-qual", "20", "--trim5", "1"], False),
])
def test_values_in_range_pass_the_argument_check(extra, read2):
    r = _map(*extra, read2=read2)  # the next thing to fail is the reference file
    assert r.returncode != 0 and "Wrong" not in r.stderr and "not supported" not in r.stderr and "need" not in r.stderr


def test_the_library_exports_the_three_calls():
    lib = ctypes.CDLL(device.hip_library_path())
    for name in ("fem_dev_set_adapter", "fem_dev_fetch_adapter", "fem_dev_adapter_count"):
        assert name in device.ABI_SYMBOLS and hasattr(lib, name)
    assert all(hasattr(device.Device, f) for f in ("set_adapter", "fetch_adapter", "adapter_count"))
    assert ctypes.sizeof(device._AdapterParams) == 24
    assert ctypes.sizeof(device._TrimParams) == 12
