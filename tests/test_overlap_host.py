"""FEM map --trim-overlap / --trim-overlap-min / --trim-overlap-err on the host: the usage lines, every refusal of the command line
(before anything is loaded), and the symbols the library exports.  No GPU."""
import ctypes

import pytest

from fem_amd import device
from tests.harness import run_fem


def _map(*extra, env=None, read2=True):
    pair = ("--read2", "r2.fq") if read2 else ()
    return run_fem("map", "-e", "3", "--ref", "a.fa", "--index", "a.idx", "--read1", "r.fq", *pair, "-o", "o.sam", *extra, env=env, text=True)


def test_usage_lists_the_three_switches():
    err = run_fem("map", "-h", text=True).stderr
    lines = err.splitlines()
    at = [i for i, l in enumerate(lines) if "--trim-overlap" in l]
    assert len(at) == 3 and at == list(range(at[0], at[0] + 3)) and "--adapter-err INT" in lines[at[0] - 1]  # beside the adapter's
    assert "--trim-overlap " in lines[at[0]] and "--read2" in lines[at[0]] and "soft clips" in lines[at[0]] and "no adapter" in lines[at[0]]
    assert "--trim-overlap-min INT" in lines[at[1]] and "(8-1024) [20]" in lines[at[1]]
    assert "--trim-overlap-err INT" in lines[at[2]] and "(0-30) [10]" in lines[at[2]]


MIN, ERR = "Wrong overlap of the mates (8-1024).", "Wrong overlap error percentage (0-30)."
NEED = "--trim-overlap-min and --trim-overlap-err need --trim-overlap."


@pytest.mark.parametrize("extra,read2,msg", [
    (["--trim-overlap"], False, "--trim-overlap needs read pairs (--read2)."),
    (["--trim-overlap", "--trim-overlap-min", "12"], False, "--trim-overlap needs read pairs (--read2)."),
    (["--trim-overlap-min", "20"], True, NEED),
    (["--trim-overlap-err", "10"], True, NEED),
    (["--trim-overlap-min", "20", "--trim-overlap-err", "10"], False, NEED),
    (["--trim-overlap", "--trim-overlap-min", "7"], True, MIN),
    (["--trim-overlap", "--trim-overlap-min", "1025"], True, MIN),
    (["--trim-overlap", "--trim-overlap-min", "0"], True, MIN),
    (["--trim-overlap", "--trim-overlap-min", "-20"], True, MIN),
    (["--trim-overlap", "--trim-overlap-min", "x"], True, MIN),
    (["--trim-overlap", "--trim-overlap-min", "20b"], True, MIN),
    (["--trim-overlap", "--trim-overlap-min", ""], True, MIN),
    (["--trim-overlap", "--trim-overlap-err", "31"], True, ERR),
    (["--trim-overlap", "--trim-overlap-err", "-1"], True, ERR),
    (["--trim-overlap", "--trim-overlap-err", "5%"], True, ERR),
    (["--trim-overlap", "--trim-overlap-err", "ten"], True, ERR),
])
def test_values_out_of_range_are_refused(extra, read2, msg):
    r = _map(*extra, read2=read2)
    assert r.returncode == 1 and r.stderr.splitlines()[0] == msg and "Loaded index" not in r.stderr


@pytest.mark.parametrize("var", ["FEM_HOST_QUALS", "FEM_HOST_TAIL", "FEM_HOST_FORMAT"])
def test_host_side_output_is_refused_before_anything_is_loaded(var):
    r = _map("--trim-overlap", env={var: "1"})
    assert r.returncode == 1
    assert r.stderr.splitlines()[0].startswith("--trim-overlap is not supported with %s=1" % var)
    assert "Loaded index" not in r.stderr and "sequence" not in r.stderr


@pytest.mark.parametrize("extra", [
    ["--trim-overlap"],
    ["--trim-overlap", "--trim-overlap-min", "8", "--trim-overlap-err", "0"],
    ["--trim-overlap", "--trim-overlap-min", "1024", "--trim-overlap-err", "30"],
    ["--trim-overlap-err", "5", "--trim-overlap"],
    ["--trim-overlap", "--adapter", "AGATCGGAAGAGC", "--adapter2", "AGATCGGAAGAGC", "--trim-qual", "20", "--trim5", "1"],
    ["--trim-overlap", "--orientation", "rf", "--infer-insert=256", "--rescue", "6", "--mate-tags"],
])
def test_values_in_range_pass_the_argument_check(extra):
    r = _map(*extra)  # the next thing to fail is the reference file
    assert r.returncode != 0 and "Wrong" not in r.stderr and "not supported" not in r.stderr and "need" not in r.stderr


def test_the_library_exports_the_three_calls():
    lib = ctypes.CDLL(device.hip_library_path())
    for name in ("fem_dev_set_pair_overlap", "fem_dev_fetch_pair_overlap", "fem_dev_pair_overlap_count"):
        assert name in device.ABI_SYMBOLS and hasattr(lib, name)
    assert all(hasattr(device.Device, f) for f in ("set_pair_overlap", "fetch_pair_overlap", "pair_overlap_count"))
    assert ctypes.sizeof(device._PairOverlapParams) == 8
    assert ctypes.sizeof(device._AdapterParams) == 24
