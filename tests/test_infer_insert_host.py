"""FEM map --infer-insert, the parts that need no GPU: the usage text, the refusals (given before any file is opened), the ABI's
new symbol."""
import os

import pytest

from tests.harness import ROOT, run_fem


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def run(*args):
    return run_fem(*args, text=True)


def _map(tmp_path, *extra, read2=True):
    # (none of these files exists: a refusal that comes all the same was given before anything was opened)
    args = ["map", "-e", "3", "--ref", str(tmp_path / "x.fa"), "--index", str(tmp_path / "x.idx"), "--read1", str(tmp_path / "r1.fq"),
            "-o", str(tmp_path / "o.sam")]
    if read2:
        args += ["--read2", str(tmp_path / "r2.fq")]
    return run(*(args + list(extra)))


def test_usage_lists_infer_insert():
    assert "--infer-insert[=INT]" in run("map", "-h").stderr


@pytest.mark.parametrize("switch", ["--infer-insert", "--infer-insert=1000"])
def test_infer_insert_needs_read_pairs(tmp_path, switch):
    r = _map(tmp_path, switch, read2=False)
    assert r.returncode == 1 and r.stderr.splitlines()[0] == "--infer-insert needs read pairs (--read2)."
    assert not (tmp_path / "o.sam").exists()


@pytest.mark.parametrize("n", ["63", "262145", "0", "-5", "many", "128x", ""])
def test_wrong_number_of_pairs(tmp_path, n):
    r = _map(tmp_path, "--infer-insert=" + n)
    assert r.returncode == 1 and r.stderr.splitlines()[0] == "Wrong number of pairs to infer from (64-262144)."
    assert not (tmp_path / "o.sam").exists()


@pytest.mark.parametrize("switch", ["--infer-insert", "--infer-insert=64", "--infer-insert=262144"])
def test_the_switch_is_accepted(tmp_path, switch):
    # (the next refusal is the missing reference: the option itself passed)
    r = _map(tmp_path, switch)
    first = r.stderr.splitlines()[0] if r.stderr else ""
    assert r.returncode != 0 and "infer" not in first and "Usage" not in first


def test_the_insert_range_is_still_checked(tmp_path):
    r = _map(tmp_path, "-I", "600", "-X", "500", "--infer-insert")
    assert r.returncode == 1 and r.stderr.splitlines()[0] == "Wrong insert size range."


def test_the_library_exports_the_new_symbol():
    from fem_amd.device import ABI_SYMBOLS
    from tests.cases import declared_symbols
    assert "fem_dev_estimate_insert" in set(ABI_SYMBOLS) & set(declared_symbols())
    hdr = open(os.path.join(ROOT, "include", "fem_hip.h")).read()
    assert "#define FEM_INSERT_MAX 16383" in hdr and "#define FEM_INSERT_MIN_PAIRS 64" in hdr
