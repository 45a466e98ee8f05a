"""FEM map --orientation, the parts that need no GPU: the usage text, the three refusals (given before any file is opened), the
ABI's two new symbols."""
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


def test_usage_lists_orientation():
    err = run("map", "-h").stderr
    assert "--orientation STR" in err and "fr, rf or ff [fr]" in err and "auto" in err


@pytest.mark.parametrize("value", ["rr", "FR", "", "fr,rf", "0"])
def test_another_value_is_refused(tmp_path, value):
    r = _map(tmp_path, "--orientation", value, "--infer-insert")
    assert r.returncode == 1 and r.stderr.splitlines()[0] == "Wrong library orientation (fr, rf, ff or auto)."
    assert not (tmp_path / "o.sam").exists()


@pytest.mark.parametrize("value", ["fr", "rf", "ff"])
def test_orientation_needs_read_pairs(tmp_path, value):
    r = _map(tmp_path, "--orientation", value, read2=False)
    assert r.returncode == 1 and r.stderr.splitlines()[0] == "--orientation needs read pairs (--read2)."
    assert not (tmp_path / "o.sam").exists()


def test_auto_needs_infer_insert(tmp_path):
    r = _map(tmp_path, "--orientation", "auto")
    assert r.returncode == 1 and r.stderr.splitlines()[0] == "--orientation auto needs --infer-insert."
    assert "Loaded index" not in r.stderr and not (tmp_path / "o.sam").exists()


@pytest.mark.parametrize("extra", [("--orientation", "fr"), ("--orientation", "rf"), ("--orientation=ff",),
                                   ("--orientation", "auto", "--infer-insert"), ("--infer-insert=64", "--orientation=auto")])
def test_the_switch_is_accepted(tmp_path, extra):
    # (the next refusal is the missing reference: the option itself passed)
    r = _map(tmp_path, *extra)
    first = r.stderr.splitlines()[0] if r.stderr else ""
    assert r.returncode != 0 and "orientation" not in first and "Usage" not in first


def test_the_library_exports_the_new_symbols():
    from fem_amd.device import ABI_SYMBOLS, hip_library_path
    from tests.cases import declared_symbols
    import ctypes
    new = {"fem_dev_set_orientation", "fem_dev_estimate_library"}
    assert new <= set(ABI_SYMBOLS) & set(declared_symbols())
    lib = ctypes.CDLL(hip_library_path())
    assert all(hasattr(lib, s) for s in new)
    hdr = open(os.path.join(ROOT, "include", "fem_hip.h")).read()
    assert all("#define FEM_ORIENT_%s %d" % (n, v) in hdr for n, v in (("FR", 0), ("RF", 1), ("FF", 2)))
