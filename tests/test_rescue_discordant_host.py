"""FEM map --rescue-discordant, the parts that need no GPU: the usage text, the refusal, the ABI's new symbols."""

import pytest

from tests.harness import run_fem


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def run(*args):
    return run_fem(*args, text=True)


def test_usage_lists_rescue_discordant():
    assert "--rescue-discordant" in run("map", "-h").stderr


@pytest.mark.parametrize("extra", [["--rescue-discordant"], ["--read2", "r2.fq", "--rescue-discordant"]])
def test_rescue_discordant_needs_rescue(tmp_path, extra):
    args = ["map", "-e", "3", "--ref", str(tmp_path / "x.fa"), "--index", str(tmp_path / "x.idx"), "--read1", str(tmp_path / "r1.fq"),
            "-o", str(tmp_path / "o.sam")] + [str(tmp_path / a) if a == "r2.fq" else a for a in extra]
    r = run(*args)
    assert r.returncode == 1 and "--rescue-discordant needs --rescue." in r.stderr


def test_with_rescue_the_switch_is_accepted(tmp_path):
    # (the next refusal is the missing reference: the option itself passed)
    r = run("map", "-e", "3", "--ref", str(tmp_path / "x.fa"), "--index", str(tmp_path / "x.idx"), "--read1", str(tmp_path / "r1.fq"),
            "--read2", str(tmp_path / "r2.fq"), "--rescue", "8", "--rescue-discordant", "-o", str(tmp_path / "o.sam"))
    assert r.returncode != 0 and "--rescue-discordant needs" not in r.stderr and "Usage" not in r.stderr.split("\n")[0]


def test_the_library_exports_the_new_symbols():
    from fem_amd.device import ABI_SYMBOLS
    from tests.cases import declared_symbols
    assert {"fem_dev_set_rescue_discordant", "fem_dev_rescue_discordant_count"} <= set(ABI_SYMBOLS) & set(declared_symbols())
