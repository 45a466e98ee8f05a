"""The header forms of FEM map --header / --rg and the validator of the --rg argument (libfemhost) against tests/tags_model.py,
and FEM map's refusals.  No GPU."""
import struct

import numpy as np
import pytest

from fem_amd import host
from tests import bam_model as bm
from tests import tags_model as tm
from tests.harness import run_fem

NAMES, LENS = ["chr1", "c2_" + "n" * 70, "x"], [1000, 123456, (1 << 31) - 1]


def _ref(names=NAMES, lens=LENS):
    text = np.zeros(1 << 10, np.uint8)
    off = np.zeros(len(lens), np.uint64)
    return host.TailReference(text, off, np.array(lens, np.uint64).astype(np.uint32), names=names)


def _sq(names=NAMES, lens=LENS):
    return "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in zip(names, lens)).encode()


def test_the_old_header_functions_give_the_same_bytes():
    ref = _ref()
    assert host.sam_header(ref).encode() == _sq()
    assert host.bam_header(ref) == bm.header(_sq(), [n.encode() for n in NAMES], LENS)


@pytest.mark.parametrize("rg,pg", [(None, None), ("@RG\tID:a\tSM:b c", None), (None, "@PG\tID:FEM\tCL:FEM map"),
                                   ("@RG\tID:a", "@PG\tID:FEM\tPN:FEM\tVN:0.2\tCL:FEM map -o x")])
def test_the_new_header_forms(rg, pg):
    ref = _ref()
    want = tm.header(_sq(), None if rg is None else rg.encode(), None if pg is None else pg.encode())
    text = host.sam_header_full(ref, rg, pg).encode("latin-1")
    assert text == want
    lines = text.split(b"\n")[:-1]
    assert lines[0] == b"@HD\tVN:1.6\tSO:unsorted\tGO:query"
    assert lines[1:1 + len(NAMES)] == _sq().split(b"\n")[:-1]
    assert lines[1 + len(NAMES):] == [x.encode() for x in (rg, pg) if x is not None]  # @RG behind the last @SQ, @PG last
    # the BAM form: the same text, the same @SQ table
    raw = host.bam_header_full(ref, rg, pg)
    assert raw == bm.header(want, [n.encode() for n in NAMES], LENS)
    (l_text,) = struct.unpack_from("<i", raw, 4)
    assert raw[:4] == b"BAM\1" and raw[8:8 + l_text] == want
    assert raw[8 + l_text:] == host.bam_header(ref)[8 + len(_sq()):]


def test_the_bam_form_refuses_a_sequence_of_2_31_bases():
    with pytest.raises(ValueError):
        host.bam_header_full(_ref(["a", "big"], [10, 1 << 31]), None, None)


def test_pg_line():
    for argv in (["FEM", "map"], ["/x y/FEM", "map", "--rg", "@RG\tID:a\tSM:b", "-o", "out\nput", "--nh"], ["FEM"]):
        assert host.pg_line(argv, "0.2").encode("latin-1") == tm.pg_line(argv, "0.2")
    assert host.pg_line(["FEM", "map", "a\tb"], "9").endswith("CL:FEM map a\\tb")


def test_the_validator_accepts():
    assert host.parse_read_group("@RG\\tID:lane1\\tSM:s 1\\tPL:ILLUMINA") == ("@RG\tID:lane1\tSM:s 1\tPL:ILLUMINA", "lane1")
    assert host.parse_read_group("@RG\tSM:x\tID:a.b:c") == ("@RG\tSM:x\tID:a.b:c", "a.b:c")
    assert host.parse_read_group("@RG\tID:a\\tDS:mixed \\n stays") == ("@RG\tID:a\tDS:mixed \\n stays", "a")  # no other escape is read
    long_id = "i" * 255
    assert host.parse_read_group("@RG\tID:" + long_id)[1] == long_id
    line, ident = host.parse_read_group("@RG\\tID:x\\tX1:~ ")
    assert line.encode() == tm.rg_line("@RG\\tID:x\\tX1:~ ") and ident == "x"


@pytest.mark.parametrize("arg,why", [
    ("RG\\tID:x", "does not begin with @RG"),
    ("@RG ID:x", "does not begin with @RG"),
    ("@RG", "does not begin with @RG"),
    ("@RG\tID:x\tsample", "is not TAG:VALUE"),
    ("@RG\tID:x\t1D:y", "is not TAG:VALUE"),
    ("@RG\tID:x\tSM:", "is not TAG:VALUE"),
    ("@RG\tID:x\tSM:caf\xe9", "is not TAG:VALUE"),
    ("@RG\tID:x\t", "is not TAG:VALUE"),
    ("@RG\tID:x\tSM:a\tSM:b", "tag SM occurs twice"),
    ("@RG\tID:x\tID:y", "tag ID occurs twice"),
    ("@RG\tSM:a", "has no ID"),
    ("@RG\tID:" + "i" * 256, "longer than 255 bytes"),
    ("@RG\tID:x\nSM:y", "contains a newline"),
    ("@RG\tID:x\tSM:y\n", "contains a newline"),
])
def test_the_validator_refuses(arg, why):
    with pytest.raises(ValueError, match=why):
        host.parse_read_group(arg)


def test_cli_usage_and_refusals():
    import __graft_entry__ as g
    g.build()
    r = run_fem("map", "-h")
    assert r.returncode == 0 and all(x in r.stderr for x in (b"--header", b"--rg", b"--nh"))
    r = run_fem("map", "--rg", "RG\\tID:x")
    assert r.returncode != 0 and b"does not begin with @RG" in r.stderr
    base = ("map", "--ref", "a", "--index", "b", "--read1", "c", "-o", "d")
    for arg, why in (("@RG\\tSM:x", b"has no ID"), ("@RG\\tID:x\\tID:y", b"tag ID occurs twice"), ("@RG\tID:x\ny", b"contains a newline")):
        r = run_fem(*(base + ("--rg", arg)))
        assert r.returncode != 0 and why in r.stderr and b"Loaded index" not in r.stderr
    for var in ("FEM_HOST_TAIL", "FEM_HOST_FORMAT"):
        for sw in (("--rg", "@RG\\tID:x"), ("--nh",)):
            r = run_fem(*(base + sw), env={var: "1"})
            assert r.returncode == 1 and (b"--rg and --nh are not supported with %s=1" % var.encode()) in r.stderr, (var, sw)
            assert b"Loaded index" not in r.stderr
        # --header alone is host text: not refused (the run then ends at the reference file that is not there)
        r = run_fem(*(base + ("--header",)), env={var: "1"})
        assert b"not supported" not in r.stderr
