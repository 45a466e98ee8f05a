"""SEQ and QUAL as SAM orders them on the device (fem_dev_set_sam_seq: sam_write_kernel and bam_write_kernel, fem_tail.hip) and
FEM map --sam-seq: the same handle's text with the option off, then on, against the plain-Python rule of tests/sam_seq_model.py;
the BAM records decoded against the text; no length changes.  Needs a GPU: -m gpu."""
import numpy as np
import pytest

from fem_amd.device import FemError
from tests import bam_model as bm
from tests import cases
from tests import sam_seq_model as m
from tests.cases import I, LINE_E, LINE_RESCUE_E, MAX_HITS, RG, STRATA, X, line_options_case, make_pairs, write_fastq
from tests.harness import build_index, counters, decode_bam_file, open_device, pairing_on, run_fem, same_text, stage_and_map

pytestmark = pytest.mark.gpu


def _device(c):
    return open_device(c["seqs"], c["names"], c["idx"])[0]


def _stage(dev, c, slot=0, packed=False, quals_on_host=False):
    return stage_and_map(dev, c["reads"], c["rnames"], c["quals"], c["e"], slot, quals_on_host, packed)


def _payload(dev, slot, level):
    data = dev.fetch_bam(slot=slot, level=level)
    payload = b"".join(x[0] for x in bm.parse_bgzf(data[0], eof=False)) if data[0] else b""
    assert data[1] == len(payload)
    return payload


def _off_on(dev, c, slot=0, at_least=20):
    """The staged batch's text with the option off, then on: on == the rule applied to off, the BAM records at both levels decode to
    on, nothing changes its length, and at least `at_least` lines were turned -> (off, on)."""
    names = [x.encode() for x in c["names"]]
    dev.set_sam_seq(False, slot=slot)
    off = dev.fetch_sam(slot=slot)[0]
    bam_off = _payload(dev, slot, 0)
    assert bm.bam_payload_to_sam(bam_off, names) == off
    dev.set_sam_seq(True, slot=slot)
    on = dev.fetch_sam(slot=slot)[0]
    same_text(on, m.apply(off))
    assert len(on) == len(off)
    for level in (0, 1):
        payload = _payload(dev, slot, level)
        same_text(bm.bam_payload_to_sam(payload, names), on)
        assert len(payload) == len(bam_off)
    assert dev.fetch_sam(slot=slot, nowait=True)[0] == on
    assert len(m.turned(off)) >= at_least, len(m.turned(off))
    return off, on


# ---- the length ladder ----

def test_ladder_as_characters():
    c = m.ladder_case()
    dev = _device(c)
    try:
        _stage(dev, c)
        off, on = _off_on(dev, c, at_least=len(m.LADDER))
        seen = m.ladder_strands(on, c)
        assert all(seen.get(L) == {0, 16} for L in m.LADDER), seen  # a reverse-strand primary line of every length
        assert len(on.splitlines()) == len(c["reads"])
    finally:
        dev.close()


def test_ladder_packed_length_by_length():
    c = m.ladder_case()
    dev = _device(c)
    try:
        for L in m.LADDER:  # (the 2-bit transfer takes reads of one length: ensure_chars makes the characters)
            sub = m.sub_case(c, [i for i, r in enumerate(c["reads"]) if len(r) == L])
            _stage(dev, sub, packed=True)
            off, on = _off_on(dev, sub, at_least=1)
            assert m.ladder_strands(on, sub) == {L: {0, 16}}
    finally:
        dev.close()


# ---- letters ----

def test_letters_lower_case_and_asserted_records():
    c = m.letters_case()
    dev = _device(c)
    try:
        _stage(dev, c)
        off, on = _off_on(dev, c)
        turned = m.turned(off)
        seqs = b"".join(l.split(b"\t")[9] for l in turned)
        assert set(b"NRYKM=") <= set(seqs) and b"." not in seqs  # (the table made N of '.')
        by_name = dict(zip(c["rnames"], c["reads"]))
        lower = [l for l in turned if by_name[l.split(b"\t")[0].decode()] != by_name[l.split(b"\t")[0].decode()].upper()]
        assert len(lower) == 2 and all(l.split(b"\t")[9].isupper() for l in lower)
        starred = [l for l in turned if l.split(b"\t")[5] == b"*"]  # 0x8000 records: turned by their 0x10 bit
        assert starred and dev.fetch_sam()[2] >= len(starred)
    finally:
        dev.close()


# ---- SEQ read against CIGAR on the device's own output ----

@pytest.mark.parametrize("case", m.NM_CASES, ids=lambda c: "e%d-L%d" % (c[1], c[2]))
def test_seq_agrees_with_nm_on_every_primary_line(case):
    c = m.nm_case(*case)
    dev = _device(c)
    try:
        _stage(dev, c)
        off, on = _off_on(dev, c, at_least=100)
        fwd, fwd_ok, rev, rev_ok = m.nm_agreement(on, c["seqs"], c["names"])
        assert fwd >= 100 and rev >= 100 and (fwd_ok, rev_ok) == (fwd, rev)
        assert m.nm_agreement(off, c["seqs"], c["names"]) == (fwd, fwd, rev, 0)
    finally:
        dev.close()


# ---- pairs, every option on ----

def test_pairs_with_every_option_on():
    c = dict(line_options_case(), e=LINE_E)
    dev = _device(c)
    try:
        pairing_on(dev, I, X, LINE_RESCUE_E)
        dev.set_report(strata=STRATA, max_hits=MAX_HITS)
        dev.set_tags(read_group=RG, hits=True)
        dev.set_mate_tags(True)
        _stage(dev, c)
        off, on = _off_on(dev, c)
        assert dev.rescue_count() > 0 and dev.rescue_discordant_count() > 0 and dev.filtered_count() > 0
        assert len(m.rescued_turned(off, c)) >= 3  # rescued mates with 0x10 among the changed lines
        placed = m.placed_at_reversed(off)
        assert placed and all(not m.flag_of(l) & 16 for l in placed) and all(l in on.splitlines() for l in placed)
        changed = [a for a, b in zip(off.splitlines(), on.splitlines()) if a != b]
        assert all(m.flag_of(l) & 16 and not m.flag_of(l) & 0x104 for l in changed)
        assert [l.split(b"\t")[11:] for l in off.splitlines()] == [l.split(b"\t")[11:] for l in on.splitlines()]  # no tag changes
    finally:
        dev.close()


# ---- off again, another slot, the refusal ----

def test_off_again_a_second_slot_and_the_refusal():
    c = m.nm_case(*m.NM_CASES[0])
    dev = _device(c)
    try:
        _stage(dev, c, slot=0)
        _stage(dev, c, slot=1)
        off, on = _off_on(dev, c, slot=0)
        assert dev.fetch_sam(slot=1)[0] == off  # the other slot's option is its own
        assert _payload(dev, 1, 0) == bm.sam_to_bam_payload(off, [x.encode() for x in c["names"]])
        assert dev.fetch_sam(slot=0)[0] == on   # sticky
        _stage(dev, c, slot=0)
        assert dev.fetch_sam(slot=0)[0] == on   # ... over batches
        dev.set_sam_seq(False)
        assert dev.fetch_sam(slot=0)[0] == off
        assert _payload(dev, 0, 0) == _payload(dev, 1, 0)
        # the qualities kept on the host: refused with the option on, text and BAM; served with it off
        dev.set_sam_seq(True)
        q, offsets = _stage(dev, c, slot=0, quals_on_host=True)
        with pytest.raises(FemError, match=r"^invalid argument: SEQ and QUAL in SAM order \(fem_dev_set_sam_seq\)"):
            dev.fetch_sam(slot=0, quals=q, offsets=offsets)
        with pytest.raises(FemError, match=r"^invalid argument: SEQ and QUAL in SAM order \(fem_dev_set_sam_seq\)"):
            dev.fetch_bam(slot=0)
        dev.set_sam_seq(False)
        assert dev.fetch_sam(slot=0, quals=q, offsets=offsets)[0] == off
        rec = dev.fetch_records(slot=0)  # records carry no SEQ: the same with the option on
        dev.set_sam_seq(True)
        again = dev.fetch_records(slot=0)
        assert np.array_equal(rec.flag, again.flag) and np.array_equal(rec.pos0, again.pos0) and np.array_equal(rec.cigar, again.cigar)
    finally:
        dev.close()


# ---- a fixed slice of drawn option sets ----

def _set_options(dev, d, E):
    dev.set_pairs(I, X) if d["paired"] else dev.set_pairs(None)
    dev.set_rescue(E if d["paired"] and d["rescue"] else None)
    dev.set_rescue_discordant(bool(d["paired"] and d["rescue"] and d["discordant"]))
    dev.set_orientation(d["orientation"] if d["paired"] else 0)
    dev.set_mate_tags(bool(d["paired"] and d["mate_tags"]))
    dev.set_mapq(d["mapq"])
    dev.set_unmapped(d["unmapped"])
    dev.set_report(strata=d["strata"], max_hits=d["max_hits"])
    dev.set_tags(read_group=d["rg"], hits=d["hits"])


@pytest.mark.parametrize("k", range(len(m.DRAW_CASES)), ids=[x[0] for x in m.DRAW_CASES])
def test_drawn_option_sets(k):
    _, maker, args = m.DRAW_CASES[k]
    c = getattr(cases, maker)(*args)
    assert len(m.DRAW_CASES) * m.DRAWS_PER_CASE >= 16
    dev = _device(c)
    try:
        _stage(dev, c)
        texts = set()
        for d in m.draws(k):
            _set_options(dev, d, c.get("E") or 8)
            off, on = _off_on(dev, c)
            texts.add(off)
        assert len(texts) >= 3  # the draws differ in what they print
    finally:
        dev.close()


# ---- FEM map --sam-seq ----

@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sam_seq")
    rng = np.random.default_rng(630)
    seqs, names = cases.reference(rng, False)
    fa = tmp / "ref.fa"
    fa.write_bytes(b"".join(b">%s desc\n%s\n" % (n.encode(), s) for n, s in zip(names, seqs)))
    idx_path = str(tmp / "ref.idx")
    build_index(fa, idx_path)
    n = 400
    x1, x2 = make_pairs(rng, seqs, n, 100, 2)
    x1[3], x2[5] = x1[3].lower(), x2[5][:50] + b"RYKM=.-*" + x2[5][58:]
    rn = ["m%d" % i for i in range(n)]
    p1, p2 = tmp / "x1.fq", tmp / "x2.fq"
    write_fastq(p1, x1, rn, m.rand_quals(rng, x1), False)
    write_fastq(p2, x2, rn, m.rand_quals(rng, x2), False)
    return dict(tmp=tmp, fa=str(fa), idx=idx_path, p1=str(p1), p2=str(p2), n=n)


@pytest.mark.parametrize("threads", [16, 24])
@pytest.mark.parametrize("paired", [False, True], ids=["single", "read2"])
def test_cli(files, threads, paired):
    out = str(files["tmp"] / ("out_%d_%d" % (threads, paired)))
    common = ["-e", "2", "-t", str(threads), "--ref", files["fa"], "--index", files["idx"], "--read1", files["p1"], "--unmapped", "--mapq", "-o", out]
    if paired:
        common += ["--read2", files["p2"], "--rescue", "8", "--mate-tags"]

    def run(*args, bam=False):
        r = run_fem("map", *(common + list(args)))
        assert r.returncode == 0, r.stderr.decode()
        got = decode_bam_file(out) if bam else open(out, "rb").read()
        return b"".join(l + b"\n" for l in got.splitlines() if not l.startswith(b"@")), counters(r.stderr)

    plain, plain_counters = run()  # (at -t 24 the qualities stay on the host here, and go to the device with the switch)
    assert len(m.turned(plain)) >= 20 and plain_counters
    on, on_counters = run("--sam-seq")
    same_text(on, m.apply(plain))
    assert on_counters == plain_counters
    plain_bam, bam_counters = run("--bam", bam=True)
    assert plain_bam == plain and bam_counters == plain_counters
    on_bam, on_bam_counters = run("--bam", "--sam-seq", bam=True)
    same_text(on_bam, m.apply(plain))
    assert on_bam_counters == plain_counters
