"""The rule of fem_dev_set_xa (tests/xa_model.py) on hand-written and on random synthetic SAM texts.  No GPU, no library."""
import numpy as np
import pytest

from tests import xa_model as m


def line(q, flag, rname=b"chr1", pos=101, cigar=b"100M", nm=0, md=b"100", tags=(), seq=True, mate=(b"*", b"0", b"0"), mapq=b"255"):
    primary = seq and not flag & 0x100
    f = [q, b"%d" % flag, rname, b"%d" % pos, mapq, cigar, mate[0], mate[1], mate[2], b"ACGT" if primary else b"*", b"IIII" if primary else b"*",
         b"NM:i:%d" % nm, b"MD:Z:" + md] + list(tags)
    return b"\t".join(f)


def text_of(lines):
    return b"".join(l + b"\n" for l in lines)


def slot(q, c, rname=b"chr2", pos0=5000, first_flag=0):
    """A slot of c lines: the primary one on chr1, secondary line t on `rname` at pos0 + t, alternating strands."""
    out = [line(q, first_flag)]
    for t in range(1, c):
        out.append(line(q, first_flag | 0x100 | (16 if t % 2 else 0), rname, pos0 + t, b"60M1D40M", t % 4, b"60^A40"))
    return out


def test_the_example_of_the_rule():
    off = text_of([line(b"r1", 0), line(b"r1", 272, b"chr2", 5001, b"60M1D40M", 1, b"60^A40"), line(b"r1", 256, b"chr1", 9001, b"100M", 2, b"7C12T79")])
    on, n = m.apply(off, m.ALL)
    assert n == 2 and on == line(b"r1", 0) + b"\tXA:Z:chr2,-5001,60M1D40M,1;chr1,+9001,100M,2;\n"
    assert m.entries(on.splitlines()[0]) == [(b"chr2", b"-", b"5001", b"60M1D40M", b"1"), (b"chr1", b"+", b"9001", b"100M", b"2")]
    assert m.unfold(on) == [m.columns(l) for l in off.splitlines()[1:]]


@pytest.mark.parametrize("N", [1, 2, m.ALL])
def test_slot_sizes_around_the_entry_limit(N):
    n_eff = 5 if N == m.ALL else N
    sizes = [1, 2, n_eff, n_eff + 1, n_eff + 2]
    lines = []
    for i, c in enumerate(sizes):
        lines += slot(b"r%d" % i, c)
    off = text_of(lines)
    on, n = m.apply(off, N)
    got = m.slots(on)
    assert len(got) == len(sizes)
    total = 0
    for c, before, after in zip(sizes, m.slots(off), got):
        f = min(c - 1, N)
        total += f
        assert len(after) == c - f
        assert len(m.entries(after[0])) == f
        assert after[1:] == before[1 + f:]  # the leftover secondary lines, unchanged
        if f:
            assert after[0].startswith(before[0] + b"\tXA:Z:") and after[0][len(before[0]) + 6:] == b"".join(m.entry(l) for l in before[1:1 + f])
        else:
            assert after[0] == before[0]
    assert n == total


def _budget_slot(sizes):
    """A slot whose entries have these byte counts, by synthetic long RNAMEs."""
    lines = [line(b"b", 0)]
    for n in sizes:
        lines.append(line(b"b", 256, b"n" * (n - len(b",+7,100M,0;")), 7))
        assert len(m.entry(lines[-1])) == n
    return lines


def test_budget_exactly_reached_and_passed_by_one():
    exact = _budget_slot([1024] * 7 + [1000, 24])
    on, n = m.apply(text_of(exact), m.ALL)
    assert n == 9 and len(on.splitlines()) == 1 and len(m.xa_of(on.splitlines()[0])) == 8192  # all fold
    over = _budget_slot([1024] * 7 + [1000, 25])
    on, n = m.apply(text_of(over), m.ALL)
    got = on.splitlines()
    assert n == 8 and got[1:] == over[-1:]  # the last stays a line
    assert len(m.xa_of(got[0])) + len(m.entry(over[-1])) == 8193
    assert m.budget_stops(text_of(over)) and not m.budget_stops(text_of(exact))


def test_an_entry_over_the_budget_never_folds():
    lines = [line(b"g", 0), line(b"g", 256, b"n" * 8193, 7), line(b"g", 256, b"chr2", 9)]
    off = text_of(lines)
    assert m.apply(off, m.ALL) == (off, 0)  # the folded lines are a prefix: nothing behind the giant folds either


def test_star_cigar_two_digit_nm_and_pos_digits():
    lines = [line(b"s", 16), line(b"s", 0x110, b"chr2", 9, b"*", 12, b""), line(b"s", 0x100, b"chr2", 10, b"100M", 3, b"1A2"),
             line(b"s", 0x100, b"chrX", 999_999_999, b"100M", 0), line(b"s", 0x110, b"chrX", 1_000_000_000, b"100M", 10)]
    on, n = m.apply(text_of(lines), m.ALL)
    assert n == 4
    assert m.xa_of(on.splitlines()[0]) == b"chr2,-9,*,12;chr2,+10,100M,3;chrX,+999999999,100M,0;chrX,-1000000000,100M,10;"
    assert [len(m.entry(l)) for l in lines[1:]] == [13, 16, 23, 25]  # (name + digits + CIGAR + digits + 5)


def test_paired_flags_adjacent_slots_and_the_strand_sign():
    m1 = [line(b"p", 0x63, mate=(b"=", b"300", b"299")),                       # mate 1 forward, its mate reverse (0x20)
          line(b"p", 0x141 | 0x20, b"chr2", 50, nm=1, mate=(b"chr1", b"300", b"0")),  # secondary, forward, 0x20 set: '+'
          line(b"p", 0x141 | 0x10, b"chr2", 70, nm=2, mate=(b"chr1", b"300", b"0"))]  # secondary, reverse: '-'
    m2 = [line(b"p", 0x93, pos=300, mate=(b"=", b"101", b"-299")),
          line(b"p", 0x181 | 0x10, b"chr3", 80, nm=0, mate=(b"chr1", b"101", b"0"))]
    on, n = m.apply(text_of(m1 + m2), m.ALL)
    got = on.splitlines()
    assert n == 3 and len(got) == 2
    assert m.xa_of(got[0]) == b"chr2,+50,100M,1;chr2,-70,100M,2;" and m.xa_of(got[1]) == b"chr3,-80,100M,0;"
    assert got[0].startswith(m1[0]) and got[1].startswith(m2[0])
    on1, n1 = m.apply(text_of(m1 + m2), 1)
    assert n1 == 2 and on1.splitlines()[1] == m1[2]  # mate 1's second secondary line stays, in front of mate 2's slot


def test_unmapped_lines_between_slots_and_a_placed_mate():
    unm = b"\t".join([b"u", b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0", b"ACGT", b"IIII"])
    placed = b"\t".join([b"w", b"133", b"chr1", b"101", b"0", b"*", b"=", b"101", b"0", b"ACGT", b"IIII", b"RG:Z:g"])
    a = slot(b"a", 3)
    w = [line(b"w", 0x49, mate=(b"=", b"101", b"0")), line(b"w", 0x149, b"chr2", 40, nm=1, mate=(b"chr1", b"101", b"0"))]
    z = slot(b"z", 2)
    off = text_of(a + [unm] + w + [placed] + z)
    on, n = m.apply(off, m.ALL)
    got = on.splitlines()
    assert n == 4 and len(got) == 5
    assert got[1] == unm and got[3] == placed  # slots of one line: as they are
    assert m.xa_of(got[0]) and m.xa_of(got[2]) == b"chr2,+40,100M,1;" and m.xa_of(got[4])


def test_xa_goes_behind_the_tags_already_there():
    tags = (b"NH:i:2", b"HI:i:1", b"RG:Z:grp", b"MC:Z:100M", b"MQ:i:255", b"ms:i:3120")
    sec = (b"NH:i:2", b"HI:i:2", b"RG:Z:grp", b"MC:Z:100M", b"MQ:i:255", b"ms:i:3120")
    off = text_of([line(b"t", 0x63, tags=tags, mate=(b"=", b"300", b"299")), line(b"t", 0x163, b"chr2", 77, nm=3, tags=sec, mate=(b"chr1", b"300", b"0"))])
    on, n = m.apply(off, m.ALL)
    f = on.splitlines()[0].split(b"\t")
    assert n == 1 and f[-2] == b"ms:i:3120" and f[-1] == b"XA:Z:chr2,+77,100M,3;"
    assert m.tag(on.splitlines()[0], b"NH:i") == b"2"  # a line keeps the numbers it has


def _random_text(rng):
    lines = []
    for i in range(int(rng.integers(5, 40))):
        c = int(rng.choice([1, 1, 2, 3, 5, 33, 70]))
        paired = bool(rng.random() < 0.5)
        base = (1 | (0x40 if rng.random() < 0.5 else 0x80)) if paired else 0
        q = b"q%d" % i
        if rng.random() < 0.15:
            lines.append(b"\t".join([q, b"%d" % (base | 4), b"*", b"0", b"0", b"*", b"*", b"0", b"0", b"ACGT", b"IIII"]))
            continue
        tags = (b"NH:i:%d" % c, b"HI:i:1") if rng.random() < 0.5 else ()
        lines.append(line(q, base | (16 if rng.random() < 0.5 else 0), pos=int(rng.integers(1, 10 ** 6)), tags=tags))
        for t in range(1, c):
            star = rng.random() < 0.1
            tags_t = (tags[0], b"HI:i:%d" % (t + 1)) if tags else ()
            lines.append(line(q, base | 0x100 | (16 if rng.random() < 0.5 else 0) | (0x20 if rng.random() < 0.3 else 0),
                              b"chr%d%s" % (int(rng.integers(0, 5)), b"x" * int(rng.integers(0, 300))), int(rng.integers(1, 2 ** 31 - 1)),
                              b"*" if star else b"%dM2I%dM" % (int(rng.integers(1, 60)), int(rng.integers(1, 60))), int(rng.integers(0, 16)),
                              b"" if star else b"50", tags=tags_t))
    return lines


@pytest.mark.parametrize("seed", range(8))
def test_properties_on_random_texts(seed):
    rng = np.random.default_rng(660 + seed)
    lines = _random_text(rng)
    off = text_of(lines)
    assert m.apply(off, 0) == (off, 0)  # N = 0 is the identity
    for N in (1, 3, 40, m.ALL):
        on, n = m.apply(off, N)
        got = on.splitlines()
        # every input line is unchanged, or unchanged plus one appended field, or exactly one entry: walk both texts
        k, gone = 0, []
        for l in lines:
            if k < len(got) and got[k] == l:
                k += 1
            elif k < len(got) and got[k].startswith(l + b"\tXA:Z:") and got[k].count(b"\t") == l.count(b"\t") + 1:
                assert not m.flag_of(l) & 0x100
                k += 1
            else:
                assert m.flag_of(l) & 0x100
                gone.append(l)
        assert k == len(got) and len(gone) == n
        assert m.unfold(on) == [m.columns(l) for l in gone]  # the removed lines' columns, in order
        assert all(len(m.xa_of(l) or b"") <= m.MAX_BYTES and len(m.entries(l)) <= N for l in got)
        # a slot folds a prefix of its secondary lines, and stops only for the limit or the budget
        for before, after in zip(m.slots(off), m.slots(on)):
            f = len(m.entries(after[0]))
            assert after[1:] == before[1 + f:]
            if f < min(len(before) - 1, N):
                assert len(m.xa_of(after[0]) or b"") + len(m.entry(before[1 + f])) > m.MAX_BYTES
