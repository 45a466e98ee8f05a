"""Read pairs for --rescue-discordant (tests/discordant_model.py): pairs whose records do not pair, because one mate maps
exactly at a decoy copy of its segment while its true place beside the other mate is more than e edits away."""
import numpy as np

from tests import util


def _fit(rng, s, ln):
    return s[:ln] if len(s) >= ln else s + util.rand_seq(rng, ln - len(s))


def make_discordant_pairs(rng, main, n, L, L2, e, E, X, n_sym=6, decoy_copies=1, near_end=False, decoy_len=30_000):
    """-> (seqs, mate 1 reads, mate 2 reads).  `main`: the sequences fragments come from (the first one also takes the
    symmetric plants, so it must be random and at least 20 kbp); a decoy sequence is added behind them.
    Pair i: i % 4 in (0, 1): one mate's true segment with e + 1 .. E edits is written into the decoy sequence
    (decoy_copies times) and that text is the read; 2: plain, 0 .. e edits per mate; 3: one mate with e + 1 .. E edits and
    no decoy (kind 1).  Mates are swapped at random.  The last n_sym pairs are symmetric plants: mate 1 exact at p with
    mate 2's segment, k substitutions in it, beside it, and mate 2 exact at q with such a copy of mate 1's segment beside it."""
    main = [bytearray(s) for s in main]
    m0 = main[0]
    plants = []
    far = X + max(L, L2) + 400           # q - p: too far apart to pair as they map
    stride = far + max(L, L2) + X + 600  # from plant to plant: outside each other's windows
    assert 1_000 + n_sym * stride <= len(m0)
    for t in range(n_sym):
        p = 1_000 + stride * t
        q = p + far
        k = e + 1 + t % max(1, E - e) if E > e else 1
        a_seg, b_seg = bytes(m0[p:p + L]), bytes(m0[q:q + L2])
        for at, seg in ((p + L + 50, b_seg), (q - L - 50, a_seg)):
            c = bytearray(seg)
            for u in range(k):  # k substitutions, spread out
                x = 5 + u * ((len(c) - 10) // k)
                c[x] = ord("A") if c[x] != ord("A") else ord("C")
            m0[at:at + len(c)] = c
        plants.append((bytes(m0[p:p + L]), util.revcomp(bytes(m0[q:q + L2]))))
    main = [bytes(s) for s in main]
    lens = np.array([len(s) for s in main], np.int64)
    ok = np.nonzero(lens > X + 200)[0]
    decoy, r1, r2 = [util.rand_seq(rng, 100)], [], []
    for i in range(n - n_sym):
        si = int(ok[rng.integers(0, len(ok))])
        frag = int(rng.integers(max(L, L2) + 20, X + 1))
        lo = 1_000 + stride * n_sym if si == 0 else 0  # (clear of the plants)
        if near_end and i % 5 == 0:
            st = int(lens[si]) - frag - int(rng.integers(0, 3))
        else:
            st = int(rng.integers(lo, lens[si] - frag))
        f = main[si][st:st + frag]
        segs = [f[:L], f[frag - L2:]]  # as they stand in the reference; mate 2 is the reverse complement of its one
        kind = i % 4
        heavy = int(rng.integers(0, 2))
        for m in (0, 1):
            k = int(rng.integers(0, e + 1))
            if kind != 2 and m == heavy and E > e:
                k = int(rng.integers(e + 1, E + 1))
            segs[m] = _fit(rng, util.mutate(rng, segs[m], k), (L, L2)[m])
        if kind < 2:
            for _ in range(decoy_copies):
                decoy += [segs[heavy], util.rand_seq(rng, 30)]
        a, b = segs[0], util.revcomp(segs[1])
        if rng.random() < 0.5:
            a, b = b, a
        r1.append(a)
        r2.append(b)
    for a, b in plants:
        r1.append(a)
        r2.append(b)
    decoy = b"".join(decoy)
    decoy += util.rand_seq(rng, max(0, decoy_len - len(decoy)) + 100)
    return main + [decoy], r1, r2


def check_fixture(kept, kinds, traced, n, min_kept=20, min_each=5):
    """What every case asserts on the model's result before the device runs: the fixture does its job."""
    k2 = {r: kept[r] for r, (kind, _) in kinds.items() if kind == 2}
    assert len(k2) >= min_kept, len(k2)
    assert sum(r < n for r in k2) >= min_each and sum(r >= n for r in k2) >= min_each
    assert any(k["rc"] for k in k2.values()) and any(not k["rc"] for k in k2.values())
    assert any(op in "ID" for k in k2.values() for _, op in k["record"][4])
    assert {kinds[r][1] for r in k2} == {0, 1}
    assert any(t.get("tie") for t in traced.values())
