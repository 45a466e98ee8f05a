"""Plain-Python model of the insert size estimate (FEM map --infer-insert; fem_dev_estimate_insert in include/fem_hip.h).

Input: the single-end records of a batch of 2 n reads, pair i being read i (mate 1) and read n + i (mate 2), in the form
fo.map_reads returns them (tests/pair_model.py).  Output: the ten fields of fem_insert_estimate.  Integers throughout."""
from tests import pair_model as pm

INSERT_MAX = 16383     # FEM_INSERT_MAX
INSERT_MIN_PAIRS = 64  # FEM_INSERT_MIN_PAIRS

FIELDS = ("n_pairs", "n_unique", "n_informative", "q25", "q50", "q75", "min_insert", "max_insert", "estimated")


def inserts(res, n_pairs):
    """(unique pairs, the informative inserts in pair order)."""
    n_unique, out = 0, []
    for i in range(n_pairs):
        a0, a1 = int(res.rec_off[i]), int(res.rec_off[i + 1])
        b0, b1 = int(res.rec_off[n_pairs + i]), int(res.rec_off[n_pairs + i + 1])
        if a1 - a0 != 1 or b1 - b0 != 1 or (int(res.r_flag[a0]) | int(res.r_flag[b0])) & 0x8000:
            continue
        n_unique += 1
        ins = pm.insert_of(res, a0, b0, 0, INSERT_MAX)  # the pairing rule's own statement, the slot's range playing no part
        if ins is not None:
            out.append(ins)
    return n_unique, out


def from_inserts(n_pairs, n_unique, ins):
    """The estimate's fields (dict) from the informative inserts."""
    v = sorted(ins)
    n = len(v)
    q25, q50, q75 = (v[(n - 1) // 4], v[2 * (n - 1) // 4], v[3 * (n - 1) // 4]) if n else (-1, -1, -1)
    iqr = q75 - q25
    est = n >= INSERT_MIN_PAIRS
    return dict(n_pairs=n_pairs, n_unique=n_unique, n_informative=n, q25=q25, q50=q50, q75=q75,
                min_insert=max(0, q25 - 3 * iqr) if est else 0, max_insert=q75 + 3 * iqr if est else 0, estimated=int(est))


def estimate(res, n_pairs):
    n_unique, ins = inserts(res, n_pairs)
    return from_inserts(n_pairs, n_unique, ins)


def as_tuple(est):
    return tuple(int(est[f]) for f in FIELDS)
