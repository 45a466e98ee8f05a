"""A slot's output options together (fem_dev_set_pairs, _rescue, _rescue_discordant, _mapq, _unmapped, _report, _tags: one
femt::LineOptions per slot, fem_hip.hip) and its counters (one femt::LineCounts): every option on and off again on one handle
and one slot, against a fresh handle with the same options and against the Python models.  Needs a GPU: -m gpu."""
import numpy as np
import pytest

from fem_amd.device import FemError
from tests import pair_model as pm
from tests import report_model as rp
from tests import tags_model as tm
from tests.cases import I, LINE_E, LINE_RESCUE_E, MAX_HITS, RG, STRATA, X
from tests.cases import line_options_case as case
from tests.harness import fetch_sam, open_device, pairing_on

pytestmark = pytest.mark.gpu

e, E = LINE_E, LINE_RESCUE_E


def _model_text(c, strata=None, max_hits=None, tags=False):
    """(the paired text with rescue, MAPQ and the unmapped reads' lines, filtered and tagged on demand; the lines dropped)."""
    text, dropped = rp.paired(c["want"], c["n"], c["names"], c["reads"], c["rnames"], c["quals"], I, X, res=c["ext"],
                              rescued=set(c["kept"]), e=e, strata=strata, max_hits=max_hits)
    return (tm.apply(text, RG, True) if tags else text), dropped


def _device(c):
    return open_device(c["seqs"], c["names"], c["idx"])[0]


def _pairing_on(dev):
    pairing_on(dev, I, X, E)


def _all_on(dev):
    _pairing_on(dev)
    dev.set_report(strata=STRATA, max_hits=MAX_HITS)
    dev.set_tags(read_group=RG, hits=True)


def _sam(dev, c):
    return fetch_sam(dev, c["reads"], c["rnames"], c["quals"], e, 0)[0]


def _counts(dev):
    return (dev.pair_count(), dev.rescue_count(), dev.rescue_discordant_count(), dev.unmapped_count(), dev.filtered_count())


def test_all_options_on_then_off_again_is_a_fresh_handle():
    c = case()
    want_on, dropped = _model_text(c, STRATA, MAX_HITS, tags=True)
    assert dropped > 0
    dev, fresh = _device(c), _device(c)
    try:
        _all_on(dev)
        on = _sam(dev, c)
        assert on.splitlines() == want_on.splitlines()
        assert _counts(dev) == (c["n_proper"], len(c["kept"]), c["n_kind2"], c["n_unmapped"], dropped)
        bam_on = dev.fetch_bam()
        assert _counts(dev) == (c["n_proper"], len(c["kept"]), c["n_kind2"], c["n_unmapped"], dropped)
        # every option off again, each through its own setter
        dev.set_tags()
        dev.set_report()
        dev.set_unmapped(False)
        dev.set_mapq(False)
        dev.set_rescue_discordant(False)
        dev.set_rescue(None)
        dev.set_pairs(None)
        off = _sam(dev, c)
        bam_off = dev.fetch_bam()
        plain = _sam(fresh, c)
        assert off == plain and on != off
        assert bam_off[:5] == fresh.fetch_bam()[:5] and bam_on[0] != bam_off[0]
        assert dev.unmapped_count() == 0 and dev.filtered_count() == 0
        for count in (dev.pair_count, dev.rescue_count, dev.rescue_discordant_count):
            with pytest.raises(FemError, match="the slot is not in pair mode"):
                count()
    finally:
        dev.close()
        fresh.close()


def test_changed_options_take_effect_and_report_consistently():
    c = case()
    want, dropped = _model_text(c)
    assert dropped == 0
    dev, fresh = _device(c), _device(c)
    try:
        _all_on(dev)
        _sam(dev, c)
        assert dev.filtered_count() > 0
        dev.set_report()
        dev.set_tags()
        text = _sam(dev, c)
        _pairing_on(fresh)
        assert text == _sam(fresh, c) and _counts(dev) == _counts(fresh)
        assert text.splitlines() == want.splitlines()
        assert _counts(fresh) == (c["n_proper"], len(c["kept"]), c["n_kind2"], c["n_unmapped"], 0)
    finally:
        dev.close()
        fresh.close()


def test_fetch_pairs_ignores_set_mapq():
    c = case()
    dev, fresh = _device(c), _device(c)
    try:
        _pairing_on(dev)
        text = _sam(dev, c)
        with_mapq = dev.fetch_pairs()
        dev.set_mapq(False)
        without = dev.fetch_pairs()
        for k, v in vars(without).items():
            assert np.array_equal(getattr(with_mapq, k), v), k
        for k, v in pm.pair_arrays(c["ext"], c["n"], I, X).items():
            assert np.array_equal(getattr(without, k), v), k
        assert (dev.pair_count(), dev.rescue_count(), dev.rescue_discordant_count()) == (c["n_proper"], len(c["kept"]), c["n_kind2"])
        # a paired text with MAPQ behind a fetch_pairs, which paired without it
        dev.set_mapq(True)
        again = dev.fetch_sam()[0]
        _pairing_on(fresh)
        assert again == text == _sam(fresh, c)
    finally:
        dev.close()
        fresh.close()
