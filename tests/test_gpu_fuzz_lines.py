"""A bounded slice of tests/fuzz_lines.py under `pytest -m gpu`: fixed seeds, twelve trials each, of the output-line options drawn
together (pairing with I and X anywhere, an insert on either bound, mate rescue, --rescue-discordant, MAPQ, the unmapped reads'
lines, --strata / --max-hits, RG / NH / HI, the orientation FR / RF / FF with the reads turned to match, --mate-tags, --sam-seq,
--xa with its entry limit on a slot's size and its byte budget met exactly under long reference names, the refusal of host
qualities, estimate_insert / estimate_library before the text or behind the BAM, BAM, staging, slot, one trial through
FEM index + FEM map; and in the cuts, cuts-pairs, coverage and cuts-command-line cases the cut stage in front of all that, the
fixed trims, the quality rule, the adapters and the mates' overlap on reads that only a cut makes mappable, with the clip points,
every producer's cuts and counters, the refusals of a trimmed batch's staging and the coverage track after every fetch, doubled
by a second mapping, and the BED file of the command line) against the composed models: pair_kernel, pair_probe_kernel, mapq_kernel, report_kernel, the rescue
kernels, xa_index_kernel / xa_write_kernel, the trim stage (adapter_match_kernel, pair_overlap_kernel, trim_clip_kernel,
trim_gather_kernel), clip_count_kernel / clip_write_kernel, coverage_kernel and the option branches of the sam_* / bam_* kernels (fem_tail.hip), and the
LineOptions plumbing of fem_hip.hip, one handle per case.  What the slice reaches, and that it would see an off-by-one or a
strand read from the wrong world, is held without a GPU by tests/test_fuzz_lines_model.py.

Wall time per case on the MI355X (the models on the host take most of it): single-end-heavy 1.4 s, copies-80 1.4 s, e-7 1.2 s,
command-line 1.7 s, long-names 1.3 s, xa-deep (200 copies: slots of more than 64 and more than 128 lines) 1.4 s, cuts 1.8 s,
cuts-pairs 1.8 s, coverage 1.6 s, cuts-command-line 2.5 s (its command-line trial with --trim3, --trim-qual and the --coverage track
under --coverage-mapq, over several batches)."""
import pytest

from tests import fuzz_lines

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,seed,trials,force,cli", fuzz_lines.SLICE, ids=[c[0] for c in fuzz_lines.SLICE])
def test_fuzz_slice(name, seed, trials, force, cli):
    lines = []
    n, bad = fuzz_lines.run(seed, trials=trials, force=force, cli_trials=cli, log=lambda *a: lines.append(" ".join(str(x) for x in a)))
    assert n == trials and bad == 0, "\n".join(lines)
