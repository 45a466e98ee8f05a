"""The drop-in command line (fem_amd/csrc/FEM): argument handling without a GPU, end-to-end `index` + `map` with one."""
import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import util
from tests.cases import expected_sam, write_case
from tests.harness import run_fem


def test_usage_and_argument_errors():
    import __graft_entry__ as g
    g.build()
    r = run_fem()
    assert r.returncode == 1 and b"Usage:   FEM <command>" in r.stderr           # src/FEM.c:24-28
    r = run_fem("frobnicate")
    assert r.returncode == 1 and b"unrecognized command" in r.stderr               # src/FEM.c:37-39
    r = run_fem("index", "12", "3")
    assert r.returncode == 1 and b"Usage: FEM index <window_size> <step_size> <reference> <output>" in r.stderr
    # k = 16 is refused from the arguments alone: before the reference is read and before a device is opened
    for k in ("16", "0"):
        r = run_fem("index", k, "3", "/nonexistent/ref.fa", "/nonexistent/out.idx")
        assert r.returncode == 1 and b"window_size must be 1..15 and step_size >= 1." in r.stderr
        assert b"Usage: FEM index" in r.stderr and b"fem_dev_open" not in r.stderr
    r = run_fem("map", "-h")
    assert r.returncode == 0 and b"--read1" in r.stderr                            # src/FEM_map.c:123-125
    r = run_fem("map", "-e", "9", "--ref", "a", "--index", "b", "--read1", "c", "-o", "d")
    assert r.returncode == 1 and b"Wrong error threshold." in r.stderr             # src/FEM_map.c:30-33
    r = run_fem("map", "-e", "3", "--index", "b", "--read1", "c", "-o", "d")
    assert r.returncode == 1 and b"Reference file path is required." in r.stderr
    r = run_fem("map", "-a", "3", "--ref", "a", "--index", "b", "--read1", "c", "-o", "d")
    assert r.returncode == 1 and b"Wrong number of additional q-grams." in r.stderr
    r = run_fem("map", "-f", "x")
    assert r.returncode == 1 and b"Wrong name of seeding algorithm!" in r.stderr   # src/FEM_map.c:113-117


@pytest.mark.gpu
@pytest.mark.parametrize("e,L,gz,batch", [(3, 100, False, 97), (7, 150, True, 1000000)])
def test_index_and_map_end_to_end(tmp_path, e, L, gz, batch):
    seqs, names, reads, rnames, quals, fa, fq = write_case(tmp_path, 77 + e, e, L, 600, gz)
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    want = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e)
    index_path, sam_path, oracle_index = str(tmp_path / "ref.idx"), str(tmp_path / "out.sam"), str(tmp_path / "o.idx")
    r = run_fem("index", "12", "3", fa, index_path)
    assert r.returncode == 0, r.stderr.decode()
    idx.save(oracle_index)
    assert open(index_path, "rb").read() == open(oracle_index, "rb").read()  # byte-identical index file
    r = run_fem("map", "-e", str(e), "-t", "3", "--ref", fa, "--index", index_path, "--read1", fq, "-o", sam_path,
            "--batch", str(batch))
    assert r.returncode == 0, r.stderr.decode()
    text = open(sam_path).read()
    header = "".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(s)) for n, s in zip(names, seqs))
    assert text.startswith(header)
    assert text[len(header):] == expected_sam(names, reads, rnames, quals, want)
    # the same run with the ordering / traceback / MD done by libfemhost instead of the device
    host_sam = str(tmp_path / "host.sam")
    r2 = run_fem("map", "-e", str(e), "-t", "3", "--ref", fa, "--index", index_path, "--read1", fq, "-o", host_sam,
             "--batch", str(batch), env={"FEM_HOST_TAIL": "1"})
    assert r2.returncode == 0, r2.stderr.decode()
    assert open(host_sam).read() == text
    # ... with the records from the device and the text spliced by the host threads between the fields of the input file's
    # mapping (the default renders the text on the device), and with those fields copied by the parser instead of read in place
    # ... and with the device's text but the qualities kept on the host (the default from 24 threads on), packed and as characters
    for env in ({"FEM_HOST_FORMAT": "1"}, {"FEM_HOST_FORMAT": "1", "FEM_SPLICE": "0"}, {"FEM_PACK_BASES": "0"}, {"FEM_HOST_QUALS": "1"},
                {"FEM_HOST_QUALS": "1", "FEM_PACK_BASES": "0"}):
        r3 = run_fem("map", "-e", str(e), "-t", "3", "--ref", fa, "--index", index_path, "--read1", fq, "-o", host_sam,
                 "--batch", str(batch), env=env)
        assert r3.returncode == 0, r3.stderr.decode()
        assert open(host_sam).read() == text, env
    err = r.stderr.decode()
    for label, v in zip(["The number of read", "The number of mapped read",
                         "The number of candidate before additional q-gram filter", "The number of candidate",
                         "The number of mapping"], want.stats):
        assert "%s: %d\n" % (label, int(v)) in err  # src/FEM_map.c:214-218


@pytest.mark.gpu
def test_map_fails_loudly_on_missing_or_truncated_reads(tmp_path):
    # the reference exits with EXIT_FAILURE in both cases (src/sequence_batch.c:33-35, 63-66): no statistics, no "Time:"
    seqs, names, reads, rnames, quals, fa, fq = write_case(tmp_path, 5, 3, 100, 300, False)
    index_path = str(tmp_path / "ref.idx")
    assert run_fem("index", "12", "3", fa, index_path).returncode == 0
    r = run_fem("map", "-e", "3", "-t", "2", "--ref", fa, "--index", index_path, "--read1", str(tmp_path / "nope.fq"), "-o",
            str(tmp_path / "a.sam"))
    assert r.returncode != 0 and b"Cannot find sequence file!" in r.stderr and b"Time:" not in r.stderr
    data = open(fq, "rb").read()
    cut = tmp_path / "cut.fq"
    cut.write_bytes(data[:len(data) - 37])  # ends inside a quality line
    r = run_fem("map", "-e", "3", "-t", "2", "--ref", fa, "--index", index_path, "--read1", str(cut), "-o", str(tmp_path / "b.sam"),
            "--batch", "50")
    assert r.returncode != 0 and b"Didn't reach the end of sequence file" in r.stderr and b"Time:" not in r.stderr
    r = run_fem("map", "-e", "3", "-t", "2", "--ref", fa, "--index", index_path, "--read1", fq, "-o", "/nonexistent_dir/x.sam")
    assert r.returncode != 0 and b"Cannot open output file" in r.stderr
    r = run_fem("map", "-e", "3", "-t", "2", "--ref", fa, "--index", index_path, "--read1", fq, "-o", "/dev/full")
    assert r.returncode != 0 and b"write error" in r.stderr


def _n_gpus():
    import torch
    return torch.cuda.device_count()  # (does not initialise the GPU)


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [True, False])
def test_map_on_several_gpus_gives_the_same_records_and_counters(tmp_path, shared):
    # src/FEM_map.c:200-212: the mapping threads' counters are summed at the end; here one RCCL all-reduce over the GPUs.
    # shared: three workers with a handle each on GPU 0 (FEM_TEST_SHARE_GPU=1) — the `--gpus N` pipeline (one thread per
    # handle, batches dealt to whichever has a free slot) on a one-GPU box; not shared: two real GPUs + RCCL
    if not shared and _n_gpus() < 2:
        pytest.skip("needs two GPUs")
    seqs, names, reads, rnames, quals, fa, fq = write_case(tmp_path, 21, 3, 100, 900, False)
    index_path = str(tmp_path / "ref.idx")
    assert run_fem("index", "12", "3", fa, index_path).returncode == 0
    outs = []
    for gpus in ("1", "3" if shared else "2"):
        sam = str(tmp_path / ("g%s.sam" % gpus))
        r = run_fem("map", "-e", "3", "-t", "4", "--gpus", gpus, "--ref", fa, "--index", index_path, "--read1", fq, "-o", sam,
                "--batch", "120", env={"FEM_TEST_SHARE_GPU": "1"} if shared else None)
        assert r.returncode == 0, r.stderr.decode()
        counters = [l for l in r.stderr.decode().splitlines() if l.startswith("The number of")]
        outs.append((sorted(open(sam).read().splitlines()), counters))
    assert outs[0] == outs[1]


@pytest.mark.gpu
def test_allreduce_stats_over_two_handles():
    if _n_gpus() < 2:
        pytest.skip("needs two GPUs")
    import ctypes as C
    from fem_amd import Device
    from fem_amd.device import load_hip
    a, b = Device(0), Device(1)
    L = load_hip()
    hs = (C.c_void_p * 2)(a._h, b._h)
    for rep in range(2):  # the second call reuses the communicator
        st = np.array([[1, 2, 3, 4, 5], [10, 20, 30, 40, 2 ** 40 + rep]], dtype=np.uint64)
        assert L.fem_dev_allreduce_stats(hs, 2, st.ctypes.data) == 0
        assert np.array_equal(st[0], st[1]) and st[0].tolist() == [11, 22, 33, 44, 2 ** 40 + rep + 5]
    a.close()
    b.close()


@pytest.mark.gpu
def test_allreduce_stats_over_one_handle_runs_rccl():
    # fem_dev_allreduce_stats with a single handle: the communicator is created (ncclCommInitAll over one device) and the
    # reduction runs over RCCL on a one-GPU box; the second and third call reuse the communicator
    import ctypes as C
    from fem_amd import Device
    from fem_amd.device import load_hip
    a = Device(0)
    L = load_hip()
    hs = (C.c_void_p * 1)(a._h)
    for rep in range(3):
        st = np.array([[7, 8, 9, 2 ** 41 + rep, 11]], dtype=np.uint64)
        assert L.fem_dev_allreduce_stats(hs, 1, st.ctypes.data) == 0
        assert st[0].tolist() == [7, 8, 9, 2 ** 41 + rep, 11]
    a.close()


@pytest.mark.gpu
def test_map_regrows_its_staging_for_unusual_records(tmp_path):
    # very long read names and short reads: a FASTQ window holds far more name bytes than the staging buffers were sized
    # for (fem_main.cc: kRegrow), with the text rendered on the device and on the host
    rng = np.random.default_rng(8)
    seqs = [util.rand_seq(rng, 120_000)]
    reads = util.make_reads(rng, seqs, 700, 64, 1)
    rnames = ["read_%d_%s" % (i, "x" * (250 + i % 90)) for i in range(len(reads))]
    quals = ["".join(chr(40 + (i + j) % 30) for j in range(64)) for i in range(len(reads))]
    fa, fq = tmp_path / "r.fa", tmp_path / "r.fq"
    fa.write_bytes(b">chrL\n" + seqs[0] + b"\n")
    with open(fq, "wb") as f:
        for n, r, q in zip(rnames, reads, quals):
            f.write(b"@" + n.encode() + b"\n" + r + b"\n+\n" + q.encode() + b"\n")
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    want = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=1)
    ix = str(tmp_path / "r.idx")
    assert run_fem("index", "12", "3", str(fa), ix).returncode == 0
    exp = "@SQ\tSN:chrL\tLN:%d\n" % len(seqs[0]) + expected_sam(["chrL"], reads, rnames, quals, want)
    for env in (None, {"FEM_HOST_FORMAT": "1"}, {"FEM_HOST_FORMAT": "1", "FEM_SPLICE": "0"}, {"FEM_PACK_BASES": "0"}, {"FEM_HOST_QUALS": "1"}):
        out = str(tmp_path / "o.sam")
        r = run_fem("map", "-e", "1", "-t", "4", "--ref", str(fa), "--index", ix, "--read1", str(fq), "-o", out, "--batch", "200", env=env)
        assert r.returncode == 0, r.stderr.decode()
        assert open(out).read() == exp
    assert want.stats[1] > 300


# ---- FEM map's argument checks, message by message: which refusal comes first, from the command line and the environment alone ----

_NO = "/nonexistent/"
_REQ = {"--ref": _NO + "a.fa", "--index": _NO + "a.idx", "--read1": _NO + "r.fq", "-o": _NO + "o.sam"}
_R2 = ["--read2", _NO + "r2.fq"]
_COV = ["--coverage", _NO + "c.bed"]
_DEV_TEXT = ", with its SAM text or BAM."
_DEV_QUAL = ", with the qualities there."
_PASSED = "Cannot find sequence file!"  # every argument check passed: the reference file is the first thing opened
_HOST_ROWS = [  # the options the host-side paths refuse, in the order they are looked at: arguments, message, refused by FEM_HOST_QUALS=1 too
    (["--bam"], "--bam is not supported with %s=1: BAM records are made on the device" + _DEV_QUAL, True),
    (_R2 + ["--mate-tags"], "--mate-tags is not supported with %s=1: the mate tags are made on the device" + _DEV_QUAL, True),
    (["--sam-seq"], "--sam-seq is not supported with %s=1: SEQ and QUAL are turned on the device" + _DEV_QUAL, True),
    (["--trim3", "2"], "--trim5, --trim3 and --trim-qual are not supported with %s=1: the reads are trimmed and their soft clips written on the device" + _DEV_QUAL, True),
    (["--adapter", "ACGTAC"], "--adapter is not supported with %s=1: the adapter is cut and the soft clips written on the device" + _DEV_QUAL, True),
    (_R2 + ["--trim-overlap"], "--trim-overlap is not supported with %s=1: the mates are cut and the soft clips written on the device" + _DEV_QUAL, True),
    (["--mapq"], "--mapq is not supported with %s=1: mapping qualities are made on the device" + _DEV_TEXT, False),
    (["--unmapped"], "--unmapped is not supported with %s=1: the lines of unmapped reads are made on the device" + _DEV_TEXT, False),
    (["--nh"], "--rg and --nh are not supported with %s=1: the tags are made on the device" + _DEV_TEXT, False),
    (["--xa"], "--xa is not supported with %s=1: the secondary lines are folded on the device" + _DEV_TEXT, False),
    (_COV, "--coverage is not supported with %s=1: the coverage track is summed on the device, from the lines of its SAM text or BAM.", False),
    (["--max-hits", "3"], "--strata and --max-hits are not supported with %s=1: the lines are filtered on the device" + _DEV_TEXT, False),
]
_TAIL, _FORMAT, _QUALS = {"FEM_HOST_TAIL": "1"}, {"FEM_HOST_FORMAT": "1"}, {"FEM_HOST_QUALS": "1"}
_REFUSALS = [  # (arguments, required arguments left out, environment, the first line on stderr)
    # refusals that nothing else pins
    (["-t", "0"], (), None, "Wrong number of threads."),
    (["--mate-tags"], (), None, "--mate-tags needs --read2."),
    (["--coverage-window", "5"], (), None, "--coverage-window, --coverage-all and --coverage-mapq need --coverage."),
    (_COV + ["--coverage-window", "0"], (), None, "Wrong coverage window (1-1000000)."),
    (_COV + ["--coverage-mapq", "61", "--mapq"], (), None, "Wrong coverage MAPQ threshold (1-60)."),
    (_COV + ["--coverage-mapq", "5"], (), None, "--coverage-mapq needs --mapq."),
    ([], ("--index",), None, "Index file path is required."),
    ([], ("--read1",), None, "Read file path is required."),
    ([], ("-o",), None, "Output file path is required."),
    (["--gpus", "0"], (), None, "Wrong number of GPUs."),
    (["--gpus", "65"], (), None, "Wrong number of GPUs."),
    (["--batch", "0"], (), None, "Wrong batch size."),
    # two faults each: the check that stands earlier in the chain speaks
    (["--mate-tags", "--trim5", "2000"], (), None, "--mate-tags needs --read2."),
    (["--trim5", "2000", "--gpus", "99"], (), None, "Wrong number of bases to trim (0-1024)."),
    (["--strata", "x", "--max-hits", "0"], (), None, "Wrong number of strata (0-15)."),
    (["-e", "9", "-t", "0"], (), None, "Wrong error threshold."),
    (["-t", "0", "-a", "3"], (), None, "Wrong number of threads."),
    (["-a", "3", "-I", "5", "-X", "2"], (), None, "Wrong number of additional q-grams."),
    (["-I", "5", "-X", "2", "--infer-insert"], (), None, "Wrong insert size range."),
    (["--infer-insert", "--orientation", "xx"], (), None, "--infer-insert needs read pairs (--read2)."),
    (_R2 + ["--infer-insert=5", "--orientation", "xx"], (), None, "Wrong number of pairs to infer from (64-262144)."),
    (["--orientation", "xx", "--mate-tags"], (), None, "Wrong library orientation (fr, rf, ff or auto)."),
    (["--orientation", "rf", "--mate-tags"], (), None, "--orientation needs read pairs (--read2)."),
    (_R2 + ["--orientation", "auto", "--rescue-discordant"], (), None, "--orientation auto needs --infer-insert."),
    (["--rescue-discordant", "--bam=5"], (), None, "--rescue-discordant needs --rescue."),
    (["--rescue", "3", "--rescue-discordant", "--bam=5"], (), None, "--rescue needs read pairs (--read2)."),
    (_R2 + ["--rescue", "16", "-X", "100000"], (), None, "Wrong rescue error threshold (0-15)."),
    (_R2 + ["--rescue", "3", "-X", "100000", "--bam=5"], (), None, "--rescue searches insert size ranges of at most 65536."),
    (["--bam=5", "--strata", "16"], (), None, "Wrong BAM compression level (0-1)."),
    (["--max-hits", "0", "--xa=0"], (), None, "Wrong hit limit (>= 1)."),
    (["--xa=0", "--trim3", "2000"], (), None, "Wrong number of --xa entries (1-1000000)."),
    (["--trim3", "2000", "--trim-qual", "0"], (), None, "Wrong number of bases to trim (0-1024)."),
    (["--trim-qual", "0", "--adapter2", "ACGT"], (), None, "Wrong trimming quality (1-93)."),
    (["--adapter-err", "5", "--adapter", "AC"], (), None, "Wrong adapter sequence (4-64 letters of ACGT)."),
    (["--adapter2", "ACGT", "--trim-overlap-min", "9"], (), None, "--adapter2, --adapter-overlap and --adapter-err need --adapter."),
    (["--adapter", "AC", "--adapter2", "ACGT"], (), None, "--adapter2 needs --read2."),
    (["--adapter", "ACGTAC", "--adapter-overlap", "7", "--adapter-err", "31"], (), None, "Wrong adapter overlap (1 to the adapter's length)."),
    (["--adapter", "ACGTAC", "--adapter-err", "31", "--trim-overlap-min", "9"], (), None, "Wrong adapter error percentage (0-30)."),
    (["--trim-overlap-min", "9", "--coverage-all"], (), None, "--trim-overlap-min and --trim-overlap-err need --trim-overlap."),
    (["--trim-overlap", "--trim-overlap-min", "2"], (), None, "--trim-overlap needs read pairs (--read2)."),
    (_R2 + ["--trim-overlap", "--trim-overlap-min", "2", "--trim-overlap-err", "40"], (), None, "Wrong overlap of the mates (8-1024)."),
    (_R2 + ["--trim-overlap", "--trim-overlap-err", "40", "--coverage-all"], (), None, "Wrong overlap error percentage (0-30)."),
    (["--coverage-all", "--gpus", "0"], (), None, "--coverage-window, --coverage-all and --coverage-mapq need --coverage."),
    (_COV + ["--coverage-window", "0", "--coverage-mapq", "99"], (), None, "Wrong coverage window (1-1000000)."),
    (_COV + ["--coverage-mapq", "99"], (), None, "Wrong coverage MAPQ threshold (1-60)."),
    (_COV + ["--coverage-mapq", "5"], ("--ref",), None, "--coverage-mapq needs --mapq."),
    ([], ("--ref", "--index"), None, "Reference file path is required."),
    ([], ("--index", "--read1"), None, "Index file path is required."),
    ([], ("--read1", "-o"), None, "Read file path is required."),
    (["--gpus", "0"], ("-o",), None, "Output file path is required."),
    (["--gpus", "0", "--batch", "0"], (), None, "Wrong number of GPUs."),
    (["--rg", "bogus", "-e", "9"], (), None, "Wrong --rg line: the read group line does not begin with @RG and a tab."),
    (["-e", "9"], (), _FORMAT, "Wrong error threshold."),  # (the argument checks stand in front of the environment's)
    # a value that is no number: the option's own range message
    (_COV + ["--coverage-window", "x"], (), None, "Wrong coverage window (1-1000000)."),
    (_COV + ["--mapq", "--coverage-mapq", "x"], (), None, "Wrong coverage MAPQ threshold (1-60)."),
    (["--strata", "x"], (), None, "Wrong number of strata (0-15)."),
    (["--max-hits", "x"], (), None, "Wrong hit limit (>= 1)."),
    (["--xa=x"], (), None, "Wrong number of --xa entries (1-1000000)."),
    (_R2 + ["--rescue", "x"], (), None, "Wrong rescue error threshold (0-15)."),
    (_R2 + ["--infer-insert=x"], (), None, "Wrong number of pairs to infer from (64-262144)."),
    (["--trim5", "x"], (), None, "Wrong number of bases to trim (0-1024)."),
    (["--trim3", "2x"], (), None, "Wrong number of bases to trim (0-1024)."),
    (["--trim-qual", "x"], (), None, "Wrong trimming quality (1-93)."),
    (["--adapter", "ACGTAC", "--adapter-overlap", "x"], (), None, "Wrong adapter overlap (1 to the adapter's length)."),
    (["--adapter", "ACGTAC", "--adapter-err", "x"], (), None, "Wrong adapter error percentage (0-30)."),
    (_R2 + ["--trim-overlap", "--trim-overlap-min", "x"], (), None, "Wrong overlap of the mates (8-1024)."),
    (_R2 + ["--trim-overlap", "--trim-overlap-err", "x"], (), None, "Wrong overlap error percentage (0-30)."),
    # the host-side paths: the first option in the table's order speaks, of the first variable that is set
    (["--unmapped", "--mapq"], (), dict(_TAIL, **_FORMAT), _HOST_ROWS[6][1] % "FEM_HOST_TAIL"),
    (["--xa", "--strata", "1", "--bam"], (), _FORMAT, _HOST_ROWS[0][1] % "FEM_HOST_FORMAT"),
    (["--coverage-all", "--sam-seq"] + _COV, (), dict(_FORMAT, **_QUALS), _HOST_ROWS[2][1] % "FEM_HOST_FORMAT"),
    (["--max-hits", "3", "--xa", "--nh"], (), _TAIL, _HOST_ROWS[8][1] % "FEM_HOST_TAIL"),
    (["--rg", "@RG\\tID:x"], (), _FORMAT, _HOST_ROWS[8][1] % "FEM_HOST_FORMAT"),
    (["--strata", "1"], (), _TAIL, _HOST_ROWS[11][1] % "FEM_HOST_TAIL"),
    (["--trim-qual", "20", "--adapter", "ACGTAC"], (), _QUALS, _HOST_ROWS[3][1] % "FEM_HOST_QUALS"),
    (_R2 + ["--trim-overlap", "--adapter", "ACGTAC", "--mapq"], (), _TAIL, _HOST_ROWS[4][1] % "FEM_HOST_TAIL"),
    (_R2, (), _FORMAT, _PASSED),  # (--read2 on the host-side paths is refused behind the reference and the index, not here)
]
# ... and every row of it: refused under FEM_HOST_FORMAT=1; under FEM_HOST_QUALS=1 refused where the qualities are needed on the
# device, and served (the argument checks passed) where they are not
_REFUSALS += [(args, (), _FORMAT, msg % "FEM_HOST_FORMAT") for args, msg, _ in _HOST_ROWS if "--read2" not in args]
_REFUSALS += [(args, (), _QUALS, msg % "FEM_HOST_QUALS" if quals else _PASSED) for args, msg, quals in _HOST_ROWS]


@pytest.mark.parametrize("args,without,env,first_line", _REFUSALS)
def test_map_refusals_in_order(args, without, env, first_line):
    required = [w for k, v in _REQ.items() if k not in without for w in (k, v)]
    # (FEM_NUMA_BIND=0: a command line that passes the checks asks for no device's NUMA node on its way to the reference file)
    r = run_fem("map", *required, *args, env=dict(env or {}, FEM_NUMA_BIND="0"), text=True)
    assert r.returncode == 1
    assert r.stderr.splitlines()[0] == first_line
