"""Coverage windows on the MI355X: the accumulation inside the BAM pass, the GC kernel and the binning against their host twins
(BAMs from tests/bam_writer.py: both framings, tiny chunks, unsorted files, 15-kb reads with long CIGARs, placed-unmapped and
unplaced records), the selection unchanged by the flag, and `genotype --expansion` end to end: -c <value> against the
stage-by-stage route, -c auto against -c <the printed mean>, a known-answer expansion longer than the reads, two ranks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import bam_writer as bw

pytestmark = pytest.mark.gpu



def _dna(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _mixed_records(rng, refs, n):
    """mapped short reads, 15-kb reads with long CIGARs, zero-length CIGARs, placed-unmapped and unplaced records"""
    recs = []
    for i in range(n):
        name, length = refs[int(rng.integers(0, len(refs)))]
        kind = rng.random()
        pos = int(rng.integers(1, length + 50))                 # some start past the last full window
        if kind < 0.6:
            L = int(rng.integers(50, 250))
            recs.append(("r%d" % i, 0, name, pos, 60, "%dM" % L, _dna(rng, L), "*"))
        elif kind < 0.7:                                         # a long read: many ops, D and N included
            ops, ql = [], 0
            while ql < 15000:
                m = int(rng.integers(20, 400))
                ops.append("%dM" % m)
                ql += m
                r = rng.random()
                if r < 0.3:
                    ops.append("%dD" % int(rng.integers(1, 40)))
                elif r < 0.4:
                    ops.append("%dN" % int(rng.integers(1, 300)))
                elif r < 0.6:
                    k = int(rng.integers(1, 30))
                    ops.append("%dI" % k)
                    ql += k
            recs.append(("l%d" % i, 0, name, pos, 60, "".join(ops), _dna(rng, ql), "*"))
        elif kind < 0.75:                                        # a CIGAR without reference bases: zero length
            recs.append(("z%d" % i, 0, name, pos, 60, "30S20I", _dna(rng, 50), "*"))
        elif kind < 0.85:                                        # placed unmapped: [pos, pos + l_seq)
            L = int(rng.integers(0, 300))
            recs.append(("p%d" % i, 4 | 0x400 * int(rng.random() < 0.3), name, pos, 0, "*", _dna(rng, L) if L else "*", "*"))
        elif kind < 0.9:                                         # secondary / supplementary / QC-fail count too
            recs.append(("s%d" % i, int(rng.choice([0x100, 0x800, 0x200])), name, pos, 0, "100M", _dna(rng, 100), "*"))
        else:                                                    # unplaced
            recs.append(("u%d" % i, 4, "*", 0, 0, "*", _dna(rng, 100), "*"))
    return recs


def _host_windows(refs, recs):
    """{reference: (bp, present)} by the host twin, intervals by coverage.record_interval of the SAM-text reads"""
    from advntr_amd import coverage, sam_utils
    sam = sam_utils.parse_sam(bw.sam_text(refs, recs))
    index = {name: i for i, (name, _) in enumerate(refs)}
    rec_ref, rs, re_ = [], [], []
    for r in sam.reads:
        s, e = coverage.record_interval(r)
        rec_ref.append(index.get(r.reference_name, -1))
        rs.append(s)
        re_.append(e)
    n_windows = [L // 100 for _, L in refs]
    bp, present = coverage.windows_host(n_windows, rec_ref, rs, re_)
    out, at = {}, 0
    for (name, _), n in zip(refs, n_windows):
        out[name] = (bp[at:at + n], present[at:at + n])
        at += n
    return out


REFS = [("chr1", 120000), ("2", 60050), ("chrUn_gl", 30000), ("chrY", 99), ("chr3", 5000)]


@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(31)
    # chr3 holds only zero-length intervals and one read: windows present with 0 bp next to empty ones
    recs = _mixed_records(rng, REFS[:4], 3000) + [("z_a", 0, "chr3", 1001, 60, "30S20I", _dna(rng, 50), "*"),
                                                   ("z_b", 4, "chr3", 3051, 0, "*", "*", "*"),
                                                   ("z_c", 0, "chr3", 4001, 60, "50M", _dna(rng, 50), "*")]
    sorted_recs = sorted(recs, key=lambda r: (r[2] == "*", r[2], r[3]))
    return recs, sorted_recs, _host_windows(REFS, recs)


@pytest.mark.parametrize("framing, chunk, order", [("htslib", 0, "sorted"), ("htsjdk", 0, "unsorted"),
                                                   ("htslib", 3000, "unsorted"), ("htsjdk", 700, "sorted")])
def test_device_windows_equal_host_twin(tmp_path, mixed, framing, chunk, order):
    from advntr_amd import bam
    recs, sorted_recs, want = mixed
    p = tmp_path / "x.bam"
    p.write_bytes(bw.write_bam(REFS, sorted_recs if order == "sorted" else recs, framing, block_data=4000 if chunk else bw.BLOCK_DATA))
    f = bam.open_alignment(str(p), [], chunk_bytes=chunk, coverage=True, coverage_windows=True)
    assert f.stats["chunks"] >= (3 if chunk else 1)
    got = f.coverage.windows
    assert set(got) == set(want)
    for name in got:
        assert np.array_equal(got[name][0], want[name][0]), name
        assert np.array_equal(got[name][1], want[name][1]), name
    assert any((want[n][1] & (want[n][0] == 0)).any() for n in want)        # a window present with 0 bp
    assert want["chr3"][1].tolist() == [int(w in (10, 30, 40)) for w in range(50)]
    # bins without a genome: every counted window in bin 0 (chr1, '2', chr3; chrUn_gl is not counted; chrY has no full window)
    from advntr_amd import coverage
    hb = coverage.bins_host(*want["chr1"])
    hb = coverage.bins_host(*want["2"], bin_windows=hb[0], bin_bp=hb[1])
    hb = coverage.bins_host(*want["chr3"], bin_windows=hb[0], bin_bp=hb[1])
    assert f.coverage.corrector.bin_windows == hb[0].tolist() and f.coverage.corrector.bin_bp == hb[1].tolist()


def test_the_flag_leaves_the_selection_unchanged(tmp_path, mixed):
    from advntr_amd import bam
    recs, sorted_recs, _ = mixed
    p = tmp_path / "x.bam"
    p.write_bytes(bw.write_bam(REFS, sorted_recs, "htslib", block_data=4000))
    windows = [("chr1", 1000, 5000), ("2", 20000, 20100)]
    a = bam.open_alignment(str(p), windows, chunk_bytes=5000, record_offsets=True)
    b = bam.open_alignment(str(p), windows, chunk_bytes=5000, record_offsets=True, coverage=True)
    assert a.coverage is None and b.coverage is not None
    keys = ("query_name", "flag", "reference_name", "reference_start", "reference_end", "mapq", "cigar", "seq", "query_qualities")
    assert [[getattr(r, k) for k in keys] for r in a.reads] == [[getattr(r, k) for k in keys] for r in b.reads]
    assert np.array_equal(a.offsets, b.offsets)
    for k in ("blocks", "compressed_bytes", "uncompressed_bytes", "records", "kept", "chunks", "fallback_blocks"):
        assert a.stats[k] == b.stats[k], k


def test_gc_kernel_and_device_bins_equal_host(tmp_path, mixed):
    from advntr_amd import bam, coverage, genome
    recs, sorted_recs, want = mixed
    rng = np.random.default_rng(32)
    seqs = {"chr1": rng.choice(np.frombuffer(b"ACGTacgtGCNn", np.uint8), 120000), "chr2": rng.choice(np.frombuffer(b"GCgcAT", np.uint8), 60050)}
    # chr3 is absent from this genome: it contributes nothing
    for codes in list(seqs.values()) + [seqs["chr1"][:12345], seqs["chr1"][:99]]:
        got, ms = coverage.gc_device(codes)
        assert np.array_equal(got, coverage.gc_host(codes))
    gen = genome.Genome({k: genome.Chromosome(k, np.ascontiguousarray(v)) for k, v in seqs.items()}, 0.0)
    p = tmp_path / "x.bam"
    p.write_bytes(bw.write_bam(REFS, sorted_recs))
    f = bam.open_alignment(str(p), [], coverage=True, genome=gen)
    hb = coverage.bins_host(*want["chr1"], gc=coverage.gc_host(seqs["chr1"]))
    hb = coverage.bins_host(*want["2"], gc=coverage.gc_host(seqs["chr2"]), bin_windows=hb[0], bin_bp=hb[1])
    assert f.coverage.corrector.bin_windows == hb[0].tolist() and f.coverage.corrector.bin_bp == hb[1].tolist()
    assert sum(1 for w in hb[0] if w) >= 3
    assert f.coverage.stats["gc_kernel_ms"] > 0 and f.coverage.stats["accumulate_kernel_ms"] > 0


# ---- genotype --expansion end to end ----

UNIT, REF_COPIES, COPIES, READ, DEPTH = "GATCCAGGTAGCATTCAGGTCCATGAGCTA", 5, 80, 150, 30
VNTR_AT, CHR1, CHR2 = 30000, 60000, 20000


@pytest.fixture(scope="module")
def expansion(tmp_path_factory):
    """a homozygous allele of 80 x 30 bp (the reference has 5 copies) sequenced at 30x with 150-bp reads: the reads that lie
    wholly inside the repeat are unplaced unmapped records, the others are mapped to the reference's coordinates"""
    d = tmp_path_factory.mktemp("expansion")
    rng = np.random.default_rng(41)
    chr1 = _dna(rng, VNTR_AT) + UNIT * REF_COPIES + _dna(rng, CHR1 - VNTR_AT - REF_COPIES * len(UNIT))
    chr2 = _dna(rng, CHR2)
    masked = "".join(c.lower() if 5000 <= i < 8000 else c for i, c in enumerate(chr2))     # soft-masked stretch
    shift = (COPIES - REF_COPIES) * len(UNIT)
    sample = chr1[:VNTR_AT] + UNIT * COPIES + chr1[VNTR_AT + REF_COPIES * len(UNIT):]
    rep_end = VNTR_AT + COPIES * len(UNIT)
    recs, n = [], 0
    for hap, L in ((sample, len(sample)), (chr2, CHR2)):
        for _ in range(DEPTH * L // READ):
            s = int(rng.integers(0, L - READ + 1))
            seq, name = hap[s:s + READ], "q%d" % n
            n += 1
            if hap is chr2:
                recs.append((name, 0, "chr2", s + 1, 60, "150M", seq, "I" * READ))
            elif s + READ <= VNTR_AT or s < VNTR_AT:
                recs.append((name, 0, "chr1", s + 1, 60, "150M", seq, "I" * READ))
            elif s + READ <= rep_end:
                recs.append((name, 4, "*", 0, 0, "*", seq, "I" * READ))
            else:
                recs.append((name, 0, "chr1", s - shift + 1, 60, "150M", seq, "I" * READ))
    mapped = sorted([r for r in recs if r[2] != "*"], key=lambda r: (r[2], r[3]))
    recs = mapped + [r for r in recs if r[2] == "*"]
    refs = [("chr1", CHR1), ("chr2", CHR2)]
    (d / "sample.bam").write_bytes(bw.write_bam(refs, recs))
    (d / "sample.sam").write_text(bw.sam_text(refs, recs))
    (d / "genome.fa").write_text(">chr1\n%s\n>chr2\n%s\n" % (chr1, masked))
    locus = {"id": 1, "left": chr1[VNTR_AT - 500:VNTR_AT], "right": chr1[VNTR_AT + REF_COPIES * len(UNIT):][:500],
             "pattern": UNIT, "repeat_segments": [UNIT] * REF_COPIES, "scaled_score": None, "chromosome": "chr1",
             "start_point": VNTR_AT}
    (d / "loci.json").write_text(json.dumps([locus]))
    depth = sum(READ for r in recs if r[2] != "*") / float(CHR1 + CHR2)     # the mapped depth the windows see
    return d, locus, recs, depth


def _cli(*args, env=None, launcher=None):
    cmd = (launcher or [sys.executable]) + ["-m", "advntr_amd", "genotype"] + [str(a) for a in args]
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, env=env)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    return out.stdout.decode(), out.stderr.decode()


def _coverage_line(err):
    lines = [l for l in err.split("\n") if l.startswith('{"coverage"')]
    assert len(lines) == 1, err[-2000:]
    return json.loads(lines[0])["coverage"]


def _stage_route(path, locus, average_coverage):
    """the genotype driver's Illumina --alignment route stage by stage: selection, keyword filter of the unmapped reads,
    models, select_illumina_reads_multi, find_repeat_count_from_selected_reads(average_coverage=...)"""
    from advntr_amd import bam, filtering, genome_analyzer, hmm_utils, models, sam_utils, settings, vntr_finder
    settings.MAX_ERROR_RATE = 0.05
    v = models.ReferenceVNTR(locus["id"], locus["pattern"], locus["start_point"], locus["chromosome"], None, None,
                             len(locus["repeat_segments"]))
    v.init_from_xml(locus["repeat_segments"], locus["left"], locus["right"])
    if str(path).endswith(".bam"):
        samfile = bam.open_alignment(str(path), bam.vntr_windows(bam.read_header(str(path))[0], [v]))
    else:
        samfile = sam_utils.parse_sam(open(str(path)).read())
    seqs = [r.seq for r in samfile.reads if r.is_unmapped]
    keywords = {1: filtering.get_keywords_for_filtering(locus["left"], locus["repeat_segments"], locus["right"], locus["pattern"],
                                                        True, 15)}
    _, ids = filtering.get_filtered_read_ids("".join(">%d\n%s\n" % (i, s.upper()) for i, s in enumerate(seqs)), keywords,
                                             min_matches=5)
    cands = [seqs[i] for i in sorted(int(x) for x in ids.get(1, ()))]
    head = [len(r.seq) for r in samfile.head(5)]
    rl = sorted(head)[len(head) // 2]
    built = hmm_utils.build_read_matcher_models([(locus["left"][-rl:], locus["right"][:rl], locus["repeat_segments"],
                                                  vntr_finder.get_copies_for_hmm(rl, len(locus["pattern"])))])
    v.scaled_score = None
    picked, _ = vntr_finder.select_illumina_reads_multi([v], samfile, [cands], models=built)
    res = vntr_finder.find_repeat_count_from_selected_reads([s.summary for s in picked[0]], average_coverage=average_coverage)
    return genome_analyzer.genotype_row("text", v, locus["id"], res, False, False), res


def test_expansion_with_a_given_coverage_equals_the_stage_route(expansion):
    d, locus, _, _ = expansion
    want, res = _stage_route(d / "sample.bam", locus, 30.0)
    assert res.copy_numbers[0] == res.copy_numbers[1] and res.maximum_likelihood == 0
    for aln in ("sample.bam", "sample.sam"):
        out, _ = _cli("--loci", d / "loci.json", "--alignment", d / aln, "--expansion", "-c", "30")
        assert out == want, aln
    assert _stage_route(d / "sample.sam", locus, 30.0)[0] == want
    # -c 0: the exact genotype; -c without -e: ignored
    exact, _ = _cli("--loci", d / "loci.json", "--alignment", d / "sample.bam")
    assert _cli("--loci", d / "loci.json", "--alignment", d / "sample.bam", "-e", "-c", "0")[0] == exact
    assert _cli("--loci", d / "loci.json", "--alignment", d / "sample.bam", "-c", "30")[0] == exact
    vcf, _ = _cli("--loci", d / "loci.json", "--alignment", d / "sample.bam", "-e", "-c", "30", "--outfmt", "vcf")
    assert vcf.rstrip("\n").split("\n")[-1].split("\t")[-1].endswith(":0.0000")


def test_auto_coverage_rows_equal_the_printed_mean(expansion):
    from advntr_amd import coverage, sam_utils
    d, locus, recs, depth = expansion
    out, err = _cli("--loci", d / "loci.json", "--alignment", d / "sample.bam", "-e", "-c", "auto")
    cov = _coverage_line(err)
    assert cov["divisor"] == "sequencing_mean" and cov["windows"] == (CHR1 + CHR2) // 100
    text = (d / "sample.sam").read_text()
    host = coverage.measure_sam(sam_utils.parse_sam(text), coverage.sam_reference_lengths(text))
    assert cov["sequencing_mean"] == host.corrector.get_sequencing_mean_coverage()
    assert abs(cov["sequencing_mean"] - depth) <= 0.02 * depth, (cov["sequencing_mean"], depth)
    again, _ = _cli("--loci", d / "loci.json", "--alignment", d / "sample.bam", "-e", "-c", repr(cov["sequencing_mean"]))
    assert out == again
    sam_out, sam_err = _cli("--loci", d / "loci.json", "--alignment", d / "sample.sam", "-e", "-c", "auto")
    assert sam_out == out and _coverage_line(sam_err) == cov


def test_auto_coverage_by_gc_bin(expansion):
    from advntr_amd import coverage, genome, sam_utils
    d, locus, _, _ = expansion
    out, err = _cli("--loci", d / "loci.json", "--alignment", d / "sample.bam", "-e", "-c", "auto", "-r", d / "genome.fa")
    cov = _coverage_line(err)
    text = (d / "sample.sam").read_text()
    host = coverage.measure_sam(sam_utils.parse_sam(text), coverage.sam_reference_lengths(text), genome.read_genome(str(d / "genome.fa")))
    assert cov == host.summary() and cov["divisor"] == "gc_bin"
    divisor, source = host.divisor(locus["repeat_segments"])
    assert source == "gc_bin"
    again, _ = _cli("--loci", d / "loci.json", "--alignment", d / "sample.bam", "-e", "-c", repr(divisor))
    assert out == again
    # the soft-masked stretch of chr2 (no uppercase G / C) fills bin 0
    assert cov["bins"][0][0] >= 30


def test_known_answer_expansion_longer_than_the_reads(expansion):
    """80 copies of 30 bp (2 400 bp, 16 reads long) at 30x: int(occurrences / (coverage x 2)).  Every base of the allele is
    read about DEPTH times over both haplotypes, so the RU occurrences are about DEPTH x COPIES and the estimator, which divides
    by coverage x haplotypes, returns about COPIES / 2 for a homozygous allele: the reference's bias, kept."""
    d, locus, _, _ = expansion
    out, err = _cli("--loci", d / "loci.json", "--alignment", d / "sample.bam", "-e", "-c", "auto")
    est = [int(x) for x in out.split("\n")[1].split("/")]
    assert est[0] == est[1]
    assert abs(est[0] - COPIES / 2) <= 0.15 * COPIES / 2, (est, _coverage_line(err))


def test_two_ranks_equal_one(expansion):
    d, locus, _, _ = expansion
    (d / "loci2.json").write_text(json.dumps([locus, dict(locus, id=2)]))      # a locus for each rank
    args = ["--loci", d / "loci2.json", "--alignment", d / "sample.bam", "-e", "-c", "auto", "-r", d / "genome.fa"]
    single, err1 = _cli(*args)
    env = dict(os.environ, ADVNTR_DIST_BACKEND="host")
    multi, err2 = _cli(*args, env=env, launcher=[sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                                                 "--master-addr", "127.0.0.1", "--master-port", "29587"])
    assert multi == single
    assert _coverage_line(err2) == _coverage_line(err1)
