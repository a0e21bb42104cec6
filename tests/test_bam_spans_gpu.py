"""Long reads of an aligned BAM on the MI355X: the device pass (pair enumeration, span kernel, trim decode) against the host
twin in both framings with records crossing chunk edges, `genotype --pacbio --alignment` on synthetic loci of known
genotype, BAM against SAM text, against the stage-by-stage route, and two ranks against one process."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import bam_writer as bw

pytestmark = pytest.mark.gpu


def _rand(rng, n):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, n))


def _long_records(rng, n):
    """n mapped long reads with CIGARs of dozens to hundreds of ops (one of more than 1 000) on two references, some
    unmapped ones, and the windows they are checked against (overlapping windows included)."""
    recs = []
    for i in range(n):
        ops = []
        if rng.random() < 0.5:
            ops.append((int(rng.integers(1, 300)), "S"))
        n_ops = 1400 if i == 7 else int(rng.integers(1, 160))
        for _ in range(n_ops):
            r = rng.random()
            op = "M" if r < 0.6 else "I" if r < 0.75 else "D" if r < 0.9 else "=" if r < 0.95 else "X"
            ops.append((int(rng.integers(1, 4)) if n_ops > 1000 else int(rng.integers(1, 120 if op in "M=X" else 6)), op))
        if rng.random() < 0.5:
            ops.append((int(rng.integers(1, 300)), "S"))
        qlen = sum(k for k, op in ops if op in "MIS=X")
        ref = "chr1" if i % 3 else "chr2"
        pos = int(rng.integers(1, 40000))
        recs.append(("L%d" % i, 0 if rng.random() < 0.9 else 256, ref, pos, 60, "".join("%d%s" % t for t in ops),
                     _rand(rng, qlen) if rng.random() > 0.01 else "*", "*"))
    recs.sort(key=lambda r: (r[2], r[3]))
    for i in range(n // 20):
        recs.append(("U%d" % i, 4, "*", 0, 0, "*", _rand(rng, int(rng.integers(500, 4000))), "*"))
    windows = []
    for k in range(120):
        ref = "chr1" if k % 2 else "chr2"
        vs = int(rng.integers(200, 45000))
        windows.append((ref, vs, vs + int(rng.integers(0, 400)), 1000 + k))
    windows.append(("chr1", windows[1][1] + 5, windows[1][1] + 200, 5000))          # overlaps window 1
    windows.append(("chr3", 100, 200, 5001))                                         # a reference the file does not have
    return recs, windows


@pytest.mark.parametrize("framing", ["htslib", "htsjdk"])
def test_device_pairs_equal_host_twin(tmp_path, framing):
    from advntr_amd import bam, sam_utils
    rng = np.random.default_rng(41)
    refs = [("chr1", 100000), ("chr2", 100000)]
    recs, windows = _long_records(rng, 2200)
    assert max(r[5].count("M") + r[5].count("I") + r[5].count("D") for r in recs) > 1000
    data = bw.write_bam(refs, recs, framing)
    path = tmp_path / "long.bam"
    path.write_bytes(data)
    raw = bw.inflate_all(data)
    offs = bw.walk_records(raw)
    reads = sam_utils.parse_sam(bw.sam_text(refs, recs)).reads          # what fetch sees: file order, reference_end
    # expected pairs: per window in input order, the mapped records overlapping it (SamFile.fetch), in file order
    want_rec, want_win = [], []
    for k, (ref, vs, ve, _) in enumerate(windows):
        for i, r in enumerate(reads):
            if r.is_unmapped or r.reference_name != ref:
                continue
            end = r.reference_end if r.reference_end is not None else r.reference_start + 1
            if r.reference_start < ve and end > vs:
                want_rec.append(i)
                want_win.append(k)
    assert len(want_rec) > 1000
    tp, tpieces = bam.span_host(raw, np.array(offs)[want_rec], [windows[k][1:3] for k in want_win])
    assert sum(p is not None for p in tpieces) > 100
    for chunk in (150000, 0):           # small chunks: records cross chunk edges
        got = bam.open_alignment_spans(str(path), windows, chunk_bytes=chunk)
        assert got.stats["chunks"] > (5 if chunk else 0)
        assert got.pairs[:, 0].tolist() == want_win
        assert got.pairs[:, 1].tolist() == [windows[k][3] for k in want_win]
        assert got.pairs[:, 2].tolist() == want_rec
        assert (got.pairs[:, 3:] == tp[:, 3:]).all()
        assert got.pieces == tpieces
        assert got.stats["pairs"] == len(want_rec) and got.stats["spanning"] == sum(p is not None for p in tpieces)
        assert got.stats["trimmed_bytes"] < got.stats["whole_bytes"]
        unmapped = [r for r in reads if r.is_unmapped]
        assert [(r.query_name, r.seq) for r in got.unmapped] == [(r.query_name, r.seq) for r in unmapped]


def test_device_cg_placeholder_is_an_error(tmp_path):
    from advntr_amd import _lib, bam
    refs = [("chr1", 100000)]
    seq = "ACGT" * 100
    recs = [("ok", 0, "chr1", 801, 60, "400M", seq, "*"), ("cg_read", 0, "chr1", 801, 60, "400S5000N", seq, "*")]
    (tmp_path / "cg.bam").write_bytes(bw.write_bam(refs, recs))
    with pytest.raises(_lib.EngineError, match="cg_read.*CG tag") as e:
        bam.open_alignment_spans(str(tmp_path / "cg.bam"), [("chr1", 1000, 1050)])
    assert e.value.code == _lib.ERR_DATA


def _known_loci(rng, n_loci, reads_per_hap=8, n_unmapped=3):
    """Loci of known genotype on chr1 and error-free long reads of their two haplotypes, mapped with I / D ops for the
    expansions and contractions; plus unmapped whole reads (some from the loci, some unrelated)."""
    chrom, loci, mapped, unmapped, truth = [_rand(rng, 3000)], [], [], [], []
    at = 3000
    for i in range(n_loci):
        plen = int(rng.integers(8, 30))
        ref_copies = int(rng.integers(4, 9))
        pattern, left, right = _rand(rng, plen), _rand(rng, 600), _rand(rng, 600)
        vs = at + len(left)
        ve = vs + plen * ref_copies
        chrom += [left, pattern * ref_copies, right, _rand(rng, 2000)]
        at = ve + len(right) + 2000
        a = max(1, ref_copies + int(rng.integers(-3, 4)))
        b = a if i % 4 == 0 else max(1, ref_copies + int(rng.integers(-3, 4)))
        truth.append(tuple(sorted((a, b))))
        loci.append({"id": 700 + i, "left": left, "right": right, "pattern": pattern, "repeat_segments": [pattern] * ref_copies,
                     "scaled_score": None, "chromosome": "chr1", "start_point": vs})
        for h, c in enumerate((a, b)):
            for j in range(reads_per_hap):
                la, lb = int(rng.integers(150, 550)), int(rng.integers(150, 550))
                seq = left[-la:] + pattern * c + right[:lb]
                if c > ref_copies:
                    cigar = "%dM%dI%dM" % (la + ref_copies * plen, (c - ref_copies) * plen, lb)
                elif c < ref_copies:
                    cigar = "%dM%dD%dM" % (la + c * plen, (ref_copies - c) * plen, lb)
                else:
                    cigar = "%dM" % len(seq)
                mapped.append(("m%d_%d_%d" % (i, h, j), 0, "chr1", vs - la + 1, 60, cigar, seq, "*"))
        for j in range(n_unmapped):
            c = (a, b)[j % 2]
            unmapped.append(("u%d_%d" % (i, j), 4, "*", 0, 0, "*", _rand(rng, 300) + left[-400:] + pattern * c + right[:400] +
                             _rand(rng, 300), "*"))
    unmapped.append(("noise", 4, "*", 0, 0, "*", _rand(rng, 3000), "*"))
    mapped.sort(key=lambda r: r[3])
    return loci, [("chr1", len("".join(chrom)))], mapped + unmapped, truth


def _cli(*args, env=None, launcher=None):
    cmd = (launcher or [sys.executable]) + ["-m", "advntr_amd", "genotype"] + [str(a) for a in args]
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, env=env)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    return out.stdout.decode()


@pytest.fixture(scope="module")
def known(tmp_path_factory):
    d = tmp_path_factory.mktemp("pacbio_aln")
    loci, refs, recs, truth = _known_loci(np.random.default_rng(5), 12)
    (d / "loci.json").write_text(json.dumps(loci))
    (d / "sample.sam").write_text(bw.sam_text(refs, recs))
    (d / "bam").mkdir()
    (d / "bam" / "sample.bam").write_bytes(bw.write_bam(refs, recs, "htsjdk"))
    return d, loci, refs, recs, truth


def test_cli_pacbio_alignment_known_genotypes(known):
    d, loci, _, _, truth = known
    out = _cli("--loci", d / "loci.json", "--alignment", d / "bam" / "sample.bam", "--pacbio")
    want = "".join("%d\n%d/%d\n" % (loc["id"], a, b) for loc, (a, b) in zip(loci, truth))
    assert out == want


def test_cli_pacbio_alignment_bam_equals_sam(known):
    d = known[0]
    for fmt in ("text", "bed", "vcf"):
        a = _cli("--loci", d / "loci.json", "--alignment", d / "sample.sam", "--pacbio", "--outfmt", fmt)
        b = _cli("--loci", d / "loci.json", "--alignment", d / "bam" / "sample.bam", "--pacbio", "--outfmt", fmt)
        assert a == b and a.strip()


def test_cli_pacbio_alignment_equals_stage_by_stage(known):
    """host-twin pieces of the mapped records + the keyword filter -> extract_spanning_reads on the unmapped records ->
    get_dominant_copy_numbers_from_spanning_reads per locus.  --min-matches 2 lets the unmapped reads that hold both
    80-base flank keywords through, so that both halves count."""
    from advntr_amd import bam, filtering, genome_analyzer, models, settings, vntr_finder
    d, loci, refs, recs, _ = known
    settings.MAX_ERROR_RATE = 0.3
    raw = bw.inflate_all((d / "bam" / "sample.bam").read_bytes())
    offs = np.array(bw.walk_records(raw))
    unmapped = [r[6] for r in recs if r[1] & 4]
    fasta = "".join(">%d\n%s\n" % (i, s) for i, s in enumerate(unmapped))
    keywords = {loc["id"]: filtering.get_keywords_for_filtering(loc["left"], loc["repeat_segments"], loc["right"], loc["pattern"],
                                                                False) for loc in loci}
    _, ids = filtering.get_filtered_read_ids(fasta, keywords, min_matches=2)
    rows, n_unaligned = [], 0
    for loc in loci:
        vs, ve = loc["start_point"], loc["start_point"] + len("".join(loc["repeat_segments"]))
        idx = [i for i, r in enumerate(recs) if not r[1] & 4 and r[3] - 1 < ve and
               r[3] - 1 + sum(int(n) for n, op in re.findall(r"(\d+)([MDN=X])", r[5])) > vs]
        _, pieces = bam.span_host(raw, offs[idx], [(vs, ve)] * len(idx))
        mapped = [p[1] for p in pieces if p is not None]
        cands = [unmapped[int(i)] for i in sorted(int(n) for n in ids.get(loc["id"], ()))]
        unaligned = [t[0] for t in vntr_finder.extract_spanning_reads(loc["left"], loc["right"], cands)[0]]
        n_unaligned += len(unaligned)
        spanning = mapped + unaligned
        geno, prob = vntr_finder.get_dominant_copy_numbers_from_spanning_reads(loc["left"], loc["right"], loc["repeat_segments"],
                                                                               loc["pattern"], spanning)
        v = models.ReferenceVNTR(loc["id"], loc["pattern"], loc["start_point"], loc["chromosome"], None, None,
                                 len(loc["repeat_segments"]))
        v.init_from_xml(loc["repeat_segments"], loc["left"], loc["right"])
        res = vntr_finder.GenotypeResult(geno, len(spanning), len(spanning), 0, prob)
        rows.append(genome_analyzer.genotype_row("bed", v, loc["id"], res, False, False))
    assert n_unaligned > 0
    out = _cli("--loci", d / "loci.json", "--alignment", d / "bam" / "sample.bam", "--pacbio", "--outfmt", "bed",
               "--min-matches", "2")
    assert out == genome_analyzer.bed_header(False) + "".join(rows)


def test_cli_pacbio_alignment_two_ranks_equal_one(known):
    d = known[0]
    args = ["--loci", d / "loci.json", "--alignment", d / "bam" / "sample.bam", "--pacbio", "--outfmt", "bed"]
    single = _cli(*args)
    env = dict(os.environ, ADVNTR_DIST_BACKEND="host")
    multi = _cli(*args, env=env, launcher=[sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                                           "--master-addr", "127.0.0.1", "--master-port", "29583"])
    rows = lambda out: [l for l in out.split("\n") if l.startswith("chr")]
    assert len(rows(single)) == 12 and rows(multi) == rows(single)
