"""BAM input on the MI355X: device inflate against zlib, the CRC check, exact record boundaries in both framings and across
chunk boundaries, the kept records against sam_utils.parse_sam of the same records as SAM text, the golden read
selection, and the genotype command line on BAM against SAM text."""
import gzip
import json
import os
import random
import struct
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import ROOT
import bam_writer as bw

pytestmark = pytest.mark.gpu

FIELDS = ("query_name", "flag", "reference_name", "reference_start", "reference_end", "mapq", "cigar", "seq", "query_qualities")


def _same_reads(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for a in FIELDS:
            assert getattr(g, a) == getattr(w, a), (w.query_name, a, getattr(g, a), getattr(w, a))


def test_inflate_parity_levels_strategies_shapes():
    from advntr_amd import bam
    rng = random.Random(7)
    pieces = [b"", os.urandom(30000), b"\0" * 65536, b"ACGT" * 16384, bytes(rng.choice(b"ACGTN") for _ in range(65280)),
              (b"q" + os.urandom(258)) * 200,                              # length-258 matches
              os.urandom(32768) * 2,                                       # distance 32 768 (length 258 in a row)
              b"a" * 60000]                                                # distance 1
    modes = [(lv, st) for lv in (0, 1, 6, 9) for st in bw.STRATEGIES]
    blocks = []
    for p in pieces:
        for m in modes:
            try:
                blocks.append(bw.bgzf_block(p, *m))
            except ValueError:         # incompressible data at 64 KiB does not fit one block: not a BGZF block
                pass
    data = b"".join(blocks) + bw.EOF_BLOCK
    assert bam.inflate(data) == bw.inflate_all(data)


def test_inflate_more_than_20000_blocks():
    from advntr_amd import bam
    rng = np.random.default_rng(3)
    pieces = [rng.integers(0, 4, int(n), dtype=np.uint8).tobytes() for n in rng.integers(0, 400, 20500)]
    data = bw.bgzf_blocks(pieces, modes=((1, "default"), (6, "huffman"), (9, "rle"), (0, "default")))
    assert bam.inflate(data) == bw.inflate_all(data)


def test_crc_mismatch_names_the_block():
    from advntr_amd import _lib, bam
    pieces = [os.urandom(1000) for _ in range(6)]
    data = bytearray(bw.bgzf_blocks(pieces))
    off, size, _ = bam.scan_framing(bytes(data))
    bad = int(off[3])
    at = bad + int(size[3]) - 8
    struct.pack_into("<I", data, at, struct.unpack_from("<I", data, at)[0] ^ 1)
    with pytest.raises(_lib.EngineError, match="file offset %d: CRC32 mismatch" % bad) as e:
        bam.inflate(bytes(data))
    assert e.value.code == _lib.ERR_DATA


def _records(rng, n, refs, long_at=None):
    recs = []
    for i in range(n):
        ref = refs[i % len(refs)][0]
        L = 70000 if i == long_at else int(rng.integers(50, 300))
        seq = "".join("ACGT"[x] for x in rng.integers(0, 4, L))
        qual = "".join(chr(33 + int(q)) for q in rng.integers(2, 41, L))
        recs.append(("read%d" % i, 0, ref, 1000 + 10 * i, 60, "%dM" % L, seq, qual))
    return recs


@pytest.mark.parametrize("framing", ["htslib", "htsjdk"])
@pytest.mark.parametrize("chunk", [0, 20000, 70000])
def test_record_boundaries_equal_sequential_walk(tmp_path, framing, chunk):
    from advntr_amd import bam
    refs = [("chr1", 10 ** 7), ("chr2", 10 ** 7)]
    recs = _records(np.random.default_rng(9), 1500, refs, long_at=700)
    data = bw.write_bam(refs, recs, framing, modes=((6, "default"), (1, "fixed"), (9, "filtered")))
    path = tmp_path / "b.bam"
    path.write_bytes(data)
    f = bam.open_alignment(str(path), [], chunk_bytes=chunk, record_offsets=True)
    assert list(f.offsets) == bw.walk_records(bw.inflate_all(data))
    assert f.stats["records"] == len(recs)
    assert [r.query_name for r in f.head(5)] == ["read%d" % i for i in range(5)]
    if chunk:
        assert f.stats["chunks"] > 1
    if framing == "htsjdk" and chunk == 0:     # (a chunk of one block starts at the carried record: nothing to check)
        assert f.stats["fallback_blocks"] > 0
    if framing == "htslib":     # only the block that starts inside the 70 kb record is walked on the host
        assert f.stats["fallback_blocks"] <= 1


def _field_records():
    refs = [("chr1", 100000), ("chr2", 5000), ("chr3", 7000)]
    rng = random.Random(4)
    recs = [
        ("h1", 0, "chr1", 101, 60, "4M2D2M1I2M3S", "ACGTACGTACGT", "IIIIIIIIIIII"),
        ("h2", 1024, "chr1", 201, 0, "12M", "ACGTACGTACGT", "#" + "I" * 11),
        ("u1", 4, "*", 0, 0, "*", "ACGTNACGT", "*"),                   # unplaced unmapped
        ("h4", 16, "chr2", 11, 30, "5M100N5M", "ACGTACGTAC", "IIIIIIIIII"),
        ("u2", 4, "chr2", 40, 0, "*", "*", "*"),                       # placed unmapped, no sequence
        ("c1", 0, "chr1", 300, 37, "1M1I1D1N1S1H1P1=1X", "=ACMGRSVTWYHKDBN", "ABCDEFGHIJKLMNOP"),
        ("c2", 0, "chr2", 90, 20, "*", "GATTACA", "IIIIIII"),           # mapped, no CIGAR: end = start + 1 for fetch
        ("c3", 0, "chr1", 5000, 60, "3S5M", "ACGTACGTA", "*"),          # odd l_seq, 0xFF qualities
        ("c4", 0, "chr1", 5003, 60, "2I", "AC", "II"),                  # no reference span
        ("far", 0, "chr1", 90000, 60, "10M", "ACGTACGTAC", "IIIIIIIIII"),   # outside every window: not kept
        ("c5", 0, "chr3", 6000, 60, "10M", "ACGTACGTAC", "IIIIIIIIII"),
    ]
    for i in range(300):
        L = rng.randint(1, 151)
        seq = "".join(rng.choice("=ACMGRSVTWYHKDBN") for _ in range(L))
        ref = rng.choice(refs)[0]
        pos = rng.randint(1, 4000)
        flag = rng.choice([0, 16, 1024, 4, 4 | 16])
        recs.append(("x%d" % i, flag, ref if flag & 4 == 0 or rng.random() < 0.5 else "*", pos if ref != "*" else 0,
                     rng.randint(0, 60), "*" if flag & 4 else "%dM" % L, seq, "".join(chr(33 + rng.randint(0, 40)) for _ in range(L))))
    for r in list(recs):
        if r[2] == "*" and r[3]:
            recs[recs.index(r)] = r[:3] + (0,) + r[4:]
    windows = [("chr1", 100, 400), ("chr1", 4990, 5010), ("chr1", 1000, 3000), ("chr2", 0, 200), ("chr2", 2000, 2500),
               ("chr3", 6005, 6006)]
    return refs, recs, windows


@pytest.mark.parametrize("framing", ["htslib", "htsjdk"])
def test_kept_records_equal_sam_text_route(tmp_path, framing):
    from advntr_amd import bam, sam_utils
    refs, recs, windows = _field_records()
    path = tmp_path / "f.bam"
    path.write_bytes(bw.write_bam(refs, recs, framing, block_data=4000 if framing == "htsjdk" else bw.BLOCK_DATA))
    got = bam.open_alignment(str(path), windows, chunk_bytes=3000)
    want = sam_utils.parse_sam(bw.sam_text(refs, recs))
    assert got.references == want.references
    _same_reads(got.head(5), want.head(5))
    _same_reads([r for r in got.reads if r.is_unmapped], [r for r in want.reads if r.is_unmapped])
    for ref, s, e in windows + [("chr1", 120, 130), ("chr3", 6005, 6006)]:
        _same_reads(list(got.fetch(ref, s, e)), list(want.fetch(ref, s, e)))
    assert "far" not in {r.query_name for r in got.reads}
    with pytest.raises(ValueError):
        list(got.fetch("chr1", 89000, 91000))
    # kept = head(5) + every read a window fetches + every unmapped one, in file order
    keep = {r.query_name for r in want.head(5)} | {r.query_name for r in want.reads if r.is_unmapped}
    for ref, s, e in windows:
        keep |= {r.query_name for r in want.fetch(ref, s, e)}
    _same_reads(got.reads, [r for r in want.reads if r.query_name in keep])


def _golden_cases():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "read_selection.json.gz"), "rt") as fh:
        return json.load(fh)["cases"]


def _sam_to_bam(sam, framing="htslib"):
    from advntr_amd import sam_utils
    refs, recs = [], []
    for line in sam.split("\n"):
        if line.startswith("@SQ"):
            f = dict(x.split(":", 1) for x in line.split("\t")[1:])
            refs.append((f["SN"], int(f["LN"])))
        elif line and not line.startswith("@"):
            f = line.split("\t")
            recs.append((f[0], int(f[1]), f[2], int(f[3]), int(f[4]), f[5], f[9], f[10]))
    assert [r[0] for r in refs] == sam_utils.parse_sam(sam).references
    return bw.write_bam(refs, recs, framing)


@pytest.mark.parametrize("index", [0, 1])
def test_select_illumina_reads_from_bam_matches_reference(tmp_path, index):
    from advntr_amd import bam, settings, vntr_finder
    case = _golden_cases()[index]
    path = tmp_path / "g.bam"
    path.write_bytes(_sam_to_bam(case["sam"]))
    saved = (settings.MAX_ERROR_RATE, settings.USE_TRAINED_HMMS)
    settings.MAX_ERROR_RATE, settings.USE_TRAINED_HMMS = 0.05, False
    try:
        segs = case["repeat_segments"]
        vntr = types.SimpleNamespace(id=3, pattern=case["pattern"], chromosome="chr5", start_point=case["start_point"],
                                     scaled_score=case["scaled_score"], left_flanking_region=case["left"],
                                     right_flanking_region=case["right"], get_repeat_segments=lambda: segs,
                                     get_length=lambda: sum(len(s) for s in segs))
        refs = bam.read_header(str(path))[0]
        samfile = bam.open_alignment(str(path), bam.vntr_windows(refs, [vntr]))
        selected, _ = vntr_finder.select_illumina_reads(vntr, samfile, case["unmapped"])
    finally:
        settings.MAX_ERROR_RATE, settings.USE_TRAINED_HMMS = saved
    want = case["selected"]
    assert [s.sequence for s in selected] == [w["sequence"] for w in want]
    assert [s.logp for s in selected] == [w["logp"] for w in want]
    assert [s.query_name for s in selected] == [w["query_name"] for w in want]
    assert [s.mapq for s in selected] == [w["mapq"] for w in want]
    assert [s.is_mapped for s in selected] == [w["is_mapped"] for w in want]


def _cli(tmp_path, loci_path, aln, *extra):
    out = subprocess.run([sys.executable, "-m", "advntr_amd", "genotype", "--loci", str(loci_path), "--alignment", str(aln)] +
                         list(extra), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    return out.stdout.decode()


@pytest.mark.parametrize("framing", ["htslib", "htsjdk"])
def test_cli_bam_equals_sam_on_golden_case(tmp_path, framing):
    case = _golden_cases()[0]
    loci = [{"id": 3, "left": case["left"], "right": case["right"], "pattern": case["pattern"],
             "repeat_segments": case["repeat_segments"], "scaled_score": None, "chromosome": "chr5",
             "start_point": case["start_point"]}]
    (tmp_path / "loci.json").write_text(json.dumps(loci))
    sam = case["sam"] + "".join("u%d\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t*\n" % (i, s) for i, s in enumerate(case["unmapped"]))
    (tmp_path / "sample.sam").write_text(sam)
    (tmp_path / "bam").mkdir()
    (tmp_path / "bam" / "sample.bam").write_bytes(_sam_to_bam(sam, framing))
    for fmt in ("text", "bed", "vcf"):
        a = _cli(tmp_path, tmp_path / "loci.json", tmp_path / "sample.sam", "--outfmt", fmt)
        b = _cli(tmp_path, tmp_path / "loci.json", tmp_path / "bam" / "sample.bam", "--outfmt", fmt)
        assert a == b
        if fmt == "text":
            assert b == "3\n6/6\n"


def test_cli_bam_equals_sam_on_synthetic_loci(tmp_path):
    from advntr_amd import workloads
    rng = np.random.default_rng(21)
    loci, mapped, unmapped = [], [], []
    for i in range(200):
        loc = workloads.make_locus(rng, flank=150, pattern_len=int(rng.integers(6, 30)), copies=int(rng.integers(2, 6)))
        chrom = "chr%d" % (1 + i % 3)
        start = 10000 + (i // 3) * 3000
        loci.append({"id": 1000 + i, "left": loc.left, "right": loc.right, "pattern": loc.units[0],
                     "repeat_segments": loc.units * loc.copies, "scaled_score": None, "chromosome": chrom, "start_point": start})
        for j, s in enumerate(workloads.make_reads(rng, loc, 6, 150, locus_fraction=0.8)):
            mapped.append(("m%d_%d" % (i, j), 0, chrom, start - 120 + 20 * j, 60, "150M", s, "I" * 150))
        for j, s in enumerate(workloads.make_reads(rng, loc, 3, 150, locus_fraction=0.8)):
            unmapped.append(("u%d_%d" % (i, j), 4, "*", 0, 0, "*", s, "I" * 150))
    mapped.sort(key=lambda r: (r[2], r[3]))
    refs = [("chr1", 10 ** 6), ("chr2", 10 ** 6), ("chr3", 10 ** 6)]
    recs = mapped + unmapped
    (tmp_path / "loci.json").write_text(json.dumps(loci))
    (tmp_path / "sample.sam").write_text(bw.sam_text(refs, recs))
    want = _cli(tmp_path, tmp_path / "loci.json", tmp_path / "sample.sam")
    assert want.count("\n") == 400
    for framing in ("htslib", "htsjdk"):
        (tmp_path / framing).mkdir()
        p = tmp_path / framing / "sample.bam"
        p.write_bytes(bw.write_bam(refs, recs, framing))
        assert _cli(tmp_path, tmp_path / "loci.json", p) == want


def test_cli_refuses_cram_and_plain_gzip(tmp_path):
    (tmp_path / "loci.json").write_text("[]")
    (tmp_path / "a.cram").write_bytes(b"CRAM\3\0" + b"\0" * 30)
    (tmp_path / "a.sam.gz").write_bytes(gzip.compress(b"@HD\tVN:1.6\n"))
    for p, what in (("a.cram", "CRAM"), ("a.sam.gz", "gzip that is not BGZF")):
        out = subprocess.run([sys.executable, "-m", "advntr_amd", "genotype", "--loci", str(tmp_path / "loci.json"),
                              "--alignment", str(tmp_path / p)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             timeout=300)
        assert out.returncode != 0 and what in out.stderr.decode()
