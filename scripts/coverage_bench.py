"""Coverage-window benchmark (not bench.py): the BAM pass of advntr_bam_select with and without ADVNTR_BAM_COVERAGE over a synthetic
~30x BAM, the scan, GC and binning kernels on a synthetic genome, and `genotype --expansion -c auto` end to end.  Prints one
JSON line.

    python scripts/coverage_bench.py [--gib 2] [--depth 30] [--chroms 4] [--out coverage_bench.json]

Records are 150-bp reads with a 150M CIGAR (277 bytes each), coordinate-sorted, uniform over --chroms chromosomes sized so
that --gib GiB of uncompressed records give --depth; sequence and quality bytes come from one random tile, so only refID, POS
and bin differ between records.  Blocks are htslib-framed and compressed with zlib level 1 on 16 threads.  Each pass runs
twice; the second is reported.
"""
import argparse
import concurrent.futures as cf
import json
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bam_writer as bw  # noqa: E402

READ, NAME = 150, 12
REC = 4 + 32 + NAME + 4 + (READ + 1) // 2 + READ


def records(rng, ref, pos):
    """uncompressed bytes of len(pos) records on reference `ref` at 0-based positions pos (sorted)"""
    n = len(pos)
    a = np.zeros((n, REC), np.uint8)
    head = np.zeros(n, dtype=np.dtype([("bs", "<i4"), ("ref", "<i4"), ("pos", "<i4"), ("ln", "u1"), ("mapq", "u1"), ("bin", "<u2"),
                                       ("ncig", "<u2"), ("flag", "<u2"), ("lseq", "<i4"), ("nref", "<i4"), ("npos", "<i4"), ("tlen", "<i4")]))
    head["bs"], head["ref"], head["pos"], head["ln"], head["mapq"] = REC - 4, ref, pos, NAME, 60
    head["bin"] = 4681 + (pos >> 14)                    # reg2bin of a 150-bp read that stays in one 16-kb bin
    head["ncig"], head["flag"], head["lseq"], head["nref"], head["npos"] = 1, 0, READ, -1, -1
    a[:, :36] = head.view(np.uint8).reshape(n, 36)
    a[:, 36:36 + NAME - 1] = np.frombuffer(b"read0000000", np.uint8)
    a[:, 36 + NAME:40 + NAME] = np.frombuffer(struct.pack("<I", READ << 4), np.uint8)
    tile = rng.integers(0, 256, (4096, (READ + 1) // 2 + READ), dtype=np.uint8)
    tile[:, (READ + 1) // 2:] = rng.integers(2, 41, (4096, READ), dtype=np.uint8)
    a[:, 40 + NAME:] = tile[np.arange(n) % 4096]
    return a.reshape(-1)


def write_bam(path, rng, gib, depth, n_chroms):
    n_rec = int(gib * (1 << 30) // REC)
    length = int(n_rec * READ // depth // n_chroms) // 100 * 100
    refs = [("chr%d" % (c + 1), length) for c in range(n_chroms)]
    header = bw.bam_header(refs, bw.sam_text(refs, []))
    per = n_rec // n_chroms
    recs_per_block = bw.BLOCK_DATA // REC
    with open(path, "wb") as fh, cf.ThreadPoolExecutor(16) as pool:
        fh.write(bw.bgzf_block(header, 1))
        for c in range(n_chroms):
            pos = np.sort(rng.integers(0, length - READ, per)).astype(np.int32)
            raw = records(rng, c, pos)
            pieces = [raw[i * REC:(i + recs_per_block) * REC].tobytes() for i in range(0, per, recs_per_block)]
            for blk in pool.map(lambda p: bw.bgzf_block(p, 1), pieces):
                fh.write(blk)
        fh.write(bw.EOF_BLOCK)
    return refs, per * n_chroms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--chroms", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from advntr_amd import _lib, bam, genome
    _lib.require_gpu()
    rng = np.random.default_rng(1)
    tmp = tempfile.mkdtemp(prefix="coverage_bench_")
    path = os.path.join(tmp, "sample.bam")
    t0 = time.perf_counter()
    refs, n_rec = write_bam(path, rng, args.gib, args.depth, args.chroms)
    gen_s = time.perf_counter() - t0
    # a synthetic genome of the header's lengths (upper case, 10 % soft-masked)
    t0 = time.perf_counter()
    chroms = {}
    for name, length in refs:
        codes = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, length)]
        codes = np.where(rng.random(length) < 0.1, codes | 0x20, codes).astype(np.uint8)
        chroms[name] = genome.Chromosome(name, codes)
    gen = genome.Genome(chroms, 0.0)
    fasta = os.path.join(tmp, "genome.fa")
    with open(fasta, "wb") as fh:
        for name, c in chroms.items():
            fh.write(b">" + name.encode() + b"\n" + c.codes.tobytes() + b"\n")
    genome_s = time.perf_counter() - t0

    def timed(**kw):
        out = None
        for _ in range(2):
            t = time.perf_counter()
            out = bam.open_alignment(path, [], **kw)
            wall = time.perf_counter() - t
        return out, wall

    plain, plain_s = timed()
    cov, cov_s = timed(coverage=True)
    covg, covg_s = timed(coverage=True, genome=gen)
    # genotype --expansion -c auto end to end: 20 loci on chr1 (random sequence; the timing is the point)
    loci = []
    for i in range(20):
        dna = "".join("ACGT"[b] for b in rng.integers(0, 4, 1060))
        loci.append({"id": i, "left": dna[:500], "right": dna[560:], "pattern": dna[500:530], "repeat_segments": [dna[500:530], dna[530:560]],
                     "scaled_score": None, "chromosome": "chr1", "start_point": 100000 + 50000 * i})
    with open(os.path.join(tmp, "loci.json"), "w") as fh:
        json.dump(loci, fh)
    walls = {}
    for key, extra in (("genotype_s", []), ("genotype_expansion_auto_s", ["-e", "-c", "auto"]),
                       ("genotype_expansion_auto_gc_s", ["-e", "-c", "auto", "-r", fasta])):
        t = time.perf_counter()
        p = subprocess.run([sys.executable, "-m", "advntr_amd", "genotype", "--loci", os.path.join(tmp, "loci.json"), "--alignment", path]
                           + extra, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1800)
        walls[key] = round(time.perf_counter() - t, 3)
        if p.returncode:
            raise SystemExit(p.stderr.decode()[-2000:])
    st = covg.coverage.stats
    line = {"bench": "coverage", "gib_uncompressed": round(plain.stats["uncompressed_bytes"] / (1 << 30), 3),
            "compressed_gib": round(os.path.getsize(path) / (1 << 30), 3), "records": n_rec, "chroms": len(refs),
            "chrom_len": refs[0][1], "depth": args.depth, "generate_s": round(gen_s, 2), "genome_s": round(genome_s, 2),
            "pass_s": round(plain_s, 3), "pass_coverage_s": round(cov_s, 3), "pass_coverage_gc_s": round(covg_s, 3),
            "inflate_kernel_ms": round(plain.stats["inflate_kernel_ms"], 2),
            "inflate_kernel_coverage_ms": round(cov.stats["inflate_kernel_ms"], 2),
            "select_ms": round(plain.stats["select_ms"], 2), "select_coverage_ms": round(cov.stats["select_ms"], 2),
            "accumulate_kernel_ms": round(cov.coverage.stats["accumulate_kernel_ms"], 3),
            "scan_kernel_ms": round(cov.coverage.stats["scan_kernel_ms"], 3),
            "bins_kernel_ms": round(cov.coverage.stats["bins_kernel_ms"], 3),
            "gc_kernel_ms": round(st["gc_kernel_ms"], 3), "chrom_upload_ms": round(st["chrom_upload_ms"], 2),
            "bins_gc_kernel_ms": round(st["bins_kernel_ms"], 3), "windows": int(st["windows"]),
            "sequencing_mean": round(cov.coverage.corrector.get_sequencing_mean_coverage(), 4),
            "accumulate_vs_inflate": round(cov.coverage.stats["accumulate_kernel_ms"] / max(1e-9, cov.stats["inflate_kernel_ms"]), 4)}
    line.update(walls)
    s = json.dumps(line)
    print(s)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(s + "\n")
    for f in os.listdir(tmp):
        os.remove(os.path.join(tmp, f))
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
