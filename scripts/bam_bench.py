"""BAM input benchmark (not bench.py): one pass of advntr_bam_select over a synthetic BAM in both framings, beside Python's
zlib inflating the same blocks on a thread pool of advntr_host_threads() workers.  Prints one JSON line.

    python scripts/bam_bench.py [--gb 2] [--chunk-mib 256] [--loci 200] [--out bam_bench.json]

The file is a tile of ~64 MiB of coordinate-sorted 150 bp reads (10 % unmapped) repeated until it holds --gb GiB of
uncompressed records; the tile is made to end on a block boundary in both framings, so its compressed blocks are reused:
  htslib: a block is flushed before a record that would not fit (records never span blocks);
  htsjdk: blocks filled to 65 280 bytes, records split anywhere (the boundary walk falls back to the host).
End to end = the genotype command line on --loci synthetic loci placed in the tile, BAM in, genotypes out.
"""
import argparse
import concurrent.futures as cf
import json
import os
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


def tile_records(rng, n_loci, loci_out):
    from advntr_amd import workloads
    recs = []
    pos = 1000
    for i in range(n_loci):          # reads over each locus, then filler reads
        loc = workloads.make_locus(rng, flank=150, pattern_len=int(rng.integers(6, 30)), copies=int(rng.integers(2, 6)))
        loci_out.append({"id": i, "left": loc.left, "right": loc.right, "pattern": loc.units[0],
                         "repeat_segments": loc.units * loc.copies, "scaled_score": None, "chromosome": "chr1",
                         "start_point": pos})
        for j, s in enumerate(workloads.make_reads(rng, loc, 8, 150, locus_fraction=0.8)):
            recs.append(("m%d_%d" % (i, j), 0, "chr1", pos - 120 + 20 * j, 60, "150M", s, "I" * 150))
        pos += 2000
    quals = "".join(chr(33 + q) for q in range(2, 42)) * 5
    n_fill = 200000
    bases = rng.integers(0, 4, (n_fill, 150))
    for k in range(n_fill):
        s = "".join("ACGT"[b] for b in bases[k])
        if k % 10 == 9:
            recs.append(("f%d" % k, 4, "*", 0, 0, "*", s, quals[k % 40:k % 40 + 150]))
        else:
            pos += 3
            recs.append(("f%d" % k, 0, "chr1", pos, 60, "150M", s, quals[k % 40:k % 40 + 150]))
    return recs


def filler(size):
    """An unmapped record of exactly `size` bytes (4 + 32 + name + (L+1)//2 + L)."""
    for ln in range(2, 12):
        for L in range(0, 200000):
            if 36 + ln + (L + 1) // 2 + L == size:
                return bw.bam_record(("p" * (ln - 1), 4, "*", 0, 0, "*", "A" * L if L else "*", "I" * L if L else "*"), {})
    raise ValueError(size)


def compress_blocks(pieces, threads):
    with cf.ThreadPoolExecutor(threads) as ex:
        return list(ex.map(lambda p: bw.bgzf_block(p, 6), pieces))


def make_bam(path, refs, header, tile, framing, copies, threads):
    if framing == "htslib":
        pieces, cur = [], bytearray()
        for r in tile:
            if cur and len(cur) + len(r) > bw.BLOCK_DATA:
                pieces.append(bytes(cur))
                cur = bytearray()
            cur += r
        pieces.append(bytes(cur))
    else:
        data = b"".join(tile)
        pad = -len(data) % bw.BLOCK_DATA
        if pad and pad < 40:
            pad += bw.BLOCK_DATA
        data += filler(pad) if pad else b""
        pieces = [data[i:i + bw.BLOCK_DATA] for i in range(0, len(data), bw.BLOCK_DATA)]
    blocks = compress_blocks(pieces, threads)
    with open(path, "wb") as fh:
        fh.write(bw.bgzf_block(header))
        body = b"".join(blocks)
        for _ in range(copies):
            fh.write(body)
        fh.write(bw.EOF_BLOCK)
    return sum(len(p) for p in pieces) * copies


def zlib_baseline(path, threads):
    from advntr_amd import bam
    data = open(path, "rb").read()
    off, size, isize = bam.scan_framing(data)
    spans = [(int(o), int(s)) for o, s in zip(off, size)]

    def one(span):
        o, s = span
        xlen = int.from_bytes(data[o + 10:o + 12], "little")
        return len(zlib.decompress(data[o + 12 + xlen:o + s - 8], -15))
    t0 = time.perf_counter()
    with cf.ThreadPoolExecutor(threads) as ex:
        total = sum(ex.map(one, spans, chunksize=256))
    dt = time.perf_counter() - t0
    return total / dt / 1e9, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=2.0, help="GiB of uncompressed records")
    ap.add_argument("--chunk-mib", type=int, default=256)
    ap.add_argument("--loci", type=int, default=200)
    ap.add_argument("--out")
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from advntr_amd import _lib, bam
    threads = _lib.load().advntr_host_threads()
    rng = np.random.default_rng(12)
    loci = []
    recs = tile_records(rng, args.loci, loci)
    refs = [("chr1", 10 ** 9)]
    tile = [bw.bam_record(r, {"chr1": 0}) for r in recs]
    tile_bytes = sum(len(r) for r in tile)
    copies = max(1, int(args.gb * 2 ** 30 // tile_bytes))
    header = bw.bam_header(refs, bw.sam_text(refs, []))
    result = {"metric": "bam_input", "gib_uncompressed": None, "host_threads": threads, "chunk_mib": args.chunk_mib}
    tmp = tempfile.mkdtemp(prefix="bam_bench_")
    loci_path = os.path.join(tmp, "loci.json")
    with open(loci_path, "w") as fh:
        json.dump(loci, fh)
    for framing in ("htslib", "htsjdk"):
        path = os.path.join(tmp, "sample_%s.bam" % framing)
        raw = make_bam(path, refs, header, tile, framing, copies, threads)
        result["gib_uncompressed"] = round(raw / 2 ** 30, 3)
        windows = bam.vntr_windows([r[0] for r in refs], [_V(l) for l in loci])
        bam.open_alignment(path, windows, chunk_bytes=args.chunk_mib << 20)          # warm-up (page cache, device init)
        t0 = time.perf_counter()
        f = bam.open_alignment(path, windows, chunk_bytes=args.chunk_mib << 20)
        wall = time.perf_counter() - t0
        s = f.stats
        out = s["uncompressed_bytes"] / 1e9
        cpu_gbs, cpu_s = zlib_baseline(path, threads)
        t0 = time.perf_counter()
        cli = subprocess.run([sys.executable, "-m", "advntr_amd", "genotype", "--loci", loci_path, "--alignment", path],
                             cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        e2e = time.perf_counter() - t0
        result[framing] = {
            "compressed_gb": round(s["compressed_bytes"] / 1e9, 3), "blocks": int(s["blocks"]), "records": int(s["records"]),
            "kept": int(s["kept"]), "chunks": int(s["chunks"]),
            "file_read_s": round(s["read_ms"] / 1e3, 3), "framing_scan_s": round(s["framing_ms"] / 1e3, 3),
            "upload_s": round(s["upload_ms"] / 1e3, 3), "inflate_kernel_s": round(s["inflate_kernel_ms"] / 1e3, 3),
            "inflate_gbps_kernel": round(out / (s["inflate_kernel_ms"] / 1e3), 2),
            "inflate_gbps_pcie_inclusive": round(out / ((s["inflate_kernel_ms"] + s["upload_ms"]) / 1e3), 2),
            "boundary_s": round(s["boundary_ms"] / 1e3, 3),
            "boundary_path": "device" if s["fallback_blocks"] == 0 else "host fallback (%d blocks)" % s["fallback_blocks"],
            "fallback_s": round(s["fallback_ms"] / 1e3, 3),
            "select_s": round(s["select_ms"] / 1e3, 3), "select_records_per_s": round(s["records"] / (s["select_ms"] / 1e3)),
            "pass_s": round(wall, 3), "pass_gbps": round(out / wall, 2),
            "cpu_zlib_gbps": round(cpu_gbs, 2), "cpu_zlib_s": round(cpu_s, 3),
            "end_to_end_genotypes_s": round(e2e, 3), "genotype_rc": cli.returncode,
            "genotyped_loci": cli.stdout.decode().count("\n") // 2,
        }
        os.remove(path)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


class _V(object):
    def __init__(self, loc):
        self.chromosome, self.start_point = loc["chromosome"], loc["start_point"]
        self._len = sum(len(s) for s in loc["repeat_segments"])

    def get_length(self):
        return self._len


if __name__ == "__main__":
    main()
