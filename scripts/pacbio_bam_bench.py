"""Aligned long-read BAM benchmark (not bench.py): one pass of advntr_bam_select_spans over a config-5-shaped file, and the
`genotype --pacbio --alignment` command line on it.  Prints one JSON line.

    python scripts/pacbio_bam_bench.py [--loci 8960] [--reads 20] [--unmapped-loci 64] [--chunk-mib 256] [--out FILE]

Loci are drawn as workloads.make_pacbio_whole_reads draws them (10-60 bp pattern, 100-1000 bp of repeat) and laid out on
one reference; each gets --reads error-free mapped reads of U(5 000, 15 000) bases from one of its two haplotypes, whose
CIGARs carry the expansion or contraction as an I or D op.  The whole reads of --unmapped-loci loci from
make_pacbio_whole_reads follow as unmapped records.  Reported: inflate / select / span-kernel ms, the trimmed bytes against
the bytes a whole decode of the same records would make, and the end-to-end wall time of the command line.
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

_NIB = np.zeros(256, np.uint8)
for _i, _c in enumerate("=ACMGRSVTWYHKDBN"):
    _NIB[ord(_c)] = _i
_OPS = {"M": 0, "I": 1, "D": 2}


def record(name, flag, ref, pos, ops, seq):
    """one BAM record (qualities absent: 0xFF), the sequence packed with numpy"""
    s = np.frombuffer(seq.encode(), np.uint8)
    codes = _NIB[s]
    if len(codes) % 2:
        codes = np.append(codes, 0)
    packed = (codes[0::2] << 4 | codes[1::2]).astype(np.uint8).tobytes()
    span = sum(n for n, op in ops if op in "MD")
    nm = name.encode() + b"\0"
    b = bw.reg2bin(max(pos, 0), max(pos + max(span, 1), 1)) if ref >= 0 else 4680
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(nm), 60 if ref >= 0 else 0, b, len(ops), flag, len(seq), -1, -1, 0)
    body += nm + b"".join(struct.pack("<I", n << 4 | _OPS[op]) for n, op in ops) + packed + b"\xff" * len(seq)
    return struct.pack("<i", len(body)) + body


def make(args, rng):
    from advntr_amd import workloads
    loci, recs, at = [], [], 20000
    for k in range(args.loci):
        plen = int(rng.integers(10, 61))
        ref_copies = max(2, int(round(int(rng.integers(100, 1001)) / plen)))
        left, right, pattern = workloads.rand_seq(rng, 8000), workloads.rand_seq(rng, 8000), workloads.rand_seq(rng, plen)
        vs = at + len(left)
        loci.append({"id": k, "left": left[-500:], "right": right[:500], "pattern": pattern,
                     "repeat_segments": [pattern] * ref_copies, "scaled_score": None, "chromosome": "chr1", "start_point": vs})
        haps = [max(1, int(round(ref_copies * (0.8 + 0.4 * rng.random())))) for _ in range(2)]
        for j in range(args.reads):
            c = haps[j % 2]
            n = int(rng.integers(5000, 15001))
            la = int(rng.integers(150, max(151, min(len(left), n - c * plen - 150))))
            lb = max(150, min(len(right), n - la - c * plen))
            seq = left[-la:] + pattern * c + right[:lb]
            if c > ref_copies:
                ops = [(la + ref_copies * plen, "M"), ((c - ref_copies) * plen, "I"), (lb, "M")]
            elif c < ref_copies:
                ops = [(la + c * plen, "M"), ((ref_copies - c) * plen, "D"), (lb, "M")]
            else:
                ops = [(len(seq), "M")]
            recs.append((vs - la, record("m%d_%d" % (k, j), 0, 0, vs - la, ops, seq)))
        at = vs + ref_copies * plen + len(right)
    recs.sort(key=lambda t: t[0])
    out = [r for _, r in recs]
    _, whole = workloads.make_pacbio_whole_reads(args.unmapped_loci, seed=20240603, n_reads=args.reads, workers=16)
    for k, reads in enumerate(whole):
        for j, s in enumerate(reads):
            out.append(record("u%d_%d" % (k, j), 4, -1, -1, [], s))
    return loci, at + 20000, out


def write(path, length, recs, workers=16):
    """htslib framing (a block is flushed before a record that does not fit; long records span blocks), compressed in parallel"""
    head = bw.bam_header([("chr1", length)], bw.sam_text([("chr1", length)], []))
    pieces, cur = [head], bytearray()
    for r in recs:
        if cur and len(cur) + len(r) > bw.BLOCK_DATA:
            pieces.append(bytes(cur))
            cur = bytearray()
        cur += r
        while len(cur) > bw.BLOCK_DATA:
            pieces.append(bytes(cur[:bw.BLOCK_DATA]))
            del cur[:bw.BLOCK_DATA]
    if cur:
        pieces.append(bytes(cur))
    with cf.ThreadPoolExecutor(workers) as ex, open(path, "wb") as fh:
        for blk in ex.map(lambda p: bw.bgzf_block(p, 1), pieces, chunksize=64):
            fh.write(blk)
        fh.write(bw.EOF_BLOCK)
    return sum(len(p) for p in pieces)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=8960)
    ap.add_argument("--reads", type=int, default=20)
    ap.add_argument("--unmapped-loci", type=int, default=64)
    ap.add_argument("--chunk-mib", type=int, default=256)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from advntr_amd import bam
    rng = np.random.default_rng(20240611)
    t = time.perf_counter()
    loci, length, recs = make(args, rng)
    tmp = tempfile.mkdtemp(prefix="pacbio_bam_")
    path = os.path.join(tmp, "sample.bam")
    raw_bytes = write(path, length, recs)
    gen_s = time.perf_counter() - t
    windows = [("chr1", l["start_point"], l["start_point"] + len("".join(l["repeat_segments"])), i) for i, l in enumerate(loci)]
    bam.open_alignment_spans(path, windows[:1], chunk_bytes=args.chunk_mib << 20)         # warm-up (device, code objects)
    t = time.perf_counter()
    got = bam.open_alignment_spans(path, windows, chunk_bytes=args.chunk_mib << 20)
    pass_s = time.perf_counter() - t
    st = got.stats
    res = {"loci": args.loci, "mapped_reads": args.loci * args.reads, "unmapped_reads": len(got.unmapped),
           "compressed_bytes": os.path.getsize(path), "uncompressed_bytes": raw_bytes, "generate_s": round(gen_s, 1),
           "pass_wall_ms": round(1000 * pass_s, 1),
           "inflate_kernel_ms": round(st["inflate_kernel_ms"], 2), "select_ms": round(st["select_ms"], 2),
           "span_kernel_ms": round(st["span_kernel_ms"], 3), "trim_kernel_ms": round(st["trim_kernel_ms"], 3),
           "boundary_ms": round(st["boundary_ms"], 2), "read_ms": round(st["read_ms"], 2), "total_ms": round(st["total_ms"], 2),
           "pairs": int(st["pairs"]), "spanning": int(st["spanning"]), "trimmed_bytes": int(st["trimmed_bytes"]),
           "whole_decode_bytes": int(st["whole_bytes"]), "unmapped_bytes": int(st["unmapped_bytes"])}
    if not args.no_cli:
        with open(os.path.join(tmp, "loci.json"), "w") as fh:
            json.dump(loci, fh)
        t = time.perf_counter()
        out = subprocess.run([sys.executable, "-m", "advntr_amd", "genotype", "--loci", os.path.join(tmp, "loci.json"),
                              "--alignment", path, "--pacbio"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        res["cli_wall_s"] = round(time.perf_counter() - t, 2)
        res["cli_rc"] = out.returncode
        lines = out.stdout.decode().split("\n")[1::2]
        res["cli_called"] = sum(1 for l in lines if l and l != "None")
        if out.returncode:
            res["cli_stderr"] = out.stderr.decode()[-500:]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
