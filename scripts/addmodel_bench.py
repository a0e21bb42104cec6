#!/usr/bin/env python3
"""Time `addmodel` at genome scale: a synthetic genome of --gb gigabases (24 chromosomes, ~3 % N in runs, planted loci with
decoys around each, 5 % of the loci low-complexity poly-A), all loci trained in one batch, one JSON line with the stages.
Also times one locus through the device scan and through the numpy mirror (vntr_extras.simulate_false_filtered_reads) on a
chromosome of --mirror-mb megabases, and checks that both give the same reads.

    python scripts/addmodel_bench.py [--gb 3.1] [--loci 1000] [--mirror-mb 48]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_ACGT = np.frombuffer(b"ACGT", np.uint8)


def _dna(rng, n):
    return _ACGT[rng.integers(0, 4, n, dtype=np.uint8)]


def make_chromosome(rng, n, loci_here, low_flags):
    """uint8 text of n bases: random, N runs making ~3 %, the loci planted (returned as rows) with 3-6 decoys each."""
    s = _dna(rng, n)
    n_runs = max(1, n // 100000)
    for at in rng.integers(0, n, n_runs):
        s[at:at + int(rng.integers(1000, 5000))] = ord("N")
    rows = []
    slot = n // (loci_here + 1)
    for k in range(loci_here):
        low = low_flags[k]
        pattern = (b"A" * 12 + b"C") if low else _dna(rng, int(rng.integers(6, 60))).tobytes()
        unit = np.frombuffer(pattern, np.uint8)
        vntr = np.concatenate([unit.copy() for _ in range(int(rng.integers(3, 10)))])
        start = slot * (k + 1)
        for _ in range(int(rng.integers(3, 7))):
            piece = np.resize(vntr, int(rng.integers(60, 150))).copy()
            piece[rng.integers(0, len(piece), 2)] = _dna(rng, 2)
            at = start + int(rng.choice([-1, 1])) * int(rng.integers(2000, 20000))
            if 0 <= at and at + len(piece) < n:
                s[at:at + len(piece)] = piece
        s[start - 700:start + len(vntr) + 700] = np.concatenate([_dna(rng, 700), vntr, _dna(rng, 700)])
        if low:
            for at in rng.integers(0, n, max(1, n // 2000000)):
                s[at:at + 30] = ord("A")
        rows.append((start, start + len(vntr), pattern.decode()))
    return s, rows


def write_genome(path, gb, n_loci, seed=1):
    rng = np.random.default_rng(seed)
    weights = np.linspace(2.0, 0.5, 24)
    sizes = (weights / weights.sum() * gb * 1e9).astype(np.int64)
    per = np.full(24, n_loci // 24)
    per[:n_loci % 24] += 1
    low = rng.random(n_loci) < 0.05
    rows, k = [], 0
    with open(path, "wb") as fh:
        for c in range(24):
            name = "chr%d" % (c + 1)
            s, here = make_chromosome(rng, int(sizes[c]), int(per[c]), low[k:k + per[c]])
            k += per[c]
            rows += [(name, a, b, p, "%s locus %d" % (name, i)) for i, (a, b, p) in enumerate(here)]
            fh.write((">%s synthetic\n" % name).encode())
            width = 60
            full = len(s) // width
            block = np.empty((full, width + 1), np.uint8)
            block[:, :width] = s[:full * width].reshape(full, width)
            block[:, width] = 10
            fh.write(block.tobytes())
            fh.write(s[full * width:].tobytes() + b"\n")
    return rows


def mirror_comparison(mb, seed=2):
    from advntr_amd import training, vntr_extras
    from types import SimpleNamespace
    rng = np.random.default_rng(seed)
    s, rows = make_chromosome(rng, int(mb * 1e6), 1, [False])
    start, end, pattern = rows[0]
    text = s.tobytes().decode("latin-1")
    segs = [pattern] * ((end - start) // len(pattern))
    v = SimpleNamespace(id=1, pattern=pattern, chromosome="chrM", start_point=start, scaled_score=0,
                        left_flanking_region=text[start - 500:start], right_flanking_region=text[end:end + 500],
                        get_repeat_segments=lambda: segs, get_length=lambda: end - start)
    training.scan_false_reads(s[:1 << 20], [v])                           # warm-up: library, device, caches
    t = time.perf_counter()
    spans, st = training.scan_false_reads(s, [v])
    t_dev = time.perf_counter() - t
    t = time.perf_counter()
    want = vntr_extras.simulate_false_filtered_reads(v, [("chrM", text)])
    t_mirror = time.perf_counter() - t
    same = training.false_read_texts(s, spans[0]) == want
    return {"mirror_mb": mb, "device_route_s": round(t_dev, 4), "device_kernel_ms": round(st["kernel_ms"], 3),
            "mirror_s": round(t_mirror, 3), "speedup": round(t_mirror / t_dev, 1), "reads": len(want), "identical": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=3.1)
    ap.add_argument("--loci", type=int, default=1000)
    ap.add_argument("--mirror-mb", type=float, default=48)
    ap.add_argument("--keep", help="directory for the genome and database (default: a temporary one, removed)")
    args = ap.parse_args()
    from advntr_amd import _lib, genome, settings, training
    _lib.require_gpu()
    settings.ALIGN_REPEATS = True            # loci whose units the repeat finder cuts unequally are aligned, not refused
    work = args.keep or tempfile.mkdtemp(prefix="addmodel_bench_")
    fa, db = os.path.join(work, "genome.fa"), os.path.join(work, "models.db")
    if os.path.exists(db):
        os.unlink(db)
    t = time.perf_counter()
    rows = write_genome(fa, args.gb, args.loci)
    t_gen = time.perf_counter() - t
    t_all = time.perf_counter()
    ref = genome.read_genome(fa)
    tm = {}
    vntrs = training.add_models(ref, rows, db, timings=tm)
    wall = time.perf_counter() - t_all
    scan = tm["scan"]
    out = {
        "bench": "addmodel", "gb": args.gb, "bases": ref.total_bases(), "loci": len(vntrs), "generate_s": round(t_gen, 2),
        "fasta_read_s": round(ref.seconds, 3),
        "init_loci_s": round(tm["init_loci"], 3),
        "upload_ms": round(scan["upload_ms"], 2),
        "scan_kernel_ms": round(scan["kernel_ms"], 3),
        "scan_gbps": round(scan["bytes"] / (scan["kernel_ms"] * 1e-3) / 1e9, 1) if scan["kernel_ms"] else None,
        "scan_hits": int(scan["hits"]), "scan_chunks": int(scan["chunks"]),
        "triple_rule_ms": round(scan["fold_ms"], 2),
        "scan_total_s": round(tm["false_reads"], 3),
        "true_reads_s": round(tm["true_reads"], 3),
        "model_build_s": round(tm["model_build"], 3),
        "encode_s": round(tm["encode"], 3),
        "scoring_s": round(tm["scoring"], 3), "reads_scored": tm["reads_scored"],
        "classifier_s": round(tm["classifier"], 3),
        "db_write_s": round(tm["db_write"], 4),
        "total_wall_s": round(wall, 2),
    }
    if not args.keep:
        os.unlink(fa)
        os.unlink(db)
        os.rmdir(work)
    out["one_locus"] = mirror_comparison(args.mirror_mb)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
