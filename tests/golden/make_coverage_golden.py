#!/usr/bin/env python3
"""Generate tests/golden/coverage.json.gz by RUNNING THE REFERENCE: advntr/coverage_bias.py and advntr/utils.py are compiled at
run time (pysam and Bio.SeqIO stubbed in sys.modules, advntr.settings loaded from the reference's file), nothing of them stored.
TEST INFRASTRUCTURE; only data is written.

The reference's loaders cannot run under Python 3 (a float window number from `/`, `range` of a float, a crash on unplaced
records), so the two loaders are replaced by the loops they run, with integer window numbers:
  - covered bases: get_covered_base_pairs_of_reference_windows's body over synthetic records (the 'chr' prefix, the
    CHROMOSOMES test, `reference_end or reference_start + len(seq)`), each record handed to the real private
    __add_bp_to_coverage_map.  Windows past a chromosome's last full window, where the reference raises KeyError later,
    are dropped from the map before it is used: the project's stated rule;
  - GC: the real get_gc_content on every full window of the mixed-case chromosome text;
and the real get_gc_content_coverage_map runs with the loaders patched to return those maps.  Then CoverageCorrector's
means and get_scaled_coverage.

    python tests/golden/make_coverage_golden.py
"""
import ast
import gzip
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("ADVNTR_REFERENCE", "/root/reference")


def _load_reference():
    """(coverage_bias namespace, settings module, get_gc_content) compiled from the reference's files"""
    for name in ("pysam", "Bio", "Bio.SeqIO"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["Bio"].SeqIO = sys.modules["Bio.SeqIO"]
    settings = types.ModuleType("advntr.settings")
    path = os.path.join(REF, "advntr", "settings.py")
    exec(compile(open(path).read(), path, "exec"), vars(settings))
    # advntr.utils: the two functions coverage_bias imports, compiled from the reference's file
    utils = types.ModuleType("advntr.utils")
    vars(utils).update({k: v for k, v in vars(settings).items() if not k.startswith("__")})
    path = os.path.join(REF, "advntr", "utils.py")
    tree = ast.parse(open(path).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("get_gc_content", "get_chromosome_reference_sequence")]
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), vars(utils))
    advntr = types.ModuleType("advntr")
    advntr.settings, advntr.utils = settings, utils
    sys.modules.update({"advntr": advntr, "advntr.settings": settings, "advntr.utils": utils})
    path = os.path.join(REF, "advntr", "coverage_bias.py")
    cb = {"__name__": "coverage_bias"}
    exec(compile(open(path).read(), path, "exec"), cb)
    return cb, settings, utils.get_gc_content


class _Read(object):
    def __init__(self, name, start, end, seq):
        self.reference_name, self.reference_start, self.reference_end, self.seq = name, start, end, seq


def main():
    cb, settings, get_gc_content = _load_reference()
    W = settings.GC_CONTENT_WINDOW_SIZE
    rng = np.random.default_rng(2024)

    def text(n, gc_bias):
        p = np.array([(1 - gc_bias) / 2, gc_bias / 2, gc_bias / 2, (1 - gc_bias) / 2])
        s = np.array(list("ACGT"))[rng.choice(4, n, p=p)]
        lower = rng.random(n) < 0.15                          # soft-masked stretches: lower case
        s = np.where(lower, np.char.lower(s), s)
        return "".join(s.tolist())

    # header references: '1' counts as chr1, chrX as itself; chrUn_x and chrM are not among settings.CHROMOSOMES
    genome = {"chr1": "".join(text(1000, g) for g in (0.2, 0.5, 0.8, 0.35, 0.65, 0.5, 0.3, 0.7)) + text(57, 0.5),
              "chr2": text(6000, 0.45) + text(30, 0.5),
              "chrX": text(4000, 0.55),
              "chrUn_x": text(3000, 0.5), "chrM": text(1600, 0.5)}
    header = [("1", len(genome["chr1"])), ("chr2", len(genome["chr2"])), ("chrX", len(genome["chrX"])),
              ("chrUn_x", len(genome["chrUn_x"])), ("chrM", len(genome["chrM"]))]
    reads = []                                        # [reference name, reference_start, reference_end or None, len(seq)]
    for name, length in header:
        hi = 4000 if name == "chr2" else length       # chr2 keeps windows 40-59 for the zero-length records below
        for _ in range(int(hi * 30 / 150)):           # ~30x of 150-bp reads
            s = int(rng.integers(0, hi - 10))
            kind = rng.random()
            if kind < 0.85:
                reads.append([name, s, min(length, s + int(rng.integers(100, 160))), 150])
            elif kind < 0.92:                           # no reference end (unmapped placed): start + len(seq)
                reads.append([name, s, None, int(rng.integers(1, 250))])
            elif kind < 0.96:                           # a CIGAR without reference bases: zero length
                reads.append([name, s, s, 150])
            else:                                       # long reads, past the last full window too
                e = s + int(rng.integers(2000, 15000))
                reads.append([name, s, min(e, hi) if hi < length else e, 15000])
    reads.append(["1", 0, 0, 120])                    # reference_end 0 is falsy: start + len(seq)
    reads.append(["chr2", 5050, None, 0])             # no end, empty sequence: zero length, window 50 present with 0 bp
    reads.append(["chr2", 5500, 5500, 0])             # window 55 present with 0 bp
    reads.append(["chr2", 5900, 6100, 200])           # past the last full window (59) of chr2
    for k in range(260):                              # windows above 200x on chrX (261 x 100 bp = 26 100 bp > 20 000)
        reads.append(["chrX", 2000, 2100, 100])
    for k in range(190):                              # near 200x on windows 22 and 23
        reads.append(["chrX", 2250, 2350, 100])

    detector = cb["CoverageBiasDetector"]("sample.bam")
    add = detector._CoverageBiasDetector__add_bp_to_coverage_map
    covered_bps = {c: {} for c in settings.CHROMOSOMES}
    for name, s, e, seq_len in reads:                 # get_covered_base_pairs_of_reference_windows, integer windows
        read = _Read(name, s, e, "A" * seq_len)
        window_number = read.reference_start // W
        read_start = read.reference_start
        read_end = read.reference_end if read.reference_end else read_start + len(read.seq)
        reference_name = read.reference_name
        if not reference_name.startswith('chr'):
            reference_name = 'chr' + reference_name
        if reference_name in covered_bps.keys():
            add(covered_bps, reference_name, window_number, read_start, read_end)
    for c in covered_bps:                             # past the last full window (KeyError in the reference): dropped
        full = len(genome.get(c, "")) // W
        covered_bps[c] = {w: bp for w, bp in covered_bps[c].items() if w < full}
    gc_map = {c: {w: get_gc_content(genome[c][w * W:w * W + W]) for w in range(len(genome[c]) // W)} if c in genome else {}
              for c in settings.CHROMOSOMES}
    detector.get_gc_contents_of_reference_windows = lambda: gc_map
    detector.get_covered_base_pairs_of_reference_windows = lambda: covered_bps
    gc_coverage_map = detector.get_gc_content_coverage_map()
    corrector = cb["CoverageCorrector"](gc_coverage_map)

    class _Vntr(object):
        def __init__(self, segments):
            self.segments = segments

        def get_repeat_segments(self):
            return self.segments

    vntrs = [["GGCCAATT"], ["GCGCGCAT", "GCGCGCAA"], ["ATATATAG"], ["GGGCCCGCGA"], ["GCAT", "GCTA", "ATTA"], ["gGcCAATT"]]
    scaled, by_gc = [], []
    for segs in vntrs:
        gc = get_gc_content("".join(segs))
        b = corrector.get_gc_bin_index(gc)
        if b in gc_coverage_map:
            by_gc.append([segs, gc, b, corrector.get_mean_coverage_of_gc_content(gc)])
            scaled.append([segs, 37.5, corrector.get_scaled_coverage(_Vntr(segs), 37.5)])
        else:
            by_gc.append([segs, gc, b, None])
    out = {"header": header, "genome": genome, "reads": reads,
           "covered_bps": {c: sorted([int(w), int(bp)] for w, bp in m.items()) for c, m in covered_bps.items() if m},
           "gc_coverage_map": {str(k): v for k, v in sorted(gc_coverage_map.items())},
           "sequencing_mean": corrector.get_sequencing_mean_coverage(), "by_gc": by_gc, "scaled": scaled}
    assert any(segs == ["GGCCAATT"] and b == 4 for segs, gc, b, _ in by_gc), "a VNTR at GC 0.5 exactly (bin 4)"
    path = os.path.join(HERE, "coverage.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, sort_keys=True).encode())
    print("wrote %s: %d reads, %d windows binned, sequencing mean %.6f" %
          (path, len(reads), sum(len(v) for v in gc_coverage_map.values()), out["sequencing_mean"]))


if __name__ == "__main__":
    main()
