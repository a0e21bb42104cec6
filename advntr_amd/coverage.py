"""Sequencing coverage per GC bin for `genotype --expansion -c auto`: the counterpart of the reference's CoverageBiasDetector
and CoverageCorrector (advntr/coverage_bias.py), built from exact integer bins.

The rule (csrc/coverage_windows.h says it in full): every record of the alignment on chr1-chr22, chrX or chrY (a 'chr' prefix
is added to a name without one) adds its [pos, end) interval to the 100-bp windows it reaches; a window reached by any record
is present; a present window with coverage (bp / 100) above 200 is left out; the others go to GC bin gc // 10, gc = the
uppercase G and C bases of the window in the reference genome (soft-masked bases do not count, as get_gc_content on the
unmodified text), or all to one bin without a genome.  For BAM input the windows are summed on the device in the same pass
that selects the reads (bam.open_alignment(..., coverage=True)); for SAM text the intervals are made here and summed by the
host twin of the device code.
"""
import ctypes
import sys

import numpy as np

from . import _lib

CHROMOSOMES = ['chr' + str(n) for n in range(1, 23)] + ['chrX', 'chrY']     # settings.CHROMOSOMES
GC_CONTENT_WINDOW_SIZE = 100
GC_CONTENT_BINS = 10
OUTLIER_COVERAGE = 200
BINS = _lib.COVERAGE_BINS


def counted_chromosome(reference_name):
    """The chromosome a record of `reference_name` counts for (coverage_bias.py:67-70), or None."""
    name = reference_name if reference_name.startswith('chr') else 'chr' + reference_name
    return name if name in CHROMOSOMES else None


def get_gc_content(s):
    """utils.get_gc_content: the fraction of uppercase 'G' and 'C' characters."""
    res = 0
    for e in s:
        if e == 'G' or e == 'C':
            res += 1
    return float(res) / len(s)


class CoverageCorrector(object):
    """CoverageCorrector (coverage_bias.py:94-125) over integer bins: bin_windows[b] windows whose covered bases sum to
    bin_bp[b].  A mean is that sum / 100 / the count, in double precision."""

    def __init__(self, bin_windows, bin_bp):
        self.bin_windows = [int(x) for x in bin_windows]
        self.bin_bp = [int(x) for x in bin_bp]

    @staticmethod
    def get_gc_bin_index(gc_content):
        return int(gc_content * GC_CONTENT_BINS - sys.float_info.epsilon * 10)

    def windows(self):
        return sum(self.bin_windows)

    def get_sequencing_mean_coverage(self):
        n = self.windows()
        if not n:
            raise ValueError("no coverage window was measured")
        return sum(self.bin_bp) / float(GC_CONTENT_WINDOW_SIZE) / n

    def has_gc_bin(self, gc_content):
        b = self.get_gc_bin_index(gc_content)
        return 0 <= b < len(self.bin_windows) and self.bin_windows[b] > 0

    def get_mean_coverage_of_gc_content(self, gc_content):
        b = self.get_gc_bin_index(gc_content)
        if not self.has_gc_bin(gc_content):
            raise KeyError(b)       # the reference's dict lookup of an empty bin
        return self.bin_bp[b] / float(GC_CONTENT_WINDOW_SIZE) / self.bin_windows[b]

    def get_scaled_coverage(self, reference_vntr, observed_coverage):
        gc_content = get_gc_content(''.join(reference_vntr.get_repeat_segments()))
        return observed_coverage * (self.get_sequencing_mean_coverage() / self.get_mean_coverage_of_gc_content(gc_content))

    def bins(self):
        """[(windows, mean coverage or None)] per bin"""
        return [(w, (bp / float(GC_CONTENT_WINDOW_SIZE) / w) if w else None) for w, bp in zip(self.bin_windows, self.bin_bp)]


class Coverage(object):
    """What one measurement gives: the corrector, whether GC bins were used (a genome was given), per-window arrays
    (reference name -> (bp int64, present uint8)) when they were asked for, and the timings."""

    def __init__(self, corrector, by_gc, windows=None, stats=None):
        self.corrector, self.by_gc, self.windows, self.stats = corrector, by_gc, windows, stats or {}

    def divisor(self, repeat_segments):
        """(the average coverage to divide by for a locus, where it came from): the mean of the locus's GC bin, the sequencing
        mean when that bin is empty or no genome was given."""
        c = self.corrector
        if self.by_gc:
            gc = get_gc_content(''.join(repeat_segments))
            if c.has_gc_bin(gc):
                return c.get_mean_coverage_of_gc_content(gc), "gc_bin"
            return c.get_sequencing_mean_coverage(), "sequencing_mean_empty_bin"
        return c.get_sequencing_mean_coverage(), "sequencing_mean"

    def summary(self):
        c = self.corrector
        return {"divisor": "gc_bin" if self.by_gc else "sequencing_mean", "sequencing_mean": c.get_sequencing_mean_coverage(),
                "windows": c.windows(), "bins": [[w, m] for w, m in c.bins()]}


def layout(references, lengths, genome=None):
    """[(header index, chromosome, reference sequence codes or None)] of the references whose records count.  With a genome,
    a counted chromosome it lacks contributes nothing and one whose length differs from the header's is an error; two
    references that name one chromosome (e.g. '1' and 'chr1') are an error."""
    out, seen = [], {}
    for i, (name, length) in enumerate(zip(references, lengths)):
        chrom = counted_chromosome(name)
        if chrom is None:
            continue
        if chrom in seen:
            raise ValueError("references %r and %r both count as %s" % (seen[chrom], name, chrom))
        seen[chrom] = name
        codes = None
        if genome is not None:
            if chrom not in genome:
                continue
            codes = genome[chrom].codes
            if len(codes) != int(length):
                raise ValueError("%s: %d bases in the reference genome, %d in the alignment's header (%r)" %
                                 (chrom, len(codes), int(length), name))
        out.append((i, chrom, codes))
    return out


def windows_host(n_windows, rec_ref, rec_start, rec_end):
    """The accumulation on the host (the device's code): concatenated (bp, present) over references of n_windows[r] windows."""
    L = _lib.load()
    nw = np.ascontiguousarray(n_windows, dtype=np.int64)
    ref = np.ascontiguousarray(rec_ref, dtype=np.int32)
    s = np.ascontiguousarray(rec_start, dtype=np.int64)
    e = np.ascontiguousarray(rec_end, dtype=np.int64)
    total = int(nw.sum())
    bp, present = np.zeros(max(1, total), np.int64), np.zeros(max(1, total), np.uint8)
    _lib.check(L.advntr_coverage_windows_host(len(nw), _lib.ptr(nw), _lib.ptr(ref), _lib.ptr(s), _lib.ptr(e), len(ref), _lib.ptr(bp),
                                              _lib.ptr(present)))
    return bp[:total], present[:total]


def gc_host(codes):
    """GC counts of the full windows of a chromosome (uint8 FASTA bytes), on the host."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    gc = np.zeros(max(1, len(codes) // GC_CONTENT_WINDOW_SIZE), np.uint8)
    _lib.check(_lib.load().advntr_coverage_gc_host(_lib.ptr(codes), len(codes), _lib.ptr(gc)))
    return gc[:len(codes) // GC_CONTENT_WINDOW_SIZE]


def gc_device(codes):
    """The same on the device: (gc counts, [upload ms, kernel ms])."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    gc = np.zeros(max(1, len(codes) // GC_CONTENT_WINDOW_SIZE), np.uint8)
    ms = np.zeros(2, np.float64)
    _lib.check(_lib.load().advntr_coverage_gc(_lib.ptr(codes), len(codes), _lib.ptr(gc), _lib.ptr(ms)))
    return gc[:len(codes) // GC_CONTENT_WINDOW_SIZE], ms


def bins_host(bp, present, gc=None, bin_windows=None, bin_bp=None):
    """Adds the windows to (bin_windows, bin_bp) (new zero arrays when None) and returns them; gc None = all in bin 0."""
    bw = np.zeros(BINS, np.int64) if bin_windows is None else bin_windows
    bb = np.zeros(BINS, np.int64) if bin_bp is None else bin_bp
    bp = np.ascontiguousarray(bp, dtype=np.int64)
    present = np.ascontiguousarray(present, dtype=np.uint8)
    g = None if gc is None else np.ascontiguousarray(gc, dtype=np.uint8)
    _lib.check(_lib.load().advntr_coverage_bins_host(_lib.ptr(bp), _lib.ptr(present), _lib.ptr(g), len(bp), _lib.ptr(bw), _lib.ptr(bb)))
    return bw, bb


def record_interval(read):
    """[start, end) of a SamRead: `reference_end or reference_start + len(seq)` (a '*' sequence has length 0)."""
    start = read.reference_start
    seq_len = 0 if read.seq in (None, '*') else len(read.seq)
    return start, (read.reference_end if read.reference_end else start + seq_len)


def sam_reference_lengths(text):
    """{name: LN} of the @SQ lines of SAM text."""
    out = {}
    for line in text.split("\n"):
        if not line.startswith("@SQ"):
            if line and not line.startswith("@"):
                break
            continue
        f = dict(x.split(":", 1) for x in line.split("\t")[1:] if ":" in x)
        if "SN" in f and "LN" in f:
            out[f["SN"]] = int(f["LN"])
    return out


def measure_sam(samfile, lengths, genome=None, keep_windows=False):
    """The coverage of SAM text records (parse_sam's SamFile) on the host; lengths = sam_reference_lengths of the text."""
    references = list(samfile.references)
    missing = [r for r in references if r not in lengths]
    if missing:
        raise ValueError("@SQ line without LN for %s" % ", ".join(missing))
    lay = layout(references, [lengths[r] for r in references], genome)
    index = {references[i]: k for k, (i, _, _) in enumerate(lay)}
    n_windows = [lengths[references[i]] // GC_CONTENT_WINDOW_SIZE for i, _, _ in lay]
    rec_ref, rec_start, rec_end = [], [], []
    for r in samfile.reads:
        k = index.get(r.reference_name)
        if k is None:
            continue
        s, e = record_interval(r)
        rec_ref.append(k)
        rec_start.append(s)
        rec_end.append(e)
    bp, present = windows_host(n_windows, rec_ref, rec_start, rec_end)
    bw, bb = np.zeros(BINS, np.int64), np.zeros(BINS, np.int64)
    windows = {}
    at = 0
    for (i, chrom, codes), n in zip(lay, n_windows):
        b, p = bp[at:at + n], present[at:at + n]
        bins_host(b, p, gc_host(codes) if codes is not None else None, bw, bb)
        if keep_windows:
            windows[references[i]] = (b, p)
        at += n
    return Coverage(CoverageCorrector(bw, bb), genome is not None, windows if keep_windows else None)


def measure_bam_handle(L, h, references, lay, by_gc, keep_windows=False):
    """Bins (and optionally windows) of an advntr_bam_select handle made with ADVNTR_BAM_COVERAGE; lay = layout(...)."""
    bw, bb = np.zeros(BINS, np.int64), np.zeros(BINS, np.int64)
    for i, _, codes in lay:
        c = None if codes is None else np.ascontiguousarray(codes, dtype=np.uint8)
        _lib.check(L.advntr_bam_coverage_bins(h, i, _lib.ptr(c), 0 if c is None else len(c), _lib.ptr(bw), _lib.ptr(bb)))
    n_ref = ctypes.c_int32()
    n_windows = np.zeros(max(1, len(references)), np.int64)
    stats = np.zeros(_lib.BAM_COVERAGE_STATS, np.float64)
    _lib.check(L.advntr_bam_coverage_info(h, ctypes.byref(n_ref), _lib.ptr(n_windows), _lib.ptr(stats)))
    windows = None
    if keep_windows:
        windows = {}
        for i in range(n_ref.value):
            n = int(n_windows[i])
            bp, present = np.zeros(max(1, n), np.int64), np.zeros(max(1, n), np.uint8)
            _lib.check(L.advntr_bam_coverage_windows(h, i, _lib.ptr(bp), _lib.ptr(present)))
            windows[references[i]] = (bp[:n], present[:n])
    keys = ("accumulate_kernel_ms", "scan_kernel_ms", "chrom_upload_ms", "gc_kernel_ms", "bins_kernel_ms", "windows")
    return Coverage(CoverageCorrector(bw, bb), by_gc, windows, dict(zip(keys, (float(x) for x in stats))))
