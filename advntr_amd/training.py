"""Recruitment-score training of many new loci at once (the `addmodel` command, advntr_commands.py:179-215).

Per locus this computes what vntr_extras.train_classifier_threshold computes (VNTRFinder.train_classifier_threshold,
vntr_finder.py:902-1021), exactly:
  * true reads: random.seed(0), then simulate_true_reads (Python, the reference's random stream);
  * false reads: one pass over each chromosome for all of its loci -- the GPU scan of csrc/genome_scan.h finds the keyword
    hits, the host folds them into reads (spans of the chromosome, no Python string per read);
then, for all loci together: one native build of the read-matcher models, one engine batch scoring every true and false read
on the forward strand, the recruit rule of find_hmm_score_of_simulated_reads, and find_recruitment_score_threshold per locus
on host threads.
"""
import random
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib

KEYWORD_SIZE = 11
READ_LENGTH = 150
_BASE4 = np.full(256, 255, np.uint8)
for _i, _c in enumerate("ACGT"):
    _BASE4[ord(_c)] = _i
    _BASE4[ord(_c.lower())] = _i

SCAN_READS = 10030             # ADVNTR_GENOME_SCAN_READS: reads one locus can hold
# positions per chunk of the device scan; 0 = the library's own.  Tests set a small value so that hits straddle chunks.
_SCAN_CHUNK = 0


def keyword_values(vntr):
    """The locus's filtering keywords (get_keywords_for_filtering(..., True, 11)) made of A/C/G/T only, as 2-bit 11-mers."""
    from .filtering import get_keywords_for_filtering
    keywords = get_keywords_for_filtering(vntr.left_flanking_region, vntr.get_repeat_segments(), vntr.right_flanking_region,
                                          vntr.pattern, True, KEYWORD_SIZE)
    words = sorted(k for k in keywords if len(k) == KEYWORD_SIZE)
    if not words:
        return np.zeros(0, np.uint32)
    codes = _BASE4[np.frombuffer("".join(words).encode("latin-1", "replace"), np.uint8)].reshape(-1, KEYWORD_SIZE)
    codes = codes[(codes < 4).all(axis=1)].astype(np.uint32)
    value = np.zeros(len(codes), np.uint32)
    for t in range(KEYWORD_SIZE):
        value = value * 4 + codes[:, t]
    return value


def _codes_of(chromosome):
    codes = chromosome.codes if hasattr(chromosome, "codes") else chromosome
    if isinstance(codes, str):
        codes = codes.encode("latin-1", "replace")
    if isinstance(codes, (bytes, bytearray)):
        codes = np.frombuffer(bytes(codes), np.uint8)
    return np.ascontiguousarray(codes, np.uint8)


def scan_false_reads(chromosome, vntrs, device=True, chunk=None):
    """simulate_false_filtered_reads for every locus in `vntrs` (all on `chromosome`: a genome.Chromosome, bytes, str or
    uint8 array) -> ([(begin int64[k], end int64[k]) per locus], stats dict).  The reads are chromosome[begin:end]; device=False
    runs the rule on the host (advntr_genome_scan_host)."""
    s = _codes_of(chromosome)
    n_loci = len(vntrs)
    kws = [keyword_values(v) for v in vntrs]
    kw_off = np.zeros(n_loci + 1, np.int32)
    np.cumsum([len(k) for k in kws], out=kw_off[1:])
    kw = np.ascontiguousarray(np.concatenate(kws) if n_loci else np.zeros(0, np.uint32), np.uint32)
    vs = np.array([v.start_point for v in vntrs], np.int64)
    ve = np.array([v.start_point + v.get_length() for v in vntrs], np.int64)
    cap = SCAN_READS
    rb = np.zeros((max(n_loci, 1), cap), np.int64)
    re_ = np.zeros((max(n_loci, 1), cap), np.int64)
    count = np.zeros(max(n_loci, 1), np.int32)
    stats = np.zeros(7, np.float64)
    p = _lib.ptr
    L = _lib.load()
    if device:
        _lib.require_gpu()
        _lib.check(L.advntr_genome_scan(p(s), len(s), n_loci, p(vs), p(ve), p(kw_off), p(kw),
                                        int(_SCAN_CHUNK if chunk is None else chunk), p(rb), p(re_), p(count), p(stats)))
    else:
        t0 = time.perf_counter()
        _lib.check(L.advntr_genome_scan_host(p(s), len(s), n_loci, p(vs), p(ve), p(kw_off), p(kw), p(rb), p(re_), p(count)))
        stats[6] = (time.perf_counter() - t0) * 1e3
    spans = [(rb[k, :count[k]].copy(), re_[k, :count[k]].copy()) for k in range(n_loci)]
    names = ("upload_ms", "kernel_ms", "fold_ms", "hits", "chunks", "bytes", "total_ms")
    return spans, dict(zip(names, stats.tolist()))


def false_read_texts(chromosome, spans):
    """The false reads of one locus as str (for tests and small inputs)."""
    s = _codes_of(chromosome)
    return [s[a:b].tobytes().decode("latin-1") for a, b in zip(spans[0].tolist(), spans[1].tolist())]


def _threads():
    return max(1, min(16, int(_lib.load().advntr_host_threads())))


def train_loci(vntrs, genome, read_length=READ_LENGTH, device=True, timings=None, scores=None):
    """Scaled recruitment scores (threshold / read_length) of loci whose repeat segments and flanks are set
    (models.init_from_vntrseek_data), each equal to vntr_extras.train_classifier_threshold(vntr, genome).  genome: a mapping
    chromosome name -> sequence (genome.Genome or dict).  timings (a dict) receives the stage times in seconds; scores (a list)
    receives each locus's (true scores, false scores) of the recruited reads."""
    from . import hmm_utils
    from .pomegranate import device_models
    from .vntr_extras import find_recruitment_score_threshold, simulate_true_reads
    from .vntr_finder import get_copies_for_hmm, recruit_mask
    tm = timings if timings is not None else {}
    n = len(vntrs)
    if n == 0:
        return []
    t = time.perf_counter()
    true_reads = []
    for v in vntrs:
        random.seed(0)          # what baking the locus's model does in the reference (hmm.pyx:858-859)
        true_reads.append(simulate_true_reads(v, read_length))
    tm["true_reads"] = time.perf_counter() - t

    t = time.perf_counter()
    by_chrom = {}
    for k, v in enumerate(vntrs):
        by_chrom.setdefault(v.chromosome, []).append(k)
    false_spans = [None] * n
    scan = dict(upload_ms=0.0, kernel_ms=0.0, fold_ms=0.0, hits=0.0, chunks=0.0, bytes=0.0, total_ms=0.0)
    for name, idx in by_chrom.items():
        spans, st = scan_false_reads(genome[name], [vntrs[k] for k in idx], device=device)
        for k, sp in zip(idx, spans):
            false_spans[k] = sp
        for key in scan:
            scan[key] += st[key]
    tm["false_reads"] = time.perf_counter() - t
    tm["scan"] = scan

    t = time.perf_counter()
    specs = [(v.left_flanking_region[-read_length:], v.right_flanking_region[:read_length], v.get_repeat_segments(),
              get_copies_for_hmm(read_length, len(v.pattern))) for v in vntrs]
    models = hmm_utils.build_read_matcher_models(specs)
    handles = device_models(models)
    tm["model_build"] = time.perf_counter() - t

    # the batch: per locus its true reads without 'N' (counted before upper-casing, as the mirror does), then its false reads
    t = time.perf_counter()
    parts, lens, owner, is_true = [], [], [], []
    for k, v in enumerate(vntrs):
        kept = [r.upper() for r in true_reads[k] if r.count('N') <= 0]
        codes, off = _lib.encode_reads(kept)
        parts.append(codes)
        lens.append(np.diff(off))
        owner.append(np.full(len(kept), k, np.int32))
        is_true.append(np.ones(len(kept), bool))
        begin, end = false_spans[k]
        if len(begin):
            s = _codes_of(genome[v.chromosome])
            codes, off, bad = _lib.encode_spans(s.ctypes.data, begin, end, case_sensitive=False)
            if bad.any():
                r = int(np.flatnonzero(bad)[0])
                raise ValueError("locus %s (%s:%d): the false read at %s:%d holds a symbol that is not A, C, G or T"
                                 % (v.id, v.chromosome, v.start_point, v.chromosome, int(begin[r])))
            parts.append(codes)
            lens.append(np.diff(off))
            owner.append(np.full(len(begin), k, np.int32))
            is_true.append(np.zeros(len(begin), bool))
    bases = np.ascontiguousarray(np.concatenate(parts), np.uint8)
    lens = np.concatenate(lens).astype(np.int64)
    read_off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=read_off[1:])
    owner = np.concatenate(owner)
    is_true = np.concatenate(is_true)
    tm["encode"] = time.perf_counter() - t

    t = time.perf_counter()
    logp, summ, _ = _lib.viterbi_batch(handles, bases, read_off, owner, want_paths=False, want_summary=True)
    ok = recruit_mask(logp, summ, lens, np.full(len(lens), -10000.0)) & (summ[:, _lib.SUM_REPEAT_BP] > 2)
    tm["scoring"] = time.perf_counter() - t
    tm["reads_scored"] = int(len(lens))

    t = time.perf_counter()
    order = np.argsort(owner, kind="stable")
    bounds = np.searchsorted(owner[order], np.arange(n + 1))

    def fit(k):
        sel = order[bounds[k]:bounds[k + 1]]
        sel = sel[ok[sel]]
        scores = logp[sel]
        true_scores = [float(x) for x in scores[is_true[sel]]]
        false_scores = [float(x) for x in scores[~is_true[sel]]]
        return true_scores, false_scores, find_recruitment_score_threshold(true_scores, false_scores) / float(read_length)
    with ThreadPoolExecutor(max_workers=min(_threads(), n)) as pool:
        fitted = list(pool.map(fit, range(n)))
    if scores is not None:
        scores.extend((f[0], f[1]) for f in fitted)
    scaled = [f[2] for f in fitted]
    tm["classifier"] = time.perf_counter() - t
    return scaled


def parse_regions(path):
    """`chrom start end pattern` rows (whitespace-separated, 0-based start; blank lines and '#' lines skipped)."""
    rows = []
    with open(path) as fh:
        for number, line in enumerate(fh, 1):
            text = line.strip()
            if not text or text.startswith("#"):
                continue
            cells = text.split()
            if len(cells) != 4:
                raise ValueError("%s line %d: expected `chrom start end pattern`, got %r" % (path, number, text))
            try:
                start, end = int(cells[1]), int(cells[2])
            except ValueError:
                raise ValueError("%s line %d: start and end must be integers: %r" % (path, number, text))
            rows.append((cells[0], start, end, cells[3], "%s line %d" % (path, number)))
    return rows


def check_rows(rows, genome):
    """Refuse bad rows before anything is written: a chromosome the FASTA lacks, a pattern that is not A/C/G/T, start >= end."""
    for chrom, start, end, pattern, where in rows:
        if chrom not in genome:
            raise ValueError("%s: chromosome %r is not in the reference" % (where, chrom))
        if not pattern or set(pattern) - set("ACGT"):
            raise ValueError("%s: pattern %r should only contain A, C, G, T" % (where, pattern))
        if start < 0 or start >= end:
            raise ValueError("%s: start %d must be >= 0 and below end %d" % (where, start, end))


def add_models(genome, rows, db_file, timings=None, device=True):
    """addmodel for every row (chrom, start, end, pattern, where) in order: ids from the database's largest + 1, each
    locus set up as add_model does (advntr_commands.py:179-215), all trained together and written in one transaction.
    Returns the new ReferenceVNTR objects."""
    import os
    from . import models, settings
    tm = timings if timings is not None else {}
    check_rows(rows, genome)
    settings.MAX_ERROR_RATE = 0.05                                      # the reference's default for addmodel
    if not os.path.exists(db_file):
        models.create_vntrs_database(db_file)
    first = models.get_largest_id_in_database(db_file) + 1
    t = time.perf_counter()
    vntrs = []
    for k, (chrom, start, end, pattern, _) in enumerate(rows):
        estimated_repeats = int((end - start) / len(pattern) + 5)
        v = models.ReferenceVNTR(first + k, pattern, start, chrom, None, None, estimated_repeats)
        models.init_from_vntrseek_data(v, genome[chrom])
        vntrs.append(v)
    tm["init_loci"] = time.perf_counter() - t
    if not settings.ALIGN_REPEATS:
        for v, row in zip(vntrs, rows):
            if len(set(map(len, v.get_repeat_segments()))) > 1:
                raise NotImplementedError("%s: the repeat units found have different lengths %s; they need a multiple "
                                          "alignment first (--align-repeats)" % (row[4], sorted(set(map(len, v.get_repeat_segments())))))
    scores = train_loci(vntrs, genome, timings=tm, device=device)
    for v, s in zip(vntrs, scores):
        v.scaled_score = s
    t = time.perf_counter()
    models.save_reference_vntrs_to_database(vntrs, db_file)
    tm["db_write"] = time.perf_counter() - t
    return vntrs
