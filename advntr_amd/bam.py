"""BAM input on the GPU: what pysam.AlignmentFile gives the Illumina path (vntr_finder.py:701-750) and what the reference's
whole-file `samtools view -b -f4` + bam2fq gives it (sam_utils.py:9-23), from one streaming pass over the file.

The BGZF blocks are inflated on the device, the records are found and selected there, and only the kept records -- the
file's first five, every mapped record that overlaps a window the file is opened with, and every unmapped record -- are
decoded and become `sam_utils.SamRead` objects.  `open_alignment(path, windows)` returns an object with the `SamFile`
surface the callers use: `references`, `reads`, `head(n)` and `fetch(reference, start, end)`; fetch raises for a region the
file was not opened with instead of answering from records it never kept.  Duplicate, length, N and quality filtering stay
in vntr_finder.select_illumina_reads_multi and sam_utils.is_low_quality_read.
"""
import ctypes

import numpy as np

from . import _lib
from .sam_utils import SamRead

_GZIP_MAGIC = b"\x1f\x8b\x08"


def sniff(path):
    """'bgzf', 'gzip' (a gzip file that is not BGZF), 'cram' or 'text'."""
    with open(path, "rb") as fh:
        head = fh.read(18)
    if head[:4] == b"CRAM":
        return "cram"
    if head[:3] != _GZIP_MAGIC:
        return "text"
    if len(head) >= 18 and head[3] & 4:
        xlen = int.from_bytes(head[10:12], "little")
        with open(path, "rb") as fh:
            extra = fh.read(12 + xlen)[12:]
        at = 0
        while at + 4 <= len(extra):
            slen = int.from_bytes(extra[at + 2:at + 4], "little")
            if extra[at:at + 2] == b"BC" and slen == 2:
                return "bgzf"
            at += 4 + slen
    return "gzip"


def scan_framing(data):
    """(block offsets, block sizes, ISIZEs) of a BGZF file held in memory (host only)."""
    L = _lib.load()
    buf = np.frombuffer(data, dtype=np.uint8)
    n = ctypes.c_int64()
    _lib.check(L.advntr_bgzf_scan(_lib.ptr(buf), len(buf), None, None, None, 0, ctypes.byref(n)))
    off, size, isize = np.zeros(n.value, np.int64), np.zeros(n.value, np.int32), np.zeros(n.value, np.uint32)
    _lib.check(L.advntr_bgzf_scan(_lib.ptr(buf), len(buf), _lib.ptr(off), _lib.ptr(size), _lib.ptr(isize), n.value, ctypes.byref(n)))
    return off, size, isize


def read_header(path):
    """(reference names, reference lengths, uncompressed header bytes) from the binary header (host only); the @SQ text is
    not consulted, as pysam's `references` does not."""
    L = _lib.load()
    n_ref, nb, hb = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64()
    p = path.encode()
    _lib.check(L.advntr_bam_header(p, None, 0, None, 0, ctypes.byref(n_ref), ctypes.byref(nb), ctypes.byref(hb)))
    names = ctypes.create_string_buffer(max(1, nb.value))
    lengths = np.zeros(max(1, n_ref.value), np.int32)
    _lib.check(L.advntr_bam_header(p, names, nb.value, _lib.ptr(lengths), n_ref.value, ctypes.byref(n_ref), ctypes.byref(nb),
                                   ctypes.byref(hb)))
    refs = [s.decode() for s in names.raw[:nb.value].split(b"\0")[:-1]] if nb.value else []
    return refs, [int(x) for x in lengths[:n_ref.value]], hb.value


def inflate(data):
    """Every block of a BGZF file held in memory, inflated on the device (ISIZE and CRC32 checked)."""
    L = _lib.load()
    buf = np.frombuffer(data, dtype=np.uint8)
    _, _, isize = scan_framing(data)
    out = np.zeros(max(1, int(isize.sum(dtype=np.int64))), np.uint8)
    n = ctypes.c_int64()
    _lib.check(L.advntr_bgzf_inflate(_lib.ptr(buf), len(buf), _lib.ptr(out), len(out), ctypes.byref(n)))
    return out[:n.value].tobytes()


def walk_host(raw, start):
    """(record offsets, end) of the sequential walk over uncompressed bytes from `start` (host only)."""
    L = _lib.load()
    buf = np.frombuffer(raw, dtype=np.uint8)
    n, end = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(L.advntr_bam_walk_host(_lib.ptr(buf), len(buf), start, None, 0, ctypes.byref(n), ctypes.byref(end)))
    offs = np.zeros(max(1, n.value), np.int64)
    _lib.check(L.advntr_bam_walk_host(_lib.ptr(buf), len(buf), start, _lib.ptr(offs), n.value, ctypes.byref(n), ctypes.byref(end)))
    return offs[:n.value], end.value


def _reads(references, fields, text, text_off):
    fields = fields.reshape(-1, _lib.BAM_FIELDS)
    tb = bytes(text)
    out = []
    for k in range(len(fields)):
        ref, pos, flag, mapq, end, ln, ls, lq, lc, _ = (int(x) for x in fields[k])
        a = int(text_off[k])
        r = SamRead()
        r.query_name = tb[a:a + ln].decode()
        a += ln
        r.seq = tb[a:a + ls].decode()
        a += ls
        r.query_qualities = list(tb[a:a + lq]) if lq else None
        a += lq
        r.cigar = tb[a:a + lc].decode()
        r.flag, r.mapq, r.reference_start = flag, mapq, pos
        r.reference_name = references[ref] if 0 <= ref < len(references) else "*"
        r.reference_end = None if end < 0 else end
        out.append(r)
    return out


def decode_host(raw, offsets, references):
    """SamRead objects of the records of uncompressed bytes `raw` at `offsets`, decoded on the host by the device's code."""
    L = _lib.load()
    buf = np.frombuffer(raw, dtype=np.uint8)
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(offs)
    toff = np.zeros(n + 1, np.int64)
    _lib.check(L.advntr_bam_decode_host(_lib.ptr(buf), len(buf), _lib.ptr(offs), n, None, None, 0, _lib.ptr(toff)))
    fields = np.zeros(max(1, n) * _lib.BAM_FIELDS, np.int32)
    text = np.zeros(max(1, int(toff[n])), np.uint8)
    _lib.check(L.advntr_bam_decode_host(_lib.ptr(buf), len(buf), _lib.ptr(offs), n, _lib.ptr(fields), _lib.ptr(text),
                                        len(text), _lib.ptr(toff)))
    return _reads(references, fields[:n * _lib.BAM_FIELDS], text, toff)


def vntr_windows(references, vntrs):
    """The fetch windows of select_illumina_reads_multi for these loci, with its chromosome naming (the vntr's own name
    when get_reference_genome_of_alignment_file says HG19, the name without 'chr' otherwise)."""
    from .sam_utils import get_reference_genome_of_alignment_file
    reference = get_reference_genome_of_alignment_file(_Refs(references))
    out = []
    for v in vntrs:
        chromosome = v.chromosome if reference == 'HG19' else v.chromosome[3:]
        out.append((chromosome, v.start_point, v.start_point + v.get_length()))
    return out


class _Refs(object):
    def __init__(self, references):
        self.references = references


class BamFile(object):
    """The kept records of one pass (file order) and the windows they were selected for."""

    def __init__(self, references, reads, windows, stats, offsets=None):
        self.references, self.reads, self.stats, self.offsets = references, reads, stats, offsets
        self.coverage = None                # coverage.Coverage of a pass opened with coverage=True
        self._windows = {}
        for ref, s, e in windows:
            self._windows.setdefault(ref, []).append((int(s), int(e)))
        self._mapped = {}
        for r in reads:
            if not r.is_unmapped:
                self._mapped.setdefault(r.reference_name, []).append(r)

    def head(self, n):
        return self.reads[:n]

    def fetch(self, reference, start, end):
        """Mapped reads of `reference` overlapping [start, end), in file order, as SamFile.fetch.  The region must lie in one
        window the file was opened with: the records outside the windows were never kept."""
        if not any(s <= start and end <= e for s, e in self._windows.get(reference, ())):
            raise ValueError("fetch(%r, %d, %d): not within a window this BAM file was opened with" % (reference, start, end))
        for r in self._mapped.get(reference, ()):
            r_end = r.reference_end if r.reference_end is not None else r.reference_start + 1
            if r.reference_start < end and r_end > start:
                yield r


def open_alignment(path, windows, chunk_bytes=0, record_offsets=False, coverage=False, genome=None, coverage_windows=False):
    """One pass over the BAM file at `path` on the device.  windows: (reference name, start, end) half-open, named as the
    file's references are (vntr_windows).  chunk_bytes: compressed bytes per streamed chunk (0 = 256 MiB).  With
    record_offsets the uncompressed offset of every record is kept as well (tests).  With coverage the same pass sums the
    covered bases per 100-bp window over every record (advntr_amd/coverage.py); the result's `coverage` is a
    coverage.Coverage whose bins use the GC content of `genome` (genome.Genome) when one is given, and which holds the
    per-window arrays of every reference when coverage_windows is set."""
    L = _lib.load()
    references, lengths, _ = read_header(path)
    lay = None
    if coverage:
        from . import coverage as coverage_mod
        lay = coverage_mod.layout(references, lengths, genome)      # the errors of the layout before the pass
    index = {name: i for i, name in enumerate(references)}
    per_ref = [[] for _ in references]
    for ref, s, e in windows:
        if ref in index:
            per_ref[index[ref]].append((int(s), int(e)))
    win_ptr = np.zeros(len(references) + 1, np.int32)
    np.cumsum([len(w) for w in per_ref], out=win_ptr[1:])
    flat = [w for ws in per_ref for w in ws]
    ws = np.array([w[0] for w in flat] or [0], np.int64)
    we = np.array([w[1] for w in flat] or [0], np.int64)
    flags = (_lib.BAM_RECORD_OFFSETS if record_offsets else 0) | (_lib.BAM_COVERAGE if coverage else 0)
    h = L.advntr_bam_select(path.encode(), len(references), _lib.ptr(win_ptr), _lib.ptr(ws), _lib.ptr(we), int(chunk_bytes), flags)
    if not h:
        err = _lib.last_error()
        raise _lib.EngineError(_lib.ERR_DEVICE if "no HIP device" in err else _lib.ERR_DATA, err)
    measured = None
    try:
        n_kept, text_bytes, n_offs = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        stats = np.zeros(_lib.BAM_STATS, np.float64)
        _lib.check(L.advntr_bam_kept_info(h, ctypes.byref(n_kept), ctypes.byref(text_bytes), ctypes.byref(n_offs), _lib.ptr(stats)))
        fields = np.zeros(max(1, n_kept.value) * _lib.BAM_FIELDS, np.int32)
        text = np.zeros(max(1, text_bytes.value), np.uint8)
        toff = np.zeros(n_kept.value + 1, np.int64)
        _lib.check(L.advntr_bam_kept_fetch(h, _lib.ptr(fields), _lib.ptr(text), _lib.ptr(toff)))
        offsets = None
        if record_offsets:
            offsets = np.zeros(max(1, n_offs.value), np.int64)
            _lib.check(L.advntr_bam_kept_offsets(h, _lib.ptr(offsets)))
            offsets = offsets[:n_offs.value]
        if coverage:
            measured = coverage_mod.measure_bam_handle(L, h, references, lay, genome is not None, coverage_windows)
    finally:
        L.advntr_bam_kept_destroy(h)
    reads = _reads(references, fields[:n_kept.value * _lib.BAM_FIELDS], text, toff)
    keys = ("blocks", "compressed_bytes", "uncompressed_bytes", "records", "kept", "chunks", "read_ms", "framing_ms",
            "upload_ms", "inflate_kernel_ms", "boundary_ms", "fallback_blocks", "fallback_ms", "select_ms", "total_ms")
    out = BamFile(references, reads, windows, dict(zip(keys, (float(x) for x in stats))), offsets)
    out.coverage = measured
    return out


# ------------------------------------------------------------------------------------------------
# Long reads (vntr_finder.py:373-471, 640-651): the mapped records that span each window, trimmed to its flanks on the device
# ------------------------------------------------------------------------------------------------
SPAN_OK, SPAN_UNMAPPED, SPAN_NO_ALIGNED, SPAN_NOT_SPANNING, SPAN_SHORT_FLANK, SPAN_NO_SEQ = range(6)
SPAN_FLANK, SPAN_MIN_FLANK = 100, 10        # hmm_flanking_region_size, min_flanking_bp (vntr_finder.py:374-375)
_SPAN_STATS = ("pairs", "spanning", "rejected_unmapped", "rejected_no_aligned", "rejected_not_spanning", "rejected_short_flank",
               "rejected_no_seq", "span_kernel_ms", "trimmed_bytes", "unmapped_bytes", "whole_bytes", "trim_kernel_ms")
_BAM_STATS = ("blocks", "compressed_bytes", "uncompressed_bytes", "records", "kept", "chunks", "read_ms", "framing_ms",
              "upload_ms", "inflate_kernel_ms", "boundary_ms", "fallback_blocks", "fallback_ms", "select_ms", "total_ms")


def _pieces(pairs, text, text_off):
    """per pair (window, locus, record, status, rs, end, left, tr, right, name length) -> (name, piece) of the spanning ones"""
    tb = bytes(text)
    out = []
    for k in range(len(pairs)):
        if pairs[k, 3] != SPAN_OK:
            out.append(None)
            continue
        a, nl = int(text_off[k]), int(pairs[k, 9])
        out.append((tb[a:a + nl].decode(), tb[a + nl:int(text_off[k + 1])].decode()))
    return out


def span_host(raw, offsets, windows, flank=SPAN_FLANK, min_flank=SPAN_MIN_FLANK):
    """The long-read rule on the host (the device's code): pair k = the record of uncompressed bytes `raw` at offsets[k] and the
    window windows[k] = (vs, ve).  Returns (pairs [n, BAM_SPAN_FIELDS] int64, [(name, piece) or None per pair])."""
    L = _lib.load()
    buf = np.frombuffer(raw, dtype=np.uint8)
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(offs)
    ws = np.array([int(w[0]) for w in windows] or [0], np.int64)
    we = np.array([int(w[1]) for w in windows] or [0], np.int64)
    toff = np.zeros(n + 1, np.int64)
    pairs = np.zeros((max(1, n), _lib.BAM_SPAN_FIELDS), np.int64)
    _lib.check(L.advntr_bam_span_host(_lib.ptr(buf), len(buf), _lib.ptr(offs), _lib.ptr(ws), _lib.ptr(we), n, flank, min_flank,
                                      None, None, 0, _lib.ptr(toff)))
    text = np.zeros(max(1, int(toff[n])), np.uint8)
    _lib.check(L.advntr_bam_span_host(_lib.ptr(buf), len(buf), _lib.ptr(offs), _lib.ptr(ws), _lib.ptr(we), n, flank, min_flank,
                                      _lib.ptr(pairs), _lib.ptr(text), len(text), _lib.ptr(toff)))
    return pairs[:n], _pieces(pairs[:n], text, toff)


class BamSpans(object):
    """One long-read pass: `pairs` (every (window, mapped record) pair, by window then file order, BAM_SPAN_FIELDS int64 each),
    `pieces[k]` = (query name, trimmed sequence) of pair k when it spans, else None; `unmapped` = the unmapped records as
    SamRead objects (file order); `stats`."""

    def __init__(self, references, pairs, pieces, unmapped, stats):
        self.references, self.pairs, self.pieces, self.unmapped, self.stats = references, pairs, pieces, unmapped, stats

    def spanning(self, n_windows):
        """per window (input order): [(query_name, trimmed sequence, left_bp, tr_bp, right_bp)] of its spanning records"""
        out = [[] for _ in range(n_windows)]
        for k, piece in enumerate(self.pieces):
            if piece is not None:
                p = self.pairs[k]
                out[int(p[0])].append((piece[0], piece[1], int(p[6]), int(p[7]), int(p[8])))
        return out


def open_alignment_spans(path, windows, chunk_bytes=0, flank=SPAN_FLANK, min_flank=SPAN_MIN_FLANK):
    """One pass over the aligned long-read BAM at `path` on the device.  windows: (reference name, vs, ve[, locus id]) as
    vntr_windows gives them; windows on references the file does not have get no pairs.  Returns a BamSpans; its
    spanning(len(windows)) lists the trimmed mapped reads of every window."""
    L = _lib.load()
    references, _, _ = read_header(path)
    index = {name: i for i, name in enumerate(references)}
    per_ref = [[] for _ in references]
    for k, w in enumerate(windows):
        if w[0] in index:
            per_ref[index[w[0]]].append((int(w[1]), int(w[2]), k, int(w[3]) if len(w) > 3 else k))
    win_ptr = np.zeros(len(references) + 1, np.int32)
    np.cumsum([len(w) for w in per_ref], out=win_ptr[1:])
    flat = [w for ws in per_ref for w in ws]
    ws = np.array([w[0] for w in flat] or [0], np.int64)
    we = np.array([w[1] for w in flat] or [0], np.int64)
    locus = np.array([w[3] for w in flat] or [0], np.int64)
    h = L.advntr_bam_select_spans(path.encode(), len(references), _lib.ptr(win_ptr), _lib.ptr(ws), _lib.ptr(we), _lib.ptr(locus),
                                  int(flank), int(min_flank), int(chunk_bytes), 0)
    if not h:
        err = _lib.last_error()
        raise _lib.EngineError(_lib.ERR_DEVICE if "no HIP device" in err else _lib.ERR_DATA, err)
    try:
        n_pairs, text_bytes, n_unmapped, ubytes = (ctypes.c_int64() for _ in range(4))
        stats = np.zeros(_lib.BAM_SPAN_STATS, np.float64)
        _lib.check(L.advntr_bam_spans_info(h, ctypes.byref(n_pairs), ctypes.byref(text_bytes), ctypes.byref(n_unmapped),
                                           ctypes.byref(ubytes), _lib.ptr(stats)))
        pairs = np.zeros((max(1, n_pairs.value), _lib.BAM_SPAN_FIELDS), np.int64)
        text = np.zeros(max(1, text_bytes.value), np.uint8)
        toff = np.zeros(n_pairs.value + 1, np.int64)
        fields = np.zeros(max(1, n_unmapped.value) * _lib.BAM_FIELDS, np.int32)
        utext = np.zeros(max(1, ubytes.value), np.uint8)
        utoff = np.zeros(n_unmapped.value + 1, np.int64)
        _lib.check(L.advntr_bam_spans_fetch(h, _lib.ptr(pairs), _lib.ptr(text), _lib.ptr(toff), _lib.ptr(fields), _lib.ptr(utext),
                                            _lib.ptr(utoff)))
    finally:
        L.advntr_bam_spans_destroy(h)
    pairs = pairs[:n_pairs.value]
    # the device reports windows by their index in its (per-reference) list: back to the caller's index
    if len(pairs):
        pairs[:, 0] = np.array([w[2] for w in flat], np.int64)[pairs[:, 0]]
        order = np.argsort(pairs[:, 0], kind="stable")
    else:
        order = np.zeros(0, np.int64)
    pieces = _pieces(pairs, text, toff)
    pairs, pieces = pairs[order], [pieces[i] for i in order.tolist()]
    unmapped = _reads(references, fields[:n_unmapped.value * _lib.BAM_FIELDS], utext, utoff)
    st = dict(zip(_BAM_STATS, (float(x) for x in stats[:15])))
    st.update(zip(_SPAN_STATS, (float(x) for x in stats[16:])))
    return BamSpans(references, pairs, pieces, unmapped, st)
