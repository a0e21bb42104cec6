"""A test-side BGZF / BAM writer, written from the SAMv1 specification (section 4: BGZF framing, the BAM header and record
layout) with struct and zlib alone.  It does not import the product.

Records are given as SAM fields (QNAME, FLAG, RNAME, POS 1-based, MAPQ, CIGAR, SEQ, QUAL as text; the mate fields are
written as unset).  Two framings:
  "htslib": a block is flushed before a record that would not fit in it (a record longer than a block still spans blocks);
  "htsjdk": blocks are filled to 65 280 uncompressed bytes, records split wherever the boundary falls.
Each block can take its own zlib level and strategy (raw deflate, wbits -15).  The spec's 28-byte EOF block ends the file.
"""
import re
import struct
import zlib

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BLOCK_DATA = 65280          # what htslib / htsjdk put in one block at most
_OPS = "MIDNSHP=X"
_BASES = "=ACMGRSVTWYHKDBN"
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE,
              "filtered": zlib.Z_FILTERED}


def bgzf_block(data, level=6, strategy="default"):
    """One BGZF block holding `data` (at most 65 536 bytes)."""
    assert len(data) <= 65536
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, STRATEGIES[strategy])
    cdata = c.compress(data) + c.flush()
    bsize = 18 + len(cdata) + 8
    if bsize > 65536:
        raise ValueError("block does not fit BSIZE: %d compressed bytes" % len(cdata))
    head = struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, bsize - 1)
    return head + cdata + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data))


def bgzf_blocks(pieces, modes=((6, "default"),)):
    """BGZF bytes of the given uncompressed pieces, one block each (block i uses modes[i % len(modes)]), plus the EOF block."""
    out = []
    for i, p in enumerate(pieces):
        level, strategy = modes[i % len(modes)]
        out.append(bgzf_block(p, level, strategy))
    return b"".join(out) + EOF_BLOCK


def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def bam_header(references, text=""):
    """references: [(name, length)]"""
    t = text.encode()
    out = [b"BAM\1", struct.pack("<i", len(t)), t, struct.pack("<i", len(references))]
    for name, length in references:
        n = name.encode() + b"\0"
        out += [struct.pack("<i", len(n)), n, struct.pack("<i", length)]
    return b"".join(out)


def bam_record(fields, ref_ids):
    """One record from SAM fields (qname, flag, rname, pos, mapq, cigar, seq, qual); ref_ids: name -> refID."""
    qname, flag, rname, pos, mapq, cigar, seq, qual = fields
    ref = -1 if rname == "*" else ref_ids[rname]
    ops = [] if cigar == "*" else [(int(n), _OPS.index(op)) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    s = "" if seq == "*" else seq
    span = sum(n for n, op in ops if _OPS[op] in "MDN=X")
    p0 = int(pos) - 1
    end = p0 + (span if span else 1)
    name = qname.encode() + b"\0"
    packed = bytearray((len(s) + 1) // 2)
    for i, ch in enumerate(s):
        packed[i // 2] |= _BASES.index(ch.upper()) << (4 if i % 2 == 0 else 0)     # (htslib: lower case as upper)
    q = bytes([0xff] * len(s)) if qual == "*" else bytes(ord(c) - 33 for c in qual)
    body = struct.pack("<iiBBHHHiiii", ref, p0, len(name), int(mapq), reg2bin(max(p0, 0), max(end, 1)) if ref >= 0 else 4680,
                       len(ops), int(flag), len(s), -1, -1, 0)
    body += name + b"".join(struct.pack("<I", n << 4 | op) for n, op in ops) + bytes(packed) + q
    return struct.pack("<i", len(body)) + body


def sam_text(references, records):
    """The same records as SAM text (what sam_utils.parse_sam reads)."""
    lines = ["@HD\tVN:1.6\tSO:coordinate"] + ["@SQ\tSN:%s\tLN:%d" % r for r in references]
    for qname, flag, rname, pos, mapq, cigar, seq, qual in records:
        lines.append("\t".join([qname, str(flag), rname, str(pos), str(mapq), cigar, "*", "0", "0", seq, qual]))
    return "\n".join(lines) + "\n"


def write_bam(references, records, framing="htslib", modes=((6, "default"),), text=None, block_data=BLOCK_DATA):
    """BAM bytes: header, records (SAM fields) in the given order, in the given framing; the EOF block last."""
    ref_ids = {name: i for i, (name, _) in enumerate(references)}
    header = bam_header(references, sam_text(references, []) if text is None else text)
    recs = [bam_record(r, ref_ids) for r in records]
    pieces = []
    if framing == "htsjdk":
        data = header + b"".join(recs)
        pieces = [data[i:i + block_data] for i in range(0, len(data), block_data)]
    elif framing == "htslib":
        cur = bytearray(header)
        while len(cur) > block_data:             # (a header longer than a block)
            pieces.append(bytes(cur[:block_data]))
            del cur[:block_data]
        if cur:                                   # htslib flushes the header in blocks of its own
            pieces.append(bytes(cur))
            cur = bytearray()
        for r in recs:
            if cur and len(cur) + len(r) > block_data:
                pieces.append(bytes(cur))
                cur = bytearray()
            cur += r
            while len(cur) > block_data:          # a record longer than a block
                pieces.append(bytes(cur[:block_data]))
                del cur[:block_data]
        if cur:
            pieces.append(bytes(cur))
    else:
        raise ValueError(framing)
    return bgzf_blocks(pieces, modes)


def inflate_all(data):
    """zlib's inflate of every block of a BGZF file (the yardstick)."""
    out, at = [], 0
    while at < len(data):
        xlen = struct.unpack_from("<H", data, at + 10)[0]
        bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
        out.append(zlib.decompress(data[at + 12 + xlen:at + bsize - 8], -15))
        at += bsize
    return b"".join(out)


def walk_records(raw):
    """Record offsets of an uncompressed BAM stream, walked sequentially after the header."""
    l_text = struct.unpack_from("<i", raw, 4)[0]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 4 + struct.unpack_from("<i", raw, at)[0] + 4
    offs = []
    while at < len(raw):
        offs.append(at)
        at += 4 + struct.unpack_from("<i", raw, at)[0]
    return offs
