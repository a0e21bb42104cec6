"""BAM input, host side (no GPU): the test writer against hand-written bytes, BGZF framing, the binary header, the
__host__ __device__ inflate core under ASan/UBSan (equal to zlib on a seeded corpus, errors without a sanitizer report on
mutated streams), and the sequential record walk and field decode of a host buffer."""
import gzip
import os
import random
import struct
import subprocess
import zlib

import pytest

from conftest import ROOT
import bam_writer as bw

REFS = [("chr1", 100000), ("chr2", 5000)]
RECORDS = [
    ("r1", 0, "chr1", 101, 60, "4M2D2M1I2M3S", "ACGTACGTACGT", "IIIIIIIIIIII"),
    ("r2", 1024, "chr1", 201, 0, "12M", "ACGTACGTACGT", "#" + "I" * 11),
    ("r3", 4, "*", 0, 0, "*", "ACGTNACGT", "*"),
    ("r4", 16, "chr2", 11, 30, "5M100N5M", "ACGTACGTAC", "IIIIIIIIII"),
    ("r5", 4, "chr2", 40, 0, "*", "*", "*"),
    ("r6", 0, "chr1", 300, 37, "1M1I1D1N1S1H1P1=1X", "=ACMGRSVTWYHKDBN", "ABCDEFGHIJKLMNOP"),
    ("r7", 0, "chr2", 90, 20, "*", "GATTACA", "IIIIIII"),
]


def test_writer_matches_hand_written_bytes():
    # the spec's EOF block
    assert bw.EOF_BLOCK == bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0] + [0] * 8)
    assert zlib.decompress(bw.EOF_BLOCK[18:-8], -15) == b""
    # a header with two references and no text
    assert bw.bam_header([("chr1", 248956422), ("chrM", 16569)], "") == (
        b"BAM\x01" + b"\x00\x00\x00\x00" + b"\x02\x00\x00\x00" +
        b"\x05\x00\x00\x00chr1\x00" + b"\x06\xc6\xd6\x0e" + b"\x05\x00\x00\x00chrM\x00" + b"\xb9\x40\x00\x00")
    # one record: name "q", flag 0, chr1:11 (pos 10), mapq 60, 2M1I, seq ACG, qual II (+33 -> 40)
    rec = bw.bam_record(("q", 0, "chr1", 11, 60, "2M1I", "ACG", "III"), {"chr1": 0})
    body = (b"\x00\x00\x00\x00" + b"\x0a\x00\x00\x00" + b"\x02" + b"\x3c" + struct.pack("<H", 4681) + b"\x02\x00" + b"\x00\x00" +
            b"\x03\x00\x00\x00" + b"\xff\xff\xff\xff" * 2 + b"\x00\x00\x00\x00" + b"q\x00" +
            b"\x20\x00\x00\x00" + b"\x11\x00\x00\x00" + b"\x12\x40" + b"\x28\x28\x28")
    assert rec == struct.pack("<i", len(body)) + body


def _bam(tmp_path, name="s.bam", framing="htslib", records=RECORDS, refs=REFS, **kw):
    data = bw.write_bam(refs, records, framing, **kw)
    p = tmp_path / name
    p.write_bytes(data)
    return str(p), data


def test_framing_scan(tmp_path):
    from advntr_amd import bam
    pieces = [os.urandom(100), b"A" * 65536, b"", b"xyz" * 1000]
    data = bw.bgzf_blocks(pieces, modes=((6, "default"), (9, "rle"), (1, "fixed")))
    off, size, isize = bam.scan_framing(data)
    want_off, at = [], 0
    while at < len(data):
        want_off.append(at)
        at += struct.unpack_from("<H", data, at + 16)[0] + 1
    assert list(off) == want_off
    assert list(isize) == [100, 65536, 0, 3000, 0]
    assert int(size.sum()) == len(data)
    from advntr_amd import _lib
    with pytest.raises(_lib.EngineError, match="truncated"):
        bam.scan_framing(data[:-5])
    with pytest.raises(_lib.EngineError, match="not BGZF"):
        bam.scan_framing(gzip.compress(b"hello"))
    big = bytearray(bw.bgzf_block(b"x" * 10))
    big[-4:] = struct.pack("<I", 65537)
    with pytest.raises(_lib.EngineError, match="ISIZE above 65536"):
        bam.scan_framing(bytes(big))


def test_header_names_from_binary_list(tmp_path):
    from advntr_amd import bam
    text = "@HD\tVN:1.6\n@SQ\tSN:wrong\tLN:1\n"          # the @SQ text is not what names the references
    path, _ = _bam(tmp_path, refs=[("1", 249250621), ("X", 155270560), ("chrUn_gl000220", 161802)], records=[], text=text)
    names, lengths, hbytes = bam.read_header(path)
    assert names == ["1", "X", "chrUn_gl000220"]
    assert lengths == [249250621, 155270560, 161802]
    assert hbytes == 8 + len(text) + 4 + (4 + 2 + 4) * 2 + 4 + 15 + 4
    # a header larger than one block
    refs = [("contig_%05d" % i, 1000 + i) for i in range(6000)]
    path, _ = _bam(tmp_path, "big.bam", refs=refs, records=[])
    names, lengths, _ = bam.read_header(path)
    assert names == [r[0] for r in refs] and lengths == [r[1] for r in refs]


def _corpus(rng):
    """(raw deflate stream, its input) pairs over levels, strategies and data shapes"""
    datas = [b"", b"a", bytes(rng.getrandbits(8) for _ in range(5000)), b"ACGT" * 5000, b"\0" * 65536,
             bytes(rng.choice(b"ACGTN") for _ in range(60000)),
             (b"x" + bytes(rng.getrandbits(8) for _ in range(258))) * 200,           # matches of length 258
             bytes(rng.getrandbits(8) for _ in range(32768)) * 2]                     # distance 32 768
    out = []
    for d in datas:
        for level in (0, 1, 6, 9):
            for strat in bw.STRATEGIES:
                c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, bw.STRATEGIES[strat])
                out.append((c.compress(d) + c.flush(), d))
    return out


def _run_core(tmp_path, cases):
    exe = str(tmp_path / "asan_inflate")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "native", "asan_inflate.cpp")])
    with open(tmp_path / "in.bin", "wb") as fh:
        for stream, cap in cases:
            fh.write(struct.pack("<II", len(stream), cap) + stream)
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    assert out.stdout.decode() == "ok %d\n" % len(cases)
    res, raw, at = [], (tmp_path / "out.bin").read_bytes(), 0
    while at < len(raw):
        rc, n = struct.unpack_from("<iI", raw, at)
        res.append((rc, raw[at + 8:at + 8 + n]))
        at += 8 + n
    return res


def test_inflate_core_equals_zlib_under_asan(tmp_path):
    corpus = _corpus(random.Random(11))
    res = _run_core(tmp_path, [(s, len(d)) for s, d in corpus])
    for (s, d), (rc, got) in zip(corpus, res):
        assert rc == 0 and got == d


def _fixed_stream(symbols):
    """A final fixed-Huffman block of (kind, value) symbols, written bit by bit (to make invalid ones)."""
    bits = [1, 1, 0]                        # BFINAL, BTYPE = 01 (LSB first)

    def code(sym):
        if sym < 144:
            c, n = 0x30 + sym, 8
        elif sym < 256:
            c, n = 0x190 + sym - 144, 9
        elif sym < 280:
            c, n = sym - 256, 7
        else:
            c, n = 0xc0 + sym - 280, 8
        return [(c >> (n - 1 - i)) & 1 for i in range(n)]       # Huffman codes go MSB first
    for kind, v in symbols:
        if kind == "lit":
            bits += code(v)
        elif kind == "raw":                 # extra bits / a distance code, LSB first
            val, n = v
            bits += [(val >> i) & 1 for i in range(n)]
        elif kind == "dist":                # 5-bit fixed distance code, MSB first
            bits += [(v >> (4 - i)) & 1 for i in range(5)]
    bits += [0] * (-len(bits) % 8)
    return bytes(sum(bits[i + k] << k for k in range(8)) for i in range(0, len(bits), 8))


def test_inflate_core_rejects_malformed_streams_under_asan(tmp_path):
    rng = random.Random(5)
    good = [s for s, d in _corpus(random.Random(3)) if len(d) > 1000][::3]
    cases, expect_error = [], []
    for s in good:
        d = zlib.decompress(s, -15)
        for _ in range(6):                                   # bit flips: an error or some output, never a sanitizer report
            m = bytearray(s)
            m[rng.randrange(len(m))] ^= 1 << rng.randrange(8)
            cases.append((bytes(m), len(d)))
            expect_error.append(None)
        cases.append((s[:len(s) // 2], len(d)))             # truncated
        expect_error.append(True)
        cases.append((s, len(d) // 2))                       # capacity (ISIZE) below the output
        expect_error.append(True)
    # distance beyond the output: literal 'a', then length 3 (257) at distance 2 (dist code 1)
    cases.append((_fixed_stream([("lit", 97), ("lit", 257), ("dist", 1), ("lit", 256)]), 100))
    expect_error.append(6)
    # the same at distance 1 is valid: "aaaa"
    cases.append((_fixed_stream([("lit", 97), ("lit", 257), ("dist", 0), ("lit", 256)]), 100))
    expect_error.append(0)
    # length symbol 286 and distance symbol 30 are invalid
    cases.append((_fixed_stream([("lit", 97), ("lit", 286), ("lit", 256)]), 100))
    expect_error.append(5)
    cases.append((_fixed_stream([("lit", 97), ("lit", 257), ("dist", 30), ("lit", 256)]), 100))
    expect_error.append(5)
    # dynamic block with an over-subscribed code-length code: HCLEN = 4 lengths, all 1
    bits = [1, 0, 1] + [0] * 5 + [0] * 5 + [0, 0, 0, 0] + [1, 0, 0] * 4
    over = bytes(sum((bits + [0] * (-len(bits) % 8))[i + k] << k for k in range(8)) for i in range(0, len(bits) + (-len(bits) % 8), 8))
    cases.append((over + b"\0" * 8, 100))
    expect_error.append(4)
    # incomplete code-length code: HCLEN = 4 lengths 2, 0, 0, 0 (one code of length 2)
    bits = [1, 0, 1] + [0] * 5 + [0] * 5 + [0, 0, 0, 0] + [0, 1, 0] + [0, 0, 0] * 3
    inc = bytes(sum((bits + [0] * (-len(bits) % 8))[i + k] << k for k in range(8)) for i in range(0, len(bits) + (-len(bits) % 8), 8))
    cases.append((inc + b"\0" * 8, 100))
    expect_error.append(4)
    cases.append((b"\x07", 10))                              # BTYPE 3
    expect_error.append(1)
    cases.append((b"\x01\x05\x00\x00\x00", 10))              # stored: LEN 5, NLEN 0
    expect_error.append(2)
    cases.append((b"", 10))
    expect_error.append(3)
    res = _run_core(tmp_path, cases)
    for (s, cap), want, (rc, got) in zip(cases, expect_error, res):
        if want is True:
            assert rc != 0
        elif want is not None:
            assert rc == want, (want, rc, s.hex())
        if want == 0:
            assert got == b"aaaa"
        assert len(got) <= cap
    # every flipped stream either fails or inflates to what zlib makes of it
    for (s, cap), want, (rc, got) in zip(cases, expect_error, res):
        if want is None and rc == 0:
            try:
                z = zlib.decompressobj(-15)
                ref = z.decompress(s, cap + 1)
                ok = z.eof
            except zlib.error:
                ok = False
            if ok:
                assert got == ref


def test_host_walk_and_field_decode(tmp_path):
    from advntr_amd import bam, sam_utils
    path, data = _bam(tmp_path)
    raw = bw.inflate_all(data)
    names, _, hbytes = bam.read_header(path)
    offs, end = bam.walk_host(raw, hbytes)
    assert list(offs) == bw.walk_records(raw) and end == len(raw)
    reads = bam.decode_host(raw, offs, names)
    want = sam_utils.parse_sam(bw.sam_text(REFS, RECORDS)).reads
    assert len(reads) == len(want)
    for r, w in zip(reads, want):
        for a in SamReadFields:
            assert getattr(r, a) == getattr(w, a), (w.query_name, a)
    # a record cut short: the walk stops before it; a block_size below the fixed part is an error
    offs2, end2 = bam.walk_host(raw[:len(raw) - 3], hbytes)
    assert list(offs2) == list(offs[:-1]) and end2 == offs[-1]
    bad = bytearray(raw)
    struct.pack_into("<i", bad, int(offs[2]), 7)
    from advntr_amd import _lib
    with pytest.raises(_lib.EngineError, match="block_size"):
        bam.walk_host(bytes(bad), hbytes)


SamReadFields = ("query_name", "flag", "reference_name", "reference_start", "reference_end", "mapq", "cigar", "seq",
                 "query_qualities")


def test_sniff_kinds(tmp_path):
    from advntr_amd import bam
    path, _ = _bam(tmp_path)
    assert bam.sniff(path) == "bgzf"
    (tmp_path / "a.gz").write_bytes(gzip.compress(b"x"))
    assert bam.sniff(str(tmp_path / "a.gz")) == "gzip"
    (tmp_path / "a.cram").write_bytes(b"CRAM\3\0" + b"\0" * 30)
    assert bam.sniff(str(tmp_path / "a.cram")) == "cram"
    (tmp_path / "a.sam").write_text(bw.sam_text(REFS, RECORDS))
    assert bam.sniff(str(tmp_path / "a.sam")) == "text"


def test_device_entry_points_fail_loudly_without_gpu(tmp_path):
    from advntr_amd import _lib, bam
    if _lib.load().advntr_device_count() > 0:
        pytest.skip("a GPU is present")
    path, data = _bam(tmp_path)
    with pytest.raises(_lib.EngineError, match="no HIP device"):
        bam.inflate(data)
    with pytest.raises(_lib.EngineError, match="no HIP device"):
        bam.open_alignment(path, [("chr1", 0, 1000)])
