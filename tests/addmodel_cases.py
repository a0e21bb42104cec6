"""Synthetic chromosomes and loci for the addmodel tests (CPU and GPU): random sequence with N runs, IUPAC codes, lower-case
stretches, low-complexity runs and planted copies of each locus's VNTR and flanks."""
import types

import numpy as np


def dna(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def make_locus(rng, chrom_len, pattern=None, start=None, copies=None):
    pattern = pattern or dna(rng, int(rng.integers(6, 40)))
    copies = copies or int(rng.integers(2, 6))
    segs = []
    for _ in range(copies):
        s = list(pattern)
        if rng.random() < 0.4:
            s[int(rng.integers(0, len(s)))] = "ACGT"[int(rng.integers(0, 4))]
        segs.append("".join(s))
    vntr = "".join(segs)
    if start is None:
        start = int(rng.integers(0, max(1, chrom_len - len(vntr))))
    return pattern, segs, start


def vntr_object(vid, chromosome, pattern, segs, start, chrom_text):
    left = chrom_text[max(0, start - 500):start].upper()
    vntr = "".join(segs)
    right = chrom_text[start + len(vntr):start + len(vntr) + 500].upper()
    return types.SimpleNamespace(id=vid, pattern=pattern, chromosome=chromosome, start_point=start, left_flanking_region=left,
                                 right_flanking_region=right, scaled_score=0, get_repeat_segments=lambda: segs,
                                 get_length=lambda: len(vntr))


def random_case(seed):
    """A small chromosome and 1-3 loci planted in it, with decoys, N runs, IUPAC codes and lower case."""
    rng = np.random.default_rng(seed)
    kind = seed % 6
    n = [11, 13, 140, 290, 1500, 6000][kind] if seed % 4 == 0 else int(rng.integers(12, 5000))
    chrom = list(dna(rng, n))
    loci = []
    for _ in range(int(rng.integers(1, 4))):
        pattern, segs, start = make_locus(rng, n)
        vntr = "".join(segs)
        chrom[start:start + len(vntr)] = list(vntr)
        chrom = chrom[:n]
        loci.append((pattern, segs, start))
    for _ in range(int(rng.integers(0, 6))):            # decoys: copies of locus pieces elsewhere, some near the ends
        pattern, segs, _ = loci[int(rng.integers(0, len(loci)))]
        piece = ("".join(segs) * 3)[:int(rng.integers(11, 160))]
        at = int(rng.choice([0, max(0, n - len(piece)), int(rng.integers(0, max(1, n)))]))
        chrom[at:at + len(piece)] = list(piece)
        chrom = chrom[:n]
    for _ in range(int(rng.integers(0, 4))):            # N runs
        at = int(rng.integers(0, max(1, n)))
        chrom[at:at + int(rng.integers(1, 30))] = ["N"]
        chrom = (chrom + list(dna(rng, n)))[:n]
    for _ in range(int(rng.integers(0, 4))):            # IUPAC codes, lower-case n
        at = int(rng.integers(0, max(1, n)))
        chrom[at] = str(rng.choice(list("RYKMSWnBDHV")))
    for _ in range(int(rng.integers(0, 3))):            # lower case
        at = int(rng.integers(0, max(1, n)))
        chrom[at:at + 200] = [c.lower() for c in chrom[at:at + 200]]
        chrom = chrom[:n]
    text = "".join(chrom)
    vntrs = [vntr_object(i, "chrT", p, s, st, text) for i, (p, s, st) in enumerate(loci)]
    if seed % 5 == 0 and len(vntrs) > 1:                # two loci sharing keywords and overlapping exclusion windows
        vntrs[1] = vntr_object(1, "chrT", vntrs[0].pattern, vntrs[0].get_repeat_segments(), vntrs[0].start_point + 7, text)
    if seed % 7 == 0:                                   # a keyword holding an N
        v = vntrs[0]
        v.left_flanking_region = v.left_flanking_region[:-5] + "N" + v.left_flanking_region[-4:]
    return text, vntrs



def synthetic_genome(seed, sizes, n_loci, low_complexity=0):
    """Chromosomes of the given sizes (text with N runs and lower-case stretches) and n_loci planted loci as rows
    (chrom, start, end, pattern, segments), spread evenly over the chromosomes, each with decoys (mutated pieces of itself)
    a few kb away.  The first `low_complexity` loci are poly-A: their keyword AAAAAAAAAAA hits in A runs planted all over
    their chromosome, so they reach the read cap part-way."""
    rng = np.random.default_rng(seed)
    names = ["chr%d" % (i + 1) for i in range(len(sizes))]
    chroms = {name: np.frombuffer(dna(rng, size).encode(), np.uint8).copy() for name, size in zip(names, sizes)}
    for name in names:
        s = chroms[name]
        n = len(s)
        for _ in range(max(1, n // 200000)):                      # N runs
            at = int(rng.integers(0, n))
            s[at:at + int(rng.integers(1, 3000))] = ord("N")
        for _ in range(max(1, n // 100000)):                      # lower case
            at = int(rng.integers(0, n))
            piece = s[at:at + int(rng.integers(100, 2000))]
            piece[piece < 97] += 32
        if low_complexity:
            for _ in range(n // 3000):                            # A runs for the poly-A keyword
                at = int(rng.integers(0, n))
                s[at:at + int(rng.integers(20, 40))] = ord("A")
    rows = []
    per_chrom = (n_loci + len(names) - 1) // len(names)
    for k in range(n_loci):
        name = names[k % len(names)]
        s = chroms[name]
        n = len(s)
        low = k < low_complexity
        pattern = "A" * 12 + "C" if low else dna(rng, int(rng.integers(6, 30)))
        segs = []
        for _ in range(int(rng.integers(3, 7))):
            u = list(pattern)
            if not low and rng.random() < 0.4:
                u[int(rng.integers(0, len(u)))] = "ACGT"[int(rng.integers(0, 4))]
            segs.append("".join(u))
        vntr = "".join(segs)
        slot = n // (per_chrom + 1)
        start = slot * (k // len(names) + 1) + int(rng.integers(-slot // 8, slot // 8))
        for _ in range(int(rng.integers(2, 6))):                  # decoys a few kb away
            piece = (vntr * 3)[int(rng.integers(0, len(pattern))):][:int(rng.integers(40, 150))]
            at = start + int(rng.choice([-1, 1])) * int(rng.integers(1500, 4000))
            if 0 <= at and at + len(piece) < n:
                s[at:at + len(piece)] = np.frombuffer(piece.encode(), np.uint8)
        s[start - 600:start + len(vntr) + 600] = np.frombuffer((dna(rng, 600) + vntr + dna(rng, 600)).encode(), np.uint8)
        rows.append((name, start, start + len(vntr), pattern, segs))
    texts = {name: chroms[name].tobytes().decode("latin-1") for name in names}
    return texts, rows
