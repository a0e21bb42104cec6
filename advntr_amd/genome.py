"""A whole reference genome from FASTA, for `addmodel`: one linear pass over the file, chromosomes kept as uint8 arrays.

A record id is the first whitespace-delimited word after '>' (what Bio.SeqIO's fasta parser gives as .id).  Sequence lines may
be wrapped and end in CRLF; blank lines and whitespace are dropped.  Case is kept: false reads are cut from the text as it is.
Two records with one id are refused (the reference would mix their hits silently).
"""
import time

import numpy as np

_WHITESPACE = np.zeros(256, dtype=bool)
for _c in b" \t\n\r\v\f":
    _WHITESPACE[_c] = True


class Chromosome(object):
    """The bytes of one record.  Slicing gives a str (Python slice semantics, a negative start included), so the
    reference's string code (init_from_vntrseek_data) runs on a piece without a str of the whole chromosome."""
    __slots__ = ("name", "codes")

    def __init__(self, name, codes):
        self.name = name
        self.codes = codes                      # uint8[n], the FASTA bytes without line breaks

    def __len__(self):
        return len(self.codes)

    def __getitem__(self, key):
        if not isinstance(key, slice):
            raise TypeError("a Chromosome is sliced, not indexed")
        return self.codes[key].tobytes().decode("latin-1")


class Genome(object):
    def __init__(self, chromosomes, seconds, path=None):
        self.chromosomes = chromosomes          # name -> Chromosome, in file order
        self.seconds = seconds                  # wall time of the read
        self.path = path

    def __contains__(self, name):
        return name in self.chromosomes

    def __getitem__(self, name):
        return self.chromosomes[name]

    def names(self):
        return list(self.chromosomes)

    def total_bases(self):
        return sum(len(c) for c in self.chromosomes.values())


def parse_fasta_bytes(data, path="<bytes>"):
    """Records of FASTA text held in a bytes object -> Genome."""
    t0 = time.perf_counter()
    view = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(0, np.uint8)
    chromosomes = _records(data, view, path)
    return Genome(chromosomes, time.perf_counter() - t0, path)


def _records(data, view, path):
    chromosomes = {}
    size = len(data)
    at = 0
    while at < size and _WHITESPACE[view[at]]:
        at += 1
    if at < size and view[at] != ord(">"):
        raise ValueError("%s: not FASTA (the first record does not start with '>')" % path)
    while at < size:
        eol = data.find(b"\n", at)
        eol = size if eol < 0 else eol
        header = bytes(data[at + 1:eol]).decode("latin-1").split()
        nxt = data.find(b"\n>", eol)
        end = size if nxt < 0 else nxt + 1
        if not header:
            raise ValueError("%s: a record without an id at byte %d" % (path, at))
        name = header[0]
        if name in chromosomes:
            raise ValueError("%s: record id %r occurs twice" % (path, name))
        body = view[min(eol + 1, size):end]
        chromosomes[name] = Chromosome(name, np.ascontiguousarray(body[~_WHITESPACE[body]]))
        at = end
    return chromosomes


def read_genome(path):
    """The records of a FASTA file, read whole and parsed in one pass."""
    t0 = time.perf_counter()
    with open(path, "rb") as fh:
        data = fh.read()
    genome = parse_fasta_bytes(data, path)
    genome.seconds = time.perf_counter() - t0
    return genome
