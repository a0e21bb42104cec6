#!/usr/bin/env python3
"""Generate tests/golden/addmodel.json.gz by RUNNING THE REFERENCE's `addmodel` flow (add_model, advntr_commands.py:179-215:
ReferenceVNTR.init_from_vntrseek_data, VNTRFinder.train_classifier_threshold, save_reference_vntr_to_database) and its
`viewmodel` (view_model / print_models, advntr_commands.py:145-176) on a synthetic genome.  TEST INFRASTRUCTURE; only data is
written: the genome, the arguments of every call in order, every database row and the viewmodel stdout.

The reference's modules cannot be imported here (biopython and others are absent): the functions and classes named below are
compiled at run time from the reference files with `ast` and executed unchanged against the vendored pomegranate build
(oracle/tools/build_reference.py), with the same harness as make_training_golden.py.

    python oracle/tools/build_reference.py && python tests/golden/make_addmodel_golden.py
"""
import argparse
import ast
import contextlib
import gzip
import io
import json
import os
import sqlite3
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_training_golden as mtg                    # noqa: E402  (sets up sys.path for the reference build)

import numpy as np                                    # noqa: E402
from advntr import settings, hmm_utils                # noqa: E402

REF = "/root/reference/advntr"


def _pick(path, names, ns):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert {n.name for n in body} == set(names), (path, names)
    mod = ast.Module(body=body, type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, path, "exec"), ns)
    return ns


def load():
    finder = mtg.load_methods()

    def make_finder(ref_vntr):
        f = finder.__new__(finder)
        f.reference_vntr = ref_vntr
        f.min_repeat_bp_to_add_read = 2
        f.min_repeat_bp_to_count_repeats = 2
        return f
    ns = dict(build_reference_repeat_finder_hmm=hmm_utils.build_reference_repeat_finder_hmm,
              get_repeat_segments_from_visited_states_and_region=hmm_utils.get_repeat_segments_from_visited_states_and_region,
              get_chromosome_reference_sequence=None)
    _pick(os.path.join(REF, "reference_vntr.py"), ["ReferenceVNTR"], ns)
    ns.update(sqlite3=sqlite3, os=os, settings=settings)
    _pick(os.path.join(REF, "models.py"), ["create_vntrs_database", "load_unique_vntrs_data", "save_reference_vntr_to_database",
                                          "get_largest_id_in_database", "delete_vntr_from_database"], ns)
    ns.update(sys=sys, SeqIO=mtg._SeqIO, VNTRFinder=make_finder)
    _pick(os.path.join(REF, "advntr_commands.py"), ["print_error", "print_models", "view_model", "add_model", "del_model"], ns)
    return ns


def genome(rng):
    """Three chromosomes (<= 300 kb) with N runs, lower-case stretches, six loci and decoys of each."""
    dna = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    sizes = {"chr1": 120000, "chr2": 90000, "chr3": 60000}
    chroms = {k: list(dna(n)) for k, n in sizes.items()}
    loci = []
    spots = [("chr1", 20000), ("chr1", 70000), ("chr2", 15000), ("chr2", 60000), ("chr3", 30000), ("chr3", 650)]
    for name, start in spots:
        pattern = dna(int(rng.integers(8, 30)))
        segs = []
        for _ in range(int(rng.integers(3, 6))):
            u = list(pattern)
            if rng.random() < 0.5:
                u[int(rng.integers(0, len(u)))] = "ACGT"[int(rng.integers(0, 4))]
            segs.append("".join(u))
        vntr = "".join(segs)
        c = chroms[name]
        for _ in range(int(rng.integers(3, 7))):                 # decoys: mutated pieces of the locus elsewhere
            piece = list((vntr * 2)[int(rng.integers(0, 10)):][:int(rng.integers(60, 140))])
            for _ in range(int(rng.integers(0, 3))):
                piece[int(rng.integers(0, len(piece)))] = "ACGT"[int(rng.integers(0, 4))]
            at = int(rng.integers(0, len(c) - len(piece)))
            if abs(at - start) > 1500:
                c[at:at + len(piece)] = piece
        c[start:start + len(vntr)] = list(vntr)
        loci.append((name, start, start + len(vntr), pattern))
    for name, c in chroms.items():
        for _ in range(3):
            at = int(rng.integers(0, len(c) - 50))
            if all(abs(at - l[1]) > 1200 for l in loci if l[0] == name):
                c[at:at + int(rng.integers(1, 40))] = ["N"] * int(rng.integers(1, 40))
        for _ in range(2):
            at = int(rng.integers(0, len(c) - 400))
            c[at:at + 300] = [x.lower() for x in c[at:at + 300]]
    texts = {k: "".join(v)[:sizes[k]] for k, v in chroms.items()}
    fasta = "".join(">%s synthetic %d\n%s" % (k, i, "".join(t[j:j + 70] + "\n" for j in range(0, len(t), 70)))
                    for i, (k, t) in enumerate(texts.items()))
    return fasta, loci


def main():
    rng = np.random.default_rng(2024)
    fasta, loci = genome(rng)
    ns = load()
    settings.USE_TRAINED_HMMS = False
    settings.MAX_ERROR_RATE = 0.05
    hmm_utils.build_profile_hmm_for_repeats = \
        lambda repeats, error_rate: hmm_utils.build_profile_hmm_pseudocounts_for_alignment(error_rate, repeats)
    work = tempfile.mkdtemp()
    ref_file = os.path.join(work, "genome.fa")
    with open(ref_file, "w") as fh:
        fh.write(fasta)
    db = os.path.join(work, "models.db")
    calls = []
    for k, (name, start, end, pattern) in enumerate(loci):
        argv = ["-c", name, "-p", pattern, "-s", str(start), "-e", str(end)]
        if k == 1:
            argv += ["-g", "GENE1", "-a", "Coding"]
        args = argparse.Namespace(reference=ref_file, chromosome=name, pattern=pattern, start=start, end=end,
                                  gene="GENE1" if k == 1 else None, annotation="Coding" if k == 1 else None, models=db)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            ns["add_model"](args, None)
        calls.append({"args": argv, "stdout": out.getvalue()})
        print(out.getvalue().strip().splitlines()[-1])
    con = sqlite3.connect(db)
    rows = con.execute("SELECT id, nonoverlapping, chromosome, ref_start, gene_name, annotation, pattern, left_flanking, "
                       "right_flanking, repeats, scaled_score FROM vntrs ORDER BY id").fetchall()
    con.close()
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        ns["view_model"](argparse.Namespace(pattern=None, models=db, gene=""), None)
    by_pattern = io.StringIO()
    with contextlib.redirect_stdout(by_pattern):
        ns["view_model"](argparse.Namespace(pattern=loci[2][3].lower(), models=db, gene=""), None)
    by_gene = io.StringIO()
    with contextlib.redirect_stdout(by_gene):
        ns["view_model"](argparse.Namespace(pattern=None, models=db, gene="gene1,other"), None)
    ns["del_model"](argparse.Namespace(vntr_id=str(rows[2][0]), models=db), None)
    after_del = io.StringIO()
    with contextlib.redirect_stdout(after_del):
        ns["view_model"](argparse.Namespace(pattern=None, models=db, gene=""), None)
    result = {"fasta": fasta, "calls": calls, "rows": rows, "viewmodel": out.getvalue(),
              "viewmodel_pattern": [loci[2][3].lower(), by_pattern.getvalue()],
              "viewmodel_gene": ["gene1,other", by_gene.getvalue()],
              "delmodel": [str(rows[2][0]), after_del.getvalue()]}
    for r in rows:
        segs = r[9].split(",")
        print(r[0], r[2], r[3], len(segs), sorted(set(map(len, segs))), r[10])
    with gzip.open(os.path.join(HERE, "addmodel.json.gz"), "wt") as fh:
        json.dump(result, fh)


if __name__ == "__main__":
    main()
