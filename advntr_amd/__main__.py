"""Thin command line over the engine: `python -m advntr_amd genotype --loci loci.json --reads reads.fa`, and the model
database commands `addmodel`, `delmodel` and `viewmodel` (advntr_commands.py:145-223).

Not a re-implementation of the reference's CLI (/root/reference/advntr/__main__.py, advntr_commands.py: CRAM input is
out of scope; --alignment takes BAM or SAM text).  It strings the GPU stages together
for reads that are already extracted: keyword prefilter -> per-locus Viterbi scoring of both strands -> recruit ->
Illumina aggregation (or PacBio dominant copy numbers) -> the reference's text output (genome_analyzer.py:158-170:
the VNTR id on one line, the genotype `a/b` on the next).

Loci come from --loci loci.json or from --models FILE.db, the reference's sqlite model database (table `vntrs`,
advntr/models.py:120-161), optionally narrowed with --vntr-id.  Repeat segments of unequal length need --align-repeats
(the library's own aligner stands in for the reference's `muscle` call).

loci.json: [{"id": 301645, "left": "...", "right": "...", "pattern": "...", "repeat_segments": ["...", ...],
             "scaled_score": -1.1}, ...]   (repeat_segments pre-aligned when more than one, equal length)
reads.fa : two-line FASTA (name line, sequence line), the format adVNTR-Filtering reads (filtering/main.cc:247-252).
"""
import argparse
import json
import sys



def _read_fasta(path):
    """Names and sequences of a FASTA file (sequence lines may be wrapped) or a four-line FASTQ file."""
    names, seqs = [], []
    with open(path) as fh:
        first = fh.readline()
        if first.startswith("@"):                                   # FASTQ: name, sequence, '+', qualities
            lines = [first] + fh.readlines()
            lines = [l.rstrip("\r\n") for l in lines]
            while lines and not lines[-1].strip():                  # trailing blank lines are not records
                lines.pop()
            if len(lines) % 4:
                raise ValueError("%s: FASTQ needs four lines per record (multi-line records are not supported)" % path)
            for i in range(0, len(lines), 4):
                if not lines[i].startswith("@") or not lines[i + 2].startswith("+"):
                    raise ValueError("%s: malformed FASTQ record at line %d" % (path, i + 1))
                names.append(lines[i][1:])
                seqs.append(lines[i + 1])
            return names, seqs
        chunks = None
        for line in [first] + fh.readlines():
            line = line.rstrip("\n")
            if line.startswith(">"):
                if chunks is not None:
                    seqs.append("".join(chunks))
                names.append(line[1:])
                chunks = []
            elif chunks is not None and line:
                chunks.append(line)
        if chunks is not None:
            seqs.append("".join(chunks))
    return names, seqs


def genotype(args):
    from . import filtering, hmm_utils, settings, vntr_finder
    settings.ALIGN_REPEATS = bool(args.align_repeats)
    from . import models
    if args.models:
        wanted = set(args.vntr_id or ())
        loci = [{"id": v.id, "left": v.left_flanking_region, "right": v.right_flanking_region, "pattern": v.pattern,
                 "repeat_segments": v.get_repeat_segments() or [v.pattern],
                 "scaled_score": v.scaled_score if v.scaled_score else None, "vntr": v}
                for v in models.load_unique_vntrs_data(args.models)
                if (not wanted or v.id in wanted) and v.left_flanking_region and v.right_flanking_region]
    else:
        loci = json.load(open(args.loci))
        for loc in loci:        # optional fields of the BED / VCF rows
            v = models.ReferenceVNTR(loc["id"], loc["pattern"], loc.get("start_point", 0), loc.get("chromosome", "chrUn"),
                                     loc.get("gene_name"), loc.get("annotation"), len(loc["repeat_segments"]))
            v.init_from_xml(loc["repeat_segments"], loc["left"], loc["right"])
            loc["vntr"] = v
    from . import comm as comm_mod, genome_analyzer, sharding
    comm = args.comm = comm_mod.init_from_env()       # one process per GPU under a launcher; None for a plain run
    rank = comm.rank if comm is not None else 0
    if rank == 0 and not args.frameshift:
        if args.outfmt == "bed":
            sys.stdout.write(genome_analyzer.bed_header(args.haploid))
        elif args.outfmt == "vcf":
            sys.stdout.write(genome_analyzer.vcf_header([loc["vntr"] for loc in loci], args.reads or args.alignment))

    def row(loc, result):
        return genome_analyzer.genotype_row(args.outfmt, loc["vntr"], loc["id"], result, False, args.haploid)

    def finish(rows):          # rows of all loci are back on rank 0, in locus order
        if rows is not None:
            sys.stdout.write("".join(rows))
        return 0
    names, seqs = _read_fasta(args.reads) if args.reads else ([], [])
    samfile = None
    if args.alignment and args.pacbio:
        settings.MAX_ERROR_RATE = 0.3                                           # advntr_commands.py:66-71
        return finish(sharding.run_sharded([len(loc["pattern"]) for loc in loci],
                                           _pacbio_alignment_job(args, loci, seqs, row), comm))
    measured = None
    if args.alignment:     # mapped reads are selected per locus, unmapped ones join --reads
        from . import bam, coverage as coverage_mod
        auto = bool(args.expansion) and args.coverage == "auto"
        reference_genome = None
        if auto and args.reference_filename:
            from . import genome
            try:
                reference_genome = genome.read_genome(args.reference_filename)
            except (OSError, ValueError) as e:
                raise SystemExit("ERROR: %s" % e)
        kind = bam.sniff(args.alignment)
        if kind == "bgzf":     # BAM: one pass on the GPU keeps the records of the loci's windows and the unmapped ones
            references, lengths, _ = bam.read_header(args.alignment)
            if auto:           # a genome that does not fit the header is refused before the pass
                _coverage_checked(coverage_mod.layout, references, lengths, reference_genome)
            samfile = bam.open_alignment(args.alignment, bam.vntr_windows(references, [loc["vntr"] for loc in loci]),
                                         coverage=auto, genome=reference_genome)
            measured = samfile.coverage
        elif kind == "text":   # SAM text (`samtools view -h`)
            from . import sam_utils
            with open(args.alignment) as fh:
                text = fh.read()
            samfile = sam_utils.parse_sam(text)
            if auto:           # the same rule on the host
                measured = _coverage_checked(coverage_mod.measure_sam, samfile, coverage_mod.sam_reference_lengths(text),
                                             reference_genome)
        else:
            raise SystemExit("%s: %s input is not supported (--alignment takes BAM or SAM text)" %
                             (args.alignment, "CRAM" if kind == "cram" else "gzip that is not BGZF"))
        seqs = seqs + [r.seq for r in samfile.reads if r.is_unmapped]
    divisors = _expansion_divisors(args, loci, samfile, measured, rank)
    settings.MAX_ERROR_RATE = 0.3 if args.pacbio else 0.05                      # advntr_commands.py:66-71
    if args.pacbio:
        def pacbio_job(indices):
            if args.extract_spanning:
                # whole long reads: extraction, per-locus models, scoring and the call for all of this rank's loci at once
                # (find_repeat_count_from_pacbio_reads, vntr_finder.py:652-665; every read is a candidate of every locus)
                desc = [(loci[i]["left"], loci[i]["right"], loci[i]["repeat_segments"], loci[i]["pattern"]) for i in indices]
                res = vntr_finder.genotype_pacbio_loci(desc, [seqs] * len(desc), accuracy_filter=args.accuracy_filter,
                                                       is_haploid=args.haploid, chunks=max(1, min(8, len(desc) // 4)))
                return [row(loci[i], r) for i, r in zip(indices, res)]
            out = []
            for i in indices:
                loc = loci[i]
                spanning = [s.upper() for s in seqs]
                if args.extract_spanning:       # untrimmed long reads: keep the ones that span the VNTR, trimmed to its flanks
                    spanning = [t[0] for t in vntr_finder.extract_spanning_reads(loc["left"], loc["right"], seqs)[0]]
                geno, prob = vntr_finder.get_dominant_copy_numbers_from_spanning_reads(
                    loc["left"], loc["right"], loc["repeat_segments"], loc["pattern"], spanning,
                    accuracy_filter=args.accuracy_filter, is_haploid=args.haploid)
                out.append(row(loc, vntr_finder.GenotypeResult(geno, len(spanning), len(spanning), 0, prob)))
            return out
        return finish(sharding.run_sharded([len(loc["pattern"]) for loc in loci], pacbio_job, comm))
    # Illumina: prefilter every read against all loci at once.  The reference runs adVNTR-Filtering on the reads as
    # they are (genome_analyzer.py:173-199), so a read sequenced from the opposite strand only passes through keywords
    # that happen to be reverse-palindromic; --prefilter-both-strands (off by default = the reference's candidate sets)
    # also scans the reverse complements and unions the hits.
    fasta = "".join(">%d\n%s\n" % (i, s.upper()) for i, s in enumerate(seqs))
    keywords = {int(loc["id"]): filtering.get_keywords_for_filtering(loc["left"], loc["repeat_segments"], loc["right"],
                                                                       loc["pattern"], True, 15) for loc in loci}
    _, ids_fwd = filtering.get_filtered_read_ids(fasta, keywords, min_matches=args.min_matches)
    ids_rev = {}
    if args.prefilter_both_strands:
        rc = "".join(">%d\n%s\n" % (i, vntr_finder.reverse_complement(s.upper()) if "N" not in s.upper() else s.upper())
                     for i, s in enumerate(seqs))
        _, ids_rev = filtering.get_filtered_read_ids(rc, keywords, min_matches=args.min_matches)
    head = [len(r.seq) for r in samfile.head(5)] if samfile is not None else [len(s) for s in seqs[:5]]
    read_length = sorted(head)[len(head) // 2] if head else 150                   # vntr_finder.py:714-718
    def candidates(loc):
        vid = int(loc["id"])
        return [seqs[i] for i in sorted(set(int(n) for n in ids_fwd.get(vid, ())) | set(int(n) for n in ids_rev.get(vid, ())))]

    cands = [candidates(loc) for loc in loci]
    # whole loci go to ranks by estimated work (calls x states); one process per GPU under a launcher
    # (`python -m torch.distributed.run --nproc-per-node N -m advntr_amd genotype ...` or any other that sets RANK /
    # LOCAL_RANK / WORLD_SIZE / MASTER_PORT), rows gathered to rank 0 over RCCL; a plain loop over everything otherwise
    work = [max(1, len(c)) * (6 * read_length + 3 * vntr_finder.get_copies_for_hmm(read_length, len(loc["pattern"])) *
                              (len(loc["repeat_segments"][0]) + 1) + 18) for loc, c in zip(loci, cands)]
    if args.frameshift:        # genome_analyzer.py:260-271: the id, then the frameshift state label or None
        def frameshift_job(indices):
            out = []
            for i in indices:
                out.append(_frameshift_row(loci[i], cands[i], read_length, hmm_utils, vntr_finder))
            return out
        return finish(sharding.run_sharded(work, frameshift_job, comm))
    def genotype_job(indices):
        # all models of this rank's share in one native build, all (read, strand, locus) calls in one engine batch
        specs = [(loci[i]["left"][-read_length:], loci[i]["right"][:read_length], loci[i]["repeat_segments"],
                  vntr_finder.get_copies_for_hmm(read_length, len(loci[i]["pattern"]))) for i in indices]
        built = hmm_utils.build_read_matcher_models(specs)
        if samfile is not None:     # vntr_finder.py:701-767: mapped reads over the locus + the filtered unmapped ones
            for i in indices:
                loci[i]["vntr"].scaled_score = loci[i].get("scaled_score")
            picked, _ = vntr_finder.select_illumina_reads_multi([loci[i]["vntr"] for i in indices], samfile,
                                                                [cands[i] for i in indices], models=built)
            return [row(loci[i], vntr_finder.find_repeat_count_from_selected_reads(
                [s.summary for s in sel], accuracy_filter=args.accuracy_filter, average_coverage=divisors[i],
                is_haploid=args.haploid)) for i, sel in zip(indices, picked)]
        # scoring (both strands), recruit rule, selection and the per-locus aggregation + genotype without a Python object
        # per read: one engine batch, then advntr_genotype_illumina on the summary records
        results = vntr_finder.genotype_loci(built, [cands[i] for i in indices], [loci[i].get("scaled_score") for i in indices],
                                            accuracy_filter=args.accuracy_filter, is_haploid=args.haploid)
        return [row(loci[i], res) for i, res in zip(indices, results)]
    return finish(sharding.run_sharded(work, genotype_job, comm))


def _pacbio_alignment_job(args, loci, seqs, row):
    """find_repeat_counts_from_pacbio_alignment_file (genome_analyzer.py:210-233, vntr_finder.py:640-651): per locus, the mapped
    records that span it, trimmed by their CIGAR (on the device for BAM, vntr_finder's mirror for SAM text), joined by the
    unmapped records (+ --reads) that pass the long-read keyword filter and span it by flank alignment; one genotype step for
    all loci of a rank.  Returns the sharded job."""
    from . import bam, filtering, vntr_finder
    vntrs = [loc["vntr"] for loc in loci]
    kind = bam.sniff(args.alignment)
    if kind == "bgzf":
        references = bam.read_header(args.alignment)[0]
        windows = [w + (i,) for i, w in enumerate(bam.vntr_windows(references, vntrs))]
        spans = bam.open_alignment_spans(args.alignment, windows)
        mapped = [[t[1] for t in ts] for ts in spans.spanning(len(loci))]
        unmapped = [r.seq for r in spans.unmapped]
    elif kind == "text":
        from . import sam_utils
        with open(args.alignment) as fh:
            samfile = sam_utils.parse_sam(fh.read())
        mapped = [[t[1] for t in vntr_finder.get_spanning_reads_of_aligned_pacbio_reads(v, samfile)] for v in vntrs]
        unmapped = [r.seq for r in samfile.reads if r.is_unmapped]
    else:
        raise SystemExit("%s: %s input is not supported (--alignment takes BAM or SAM text)" %
                         (args.alignment, "CRAM" if kind == "cram" else "gzip that is not BGZF"))
    seqs = seqs + unmapped
    # adVNTR-Filtering with the long-read keywords (the flanks' last / first 80 bases, vntr_finder.py:151-152)
    fasta = "".join(">%d\n%s\n" % (i, s.upper()) for i, s in enumerate(seqs))
    keywords = {int(loc["id"]): filtering.get_keywords_for_filtering(loc["left"], loc["repeat_segments"], loc["right"],
                                                                       loc["pattern"], False) for loc in loci}
    _, ids = filtering.get_filtered_read_ids(fasta, keywords, min_matches=args.min_matches)
    cands = [[seqs[i] for i in sorted(int(n) for n in ids.get(int(loc["id"]), ()))] for loc in loci]

    def job(indices):
        unaligned = vntr_finder.extract_spanning_reads_multi([(loci[i]["left"], loci[i]["right"]) for i in indices],
                                                            [cands[i] for i in indices])
        desc = [(loci[i]["left"], loci[i]["right"], loci[i]["repeat_segments"], loci[i]["pattern"]) for i in indices]
        spanning = [mapped[i] + [t[0] for t in u[0]] for i, u in zip(indices, unaligned)]
        res = vntr_finder.genotype_pacbio_loci(desc, spanning, accuracy_filter=args.accuracy_filter, is_haploid=args.haploid,
                                               chunks=max(1, min(8, len(desc) // 4)), trimmed=True)
        return [row(loci[i], r) for i, r in zip(indices, res)]
    return job


def _frameshift_row(loc, cand, read_length, hmm_utils, vntr_finder):
    copies = vntr_finder.get_copies_for_hmm(read_length, len(loc["pattern"]))
    model = hmm_utils.get_read_matcher_model(loc["left"][-read_length:], loc["right"][:read_length],
                                             loc["repeat_segments"], copies)
    result = vntr_finder.find_frameshift(model, len(loc["pattern"]), sum(len(x) for x in loc["repeat_segments"]), cand,
                                         loc.get("scaled_score"))
    return "%s\n%s\n" % (loc["id"], result)


def _coverage_arg(text):
    """-c: a float as the reference's type=float, or `auto`"""
    if text == "auto":
        return text
    try:
        return float(text)
    except ValueError:
        raise argparse.ArgumentTypeError("%r is neither a number nor `auto`" % text)


def _coverage_checked(fn, *a):
    """fn(*a), its ValueError (an alignment header and a genome that do not fit) as the command's error"""
    try:
        return fn(*a)
    except ValueError as e:
        raise SystemExit("ERROR: -c auto: %s" % e)


def _expansion_divisors(args, loci, samfile, measured, rank):
    """The average coverage to divide by, per locus: -c's value, or (-c auto) what was measured.  In auto mode rank 0 writes
    one JSON line to stderr: where the divisor comes from, the sequencing mean, the windows, (windows, mean) per GC bin."""
    if not args.expansion:
        return [None] * len(loci)
    if args.coverage != "auto":
        return [args.coverage] * len(loci)
    try:
        out, empty = [], []
        for loc in loci:
            d, source = measured.divisor(loc["repeat_segments"])
            out.append(d)
            if source == "sequencing_mean_empty_bin":
                empty.append(loc["id"])
        summary = measured.summary()
    except ValueError as e:
        raise SystemExit("ERROR: -c auto: %s" % e)
    if rank == 0:
        for vid in empty:
            sys.stderr.write("coverage: the GC bin of VNTR %s holds no window; its divisor is the sequencing mean\n" % vid)
        sys.stderr.write(json.dumps({"coverage": summary}) + "\n")
    return out


def _print_error(parser, msg):
    """advntr_commands.py:23-25: the command's help, then the error, exit status 1."""
    parser.print_help()
    sys.exit("\nERROR: %s" % msg)


def _print_models(reference_vntrs):
    """print_models, advntr_commands.py:145-153 (its tabs included)."""
    print('VNTR ID\t| Chr\t| Gene\t| Start Position | Pattern')
    print('--------------------------------------------------')
    for ref_vntr in reference_vntrs:
        gene_name = ref_vntr.gene_name
        if len(gene_name) < 7:
            gene_name += '\t'
        print('%s\t| %s\t|%s| %s\t | %s' % (ref_vntr.id, ref_vntr.chromosome, gene_name, ref_vntr.start_point,
                                            ref_vntr.pattern))


def view_model(args, parser):
    """view_model, advntr_commands.py:156-176."""
    from . import models
    if args.pattern:
        for element in set(args.pattern.upper()):
            if element not in {'A', 'C', 'G', 'T'}:
                _print_error(parser, 'Pattern should only contain A, C, G, T')
    if args.models is None:
        _print_error(parser, '--models is required')
    genes = [gene.upper() for gene in args.gene.split(',') if gene]
    results = []
    for ref_vntr in models.load_unique_vntrs_data(args.models):
        if len(genes) and ref_vntr.gene_name.upper() not in genes:
            continue
        if args.pattern and ref_vntr.pattern != args.pattern.upper():
            continue
        results.append(ref_vntr)
    _print_models(results)
    return 0


def del_model(args, parser):
    """del_model, advntr_commands.py:218-223."""
    from . import models
    if not args.vntr_id:
        _print_error(parser, '--vntr_id is required')
    if args.models is None:
        _print_error(parser, '--models is required')
    models.delete_vntr_from_database(args.vntr_id, args.models)
    return 0


def add_model(args, parser):
    """add_model, advntr_commands.py:179-215, for one locus or (--regions) many: every locus is set up, then all are trained
    together (one GPU scan per chromosome, one scoring batch) and written in one transaction."""
    from . import genome, settings, training
    settings.ALIGN_REPEATS = bool(args.align_repeats)
    if not args.reference:
        _print_error(parser, '--reference is required')
    if args.regions:
        if args.chromosome or args.pattern or args.start is not None or args.end is not None:
            _print_error(parser, '--regions does not go with --chromosome, --pattern, --start or --end')
    else:
        if not args.chromosome:
            _print_error(parser, '--chromosome is required')
        if not args.pattern:
            _print_error(parser, '--pattern is required')
        if not args.start:
            _print_error(parser, '--start is required')
        if not args.end:
            _print_error(parser, '--end is required')
    if args.models is None:
        _print_error(parser, '--models is required')
    try:
        rows = training.parse_regions(args.regions) if args.regions else \
            [(args.chromosome, args.start, args.end, args.pattern, "--chromosome %s --start %d --end %d --pattern %s"
              % (args.chromosome, args.start, args.end, args.pattern))]
        ref = genome.read_genome(args.reference)
        sys.stderr.write("read %d records, %d bases from %s in %.2f s\n" % (len(ref.names()), ref.total_bases(),
                                                                          args.reference, ref.seconds))
        training.check_rows(rows, ref)
    except (OSError, ValueError) as e:
        raise SystemExit("ERROR: %s" % e)
    print('Searching reference genome for regions with shared kmers with VNTR. It takes a few hours for human genome')
    try:
        vntrs = training.add_models(ref, rows, args.models)
    except NotImplementedError as e:
        raise SystemExit("ERROR: %s" % e)
    for v in vntrs:
        print('Training completed. VNTR saved with ID: %s to the database' % v.id)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m advntr_amd")
    sub = ap.add_subparsers(dest="cmd")
    g = sub.add_parser("genotype", help="RU-count genotypes of the given loci from extracted reads (GPU)")
    src = g.add_mutually_exclusive_group(required=True)
    src.add_argument("--loci", help="JSON list of loci")
    src.add_argument("--models", help="sqlite model database in the reference's format (table vntrs)")
    g.add_argument("--vntr-id", type=int, action="append", help="with --models: genotype only these ids")
    g.add_argument("--align-repeats", action="store_true",
                   help="align repeat segments of unequal length with the built-in aligner (instead of refusing them)")
    g.add_argument("--reads", help="FASTA / FASTQ of extracted reads")
    g.add_argument("--alignment", help="BAM file (read on the GPU) or SAM text of the sample: mapped reads over each VNTR are "
                                       "selected as vntr_finder.py:701-750 does, unmapped records are added to --reads")
    g.add_argument("--pacbio", action="store_true", help="reads are trimmed spanning long reads (error rate 0.3); with "
                   "--alignment: the mapped long reads that span each VNTR are trimmed by their CIGAR, the unmapped ones "
                   "(and --reads) are filtered and trimmed by flank alignment (vntr_finder.py:640-651)")
    g.add_argument("--extract-spanning", action="store_true",
                   help="with --pacbio: the reads are whole long reads; find the ones that span each VNTR by aligning its "
                        "flanks (vntr_finder.py:324-371; GPU Smith-Waterman, parity with biopython unpinned) and trim them")
    g.add_argument("--haploid", action="store_true")
    g.add_argument("--accuracy-filter", action="store_true")
    g.add_argument("--min-matches", type=int, default=5)
    g.add_argument("--prefilter-both-strands", action="store_true",
                   help="also run the keyword prefilter on the reverse complement of every read (a superset of the "
                        "reference's candidate reads; the reference scans the reads as given, genome_analyzer.py:173-199)")
    g.add_argument("-fs", "--frameshift", action="store_true",
                   help="search for a frameshift in the VNTR instead of a copy number (vntr_finder.py:256-309)")
    g.add_argument("--outfmt", choices=["text", "bed", "vcf"], default="text",
                   help="result rows as the reference writes them (genome_analyzer.py:28-170)")
    g.add_argument("-e", "--expansion", action="store_true",
                   help="with --alignment: estimate long expansions from PCR-free data as int(RU occurrences / (coverage x "
                        "haplotypes)) for both alleles (vntr_finder.py:879-887); needs -c")
    g.add_argument("-c", "--coverage", type=_coverage_arg, metavar="<float>|auto",
                   help="with -e: average sequencing coverage (0 = the exact genotype), or `auto` to measure it from "
                        "--alignment in the same pass (covered bases per 100-bp window on chr1-22, X, Y, windows above 200x "
                        "left out; with -r the mean of the locus's GC bin, else the sequencing mean)")
    g.add_argument("-r", "--reference-filename", "--reference_filename", dest="reference_filename", metavar="<file>",
                   help="with -e -c auto: the reference genome (FASTA) the alignment was made against; windows are binned "
                        "by its GC content (only uppercase G / C count, as the reference's get_gc_content)")
    a = sub.add_parser("addmodel", add_help=False,
                       help="train a new locus (or every row of --regions) on a reference genome and add it to --models")
    req, other = a.add_argument_group("Required arguments"), a.add_argument_group("Other options")
    req.add_argument("-r", "--reference", help="reference genome (FASTA)")
    req.add_argument("-c", "--chromosome", help="chromosome (e.g. chr1)")
    req.add_argument("-p", "--pattern", help="first repeating pattern of the VNTR in forward (5' to 3') direction")
    req.add_argument("-s", "--start", type=int, help="0-based start of the VNTR")
    req.add_argument("-e", "--end", type=int, help="end of the VNTR")
    req.add_argument("-m", "--models", help="sqlite model database (created when missing)")
    other.add_argument("--regions", help="instead of -c/-p/-s/-e: a file of `chrom start end pattern` rows (0-based start); "
                                         "ids follow the file order, all rows are written in one transaction")
    other.add_argument("--align-repeats", action="store_true",
                       help="align repeat units of unequal length with the built-in aligner (instead of refusing them)")
    other.add_argument("-g", "--gene", help="accepted and stored as NULL, as the reference does")
    other.add_argument("-a", "--annotation", help="accepted and stored as NULL, as the reference does")
    other.add_argument("-h", "--help", action="help", help="show this help message and exit")
    d = sub.add_parser("delmodel", add_help=False, help="remove a locus from --models")
    req, other = d.add_argument_group("Required arguments"), d.add_argument_group("Other options")
    req.add_argument("-vid", "--vntr-id", "--vntr_id", dest="vntr_id", help="VNTR ID")
    req.add_argument("-m", "--models", help="sqlite model database")
    other.add_argument("-h", "--help", action="help", help="show this help message and exit")
    v = sub.add_parser("viewmodel", help="list the loci of --models")
    v.add_argument("-g", "--gene", default="", help="comma-separated list of gene names")
    v.add_argument("-p", "--pattern", help="repeating pattern of the VNTR in forward (5' to 3') direction")
    v.add_argument("-m", "--models", help="sqlite model database")
    args = ap.parse_args(argv)
    if args.cmd == "addmodel":
        return add_model(args, a)
    if args.cmd == "delmodel":
        return del_model(args, d)
    if args.cmd == "viewmodel":
        return view_model(args, v)
    if args.cmd == "genotype":
        if not args.reads and not args.alignment:
            ap.error("genotype needs --reads and/or --alignment")
        if args.expansion:
            if args.coverage is None:
                _print_error(g, 'Please specify the average coverage to identify the expansion')
            if not args.alignment:
                _print_error(g, '--expansion needs --alignment: the coverage method counts the reads of an alignment file')
            if args.pacbio or args.frameshift:
                _print_error(g, '--expansion does not go with %s' % ("--pacbio" if args.pacbio else "--frameshift"))
        if args.alignment and args.frameshift:
            ap.error("--alignment does not go with --frameshift")
        args.comm = None
        try:
            return genotype(args)
        finally:
            if args.comm is not None:
                args.comm.close()
    ap.print_help()
    return 2


if __name__ == "__main__":
    sys.exit(main())
